"""GPU: the device PNG encoder (cg_image_encode_png_device, cg_image_encode_png) against the
hashes of tests/golden/png_enc_cases.json, files that zlib and Pillow accept
(tests/test_png_encode.py holds the host encoder and the numpy restatement to the same hashes
without a GPU).  Output buffers are pre-filled with 0xA5, and every byte that is not part of a file
must still hold it afterwards."""
import hashlib
import json
import os

import numpy as np
import pytest

import cgamd
import make_png_enc_cases as mk
import png_enc_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_enc_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
GROUPS = mk.groups()
FILL = 0xA5
TAIL = 256
A = ref.ADAPTIVE


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _frames_dev(frames, stride=0, gap_value=0x00FF00FF):
    """uint32 frames (n, H, W) on the device, `stride` pixels apart (0: packed), as an int32 tensor."""
    torch, dev = _torch()
    n, h, w = frames.shape
    stride = stride or h * w
    buf = np.full((n, stride), gap_value, np.uint32)
    buf[:, :h * w] = frames.reshape(n, -1)
    t = torch.from_numpy(buf.view(np.int32).reshape(-1).copy()).to(dev)
    torch.cuda.synchronize()
    return t


def _encode(ctx, frames, colour, filt, slot_bytes, stride=0, stream=None, d_in=None):
    """One device call: (the output tensor of n slots and a tail, d_bytes).  Not synchronised."""
    torch, dev = _torch()
    n, h, w = frames.shape
    d_in = d_in if d_in is not None else _frames_dev(frames, stride)
    d_out = torch.full((n * slot_bytes + TAIL,), FILL, dtype=torch.uint8, device=dev)
    d_bytes = torch.full((n,), -777, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.image_encode_png_device(d_in.data_ptr(), w, h, n, d_out.data_ptr(), slot_bytes, d_bytes.data_ptr(), colour, filt,
                                frame_stride=stride, stream=stream)
    return d_out, d_bytes, d_in


def _check(d_out, d_bytes, slot_bytes, names, what):
    """Every slot against the golden of its name (None: the slot must report CG_E_CAPACITY and be untouched)."""
    torch, _ = _torch()
    torch.cuda.synchronize()
    out, lens = d_out.cpu().numpy(), d_bytes.cpu().numpy()
    for f, name in enumerate(names):
        slot = out[f * slot_bytes:(f + 1) * slot_bytes]
        if name is None:
            assert lens[f] == cgamd.CG_E_CAPACITY, f"{what} frame {f}: d_bytes {lens[f]}"
            assert (slot == FILL).all(), f"{what} frame {f}: bytes written to a slot that reported CG_E_CAPACITY"
            continue
        want = GOLDEN[name]
        assert lens[f] == want["length"], f"{what} {name}: d_bytes {lens[f]} != {want['length']}"
        assert _sha(slot[:lens[f]]) == want["sha256"], f"{what} {name}: bytes differ from the contract's"
        assert (slot[lens[f]:] == FILL).all(), f"{what} {name}: bytes written past the file's end"
    assert (out[len(names) * slot_bytes:] == FILL).all(), f"{what}: bytes written past the last slot"


def _names(h, w, contents, colour, filt):
    return [mk.case_name(h, w, c, colour, filt) for c in contents]


@pytest.mark.parametrize("size", list(mk.SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_matches_goldens(ctx, size):
    """Every case: the contents of a (size, colour, filter) are the frames of one call."""
    h, w = size
    for (gh, gw, colour, filt), contents in GROUPS.items():
        if (gh, gw) != size:
            continue
        frames = np.stack([mk.inputs(h, w, c, colour) for c in contents])
        slot = cgamd.image_png_bound(w, h, colour)
        d_out, d_bytes, _ = _encode(ctx, frames, colour, filt, slot)
        _check(d_out, d_bytes, slot, _names(h, w, contents, colour, filt), f"c{colour} f{filt}")


def test_the_big_cases_cross_the_kernels_limits():
    """From the library's constants: bands longer than a piece, a dynamic block longer than the
    window, a stored band of more than one block."""
    threads, window = cgamd.image_png_enc_limits()
    assert 16 * (1 + 3 * 65) > threads and 5 * (1 + 3 * 64) < threads
    _, bands = ref.info(mk.inputs(20, 900, "nibble", ref.RGB), ref.RGB, A)
    assert not bands[0]["stored"] and bands[0]["dyn_bits"] > 8 * window
    assert GOLDEN[mk.case_name(17, 1400, "noise", ref.RGB, A)]["stored_bands"] == 2 and 16 * (1 + 3 * 1400) > 65535


def test_nine_frames_cross_the_scratch_chunk(ctx):
    """9 frames: the context's scratch holds 8, so the call runs two chunks."""
    h, w = 33, 7
    contents = [GROUPS[(h, w, ref.RGB, A)][k % 7] for k in range(9)]
    frames = np.stack([mk.inputs(h, w, c, ref.RGB) for c in contents])
    slot = cgamd.image_png_bound(w, h, ref.RGB)
    d_out, d_bytes, _ = _encode(ctx, frames, ref.RGB, A, slot)
    _check(d_out, d_bytes, slot, _names(h, w, contents, ref.RGB, A), "9 frames")


def test_frame_stride_with_gap_pixels(ctx):
    h, w = 17, 5
    contents = ("patch", "hgrad", "noise")
    for colour in mk.COLOURS:
        frames = np.stack([mk.inputs(h, w, c, colour) for c in contents])
        slot = 1024
        d_out, d_bytes, _ = _encode(ctx, frames, colour, A, slot, stride=h * w + 37)
        _check(d_out, d_bytes, slot, _names(h, w, contents, colour, A), f"strided c{colour}")


def test_slot_too_small_for_the_middle_frame(ctx):
    """Gradient, noise, constant: a slot that holds the outer two and not the noise.  The middle
    frame reports CG_E_CAPACITY and leaves its slot as it was; the neighbours are exact and nothing
    follows their last byte."""
    h, w = 40, 65
    contents = ("hgrad", "noise", "constant")
    for colour in mk.COLOURS:
        frames = np.stack([mk.inputs(h, w, c, colour) for c in contents])
        names = _names(h, w, contents, colour, A)
        lens = [GOLDEN[n]["length"] for n in names]
        assert lens[1] > max(lens[0], lens[2]) + 1
        for slot in (max(lens[0], lens[2]), lens[1] - 1):
            d_out, d_bytes, _ = _encode(ctx, frames, colour, A, slot)
            _check(d_out, d_bytes, slot, [names[0], None, names[2]], f"slot {slot} c{colour}")
        d_out, d_bytes, _ = _encode(ctx, frames, colour, A, lens[1])       # exactly enough
        _check(d_out, d_bytes, lens[1], names, f"slot {lens[1]} c{colour}")


def test_two_contexts_on_two_streams_at_once(ctx):
    """The scratch is one set per context: two contexts, each on a stream of the caller's, enqueued
    back to back and read after one synchronisation."""
    torch, _ = _torch()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca, cb = GROUPS[(40, 65, ref.RGB, A)], GROUPS[(33, 7, ref.RGBA, 4)]
    a = np.stack([mk.inputs(40, 65, c, ref.RGB) for c in ca])
    b = np.stack([mk.inputs(33, 7, c, ref.RGBA) for c in cb])
    slot_a, slot_b = cgamd.image_png_bound(65, 40, ref.RGB), cgamd.image_png_bound(7, 33, ref.RGBA)
    with cgamd.Context(0) as other:
        d_a, d_b = _frames_dev(a), _frames_dev(b)
        ra = _encode(ctx, a, ref.RGB, A, slot_a, stream=s1.cuda_stream, d_in=d_a)
        rb = _encode(other, b, ref.RGBA, 4, slot_b, stream=s2.cuda_stream, d_in=d_b)
        _check(ra[0], ra[1], slot_a, _names(40, 65, ca, ref.RGB, A), "stream 1")
        _check(rb[0], rb[1], slot_b, _names(33, 7, cb, ref.RGBA, 4), "stream 2")


def test_scratch_reuse_larger_then_smaller_and_back(ctx):
    for (h, w, colour) in [(40, 65, ref.RGBA), (1, 1, ref.RGB), (20, 900, ref.RGB), (2, 1, ref.RGBA), (40, 65, ref.RGBA)]:
        frames = np.stack([mk.inputs(h, w, "patch", colour)])
        slot = cgamd.image_png_bound(w, h, colour)
        d_out, d_bytes, _ = _encode(ctx, frames, colour, A, slot)
        _check(d_out, d_bytes, slot, _names(h, w, ["patch"], colour, A), f"{h}x{w}")


def test_host_memory_form_equals_the_host_function(ctx):
    for (h, w, content, colour, filt) in [(33, 7, "patch", ref.RGB, 3), (17, 1400, "noise", ref.RGBA, A), (1, 1, "constant", ref.RGB, A),
                                          (17, 1400, "fib", ref.RGB, 0)]:
        argb = mk.inputs(h, w, content, colour)
        want = GOLDEN[mk.case_name(h, w, content, colour, filt)]
        data = ctx.image_encode_png(argb, colour, filt)
        assert (len(data), _sha(data)) == (want["length"], want["sha256"])
        assert data == cgamd.image_encode_png_host(argb, colour, filt)


def test_refusals_and_no_frames(ctx):
    torch, dev = _torch()
    t = torch.zeros(4096, dtype=torch.int64, device=dev)
    p = t.data_ptr()
    for kw in [dict(width=0), dict(height=65536), dict(colour=0), dict(colour=4), dict(filter=5), dict(filter=-2),
               dict(n_frames=-1), dict(d_argb=0), dict(d_out=0), dict(d_bytes=0), dict(d_bytes=p + 4), dict(frame_stride=63)]:
        a = dict(d_argb=p, width=8, height=8, n_frames=1, d_out=p + 1024, slot_bytes=1024, d_bytes=p + 8192, colour=ref.RGB,
                 filter=A, frame_stride=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.image_encode_png_device(**a)
    ctx.image_encode_png_device(p, 8, 8, 0, p + 1024, 1024, p + 8192)    # no frames: nothing happens
    torch.cuda.synchronize()
    assert not t.cpu().numpy().any()


def test_nothing_live_after_destroy():
    base = cgamd.debug_live()
    with cgamd.Context(0) as c:
        frames = np.stack([mk.inputs(33, 7, "patch", ref.RGB)])
        slot = cgamd.image_png_bound(7, 33, ref.RGB)
        d_out, d_bytes, _ = _encode(c, frames, ref.RGB, A, slot)
        _check(d_out, d_bytes, slot, _names(33, 7, ["patch"], ref.RGB, A), "own context")
        assert c.image_encode_png(frames[0]) == bytes(d_out.cpu().numpy()[:int(d_bytes.cpu()[0])])
        assert cgamd.debug_live() != base
    assert cgamd.debug_live() == base
