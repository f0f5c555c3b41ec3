"""GPU: the device JPEG encoder (cg_image_encode_jpeg_device, cg_image_encode_jpeg) against the
bytes Pillow writes, which travel as the hashes of tests/golden/jpeg_enc_cases.json
(tests/test_jpeg_encode.py holds the host encoder and the numpy restatement to the same hashes
without a GPU).  Output buffers are pre-filled with 0xA5, and every byte that is not part of a file
must still hold it afterwards."""
import hashlib
import json
import os

import numpy as np
import pytest

import cgamd
import jpeg_enc_ref as ref
import make_jpeg_enc_cases as mk
import oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "jpeg_enc_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
FILL = 0xA5
TAIL = 256


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


def _encode(ctx, frames, quality, sub, slot_bytes, stride=0, stream=None, d_in=None):
    """One device call: (the output tensor of n slots and a tail, d_bytes).  Not synchronised."""
    torch, dev = _torch()
    n, h, w = frames.shape
    d_in = d_in if d_in is not None else _frames_dev(frames, stride)
    d_out = torch.full((n * slot_bytes + TAIL,), FILL, dtype=torch.uint8, device=dev)
    d_bytes = torch.full((n,), -777, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.image_encode_jpeg_device(d_in.data_ptr(), w, h, n, d_out.data_ptr(), slot_bytes, d_bytes.data_ptr(), quality, sub,
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
        assert _sha(slot[:lens[f]]) == want["sha256"], f"{what} {name}: bytes differ from Pillow's"
        assert (slot[lens[f]:] == FILL).all(), f"{what} {name}: bytes written past the file's end"
    assert (out[len(names) * slot_bytes:] == FILL).all(), f"{what}: bytes written past the last slot"


@pytest.mark.parametrize("size", list(mk.SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_matches_goldens(ctx, size):
    """Every case: the four contents of a size are the four frames of one call per quality and subsampling."""
    h, w = size
    frames = np.stack([mk.inputs(h, w, c) for c in mk.CONTENTS])
    d_in = _frames_dev(frames)
    for q in mk.QUALITIES:
        for sub in mk.SUBSAMPLINGS:
            slot = cgamd.image_jpeg_bound(w, h, sub)
            d_out, d_bytes, _ = _encode(ctx, frames, q, sub, slot, d_in=d_in)
            _check(d_out, d_bytes, slot, [mk.case_name(h, w, c, q, sub) for c in mk.CONTENTS], f"q{q} s{sub}")


def test_more_frames_than_a_chunk_of_scratch(ctx):
    """11 frames: the context's scratch holds 8, so the call runs two chunks."""
    h, w = 17, 33
    contents = [mk.CONTENTS[k % 4] for k in range(11)]
    frames = np.stack([mk.inputs(h, w, c) for c in contents])
    slot = cgamd.image_jpeg_bound(w, h, 2)
    d_out, d_bytes, _ = _encode(ctx, frames, 75, 2, slot)
    _check(d_out, d_bytes, slot, [mk.case_name(h, w, c, 75, 2) for c in contents], "11 frames")


def test_three_frames_with_a_frame_stride(ctx):
    h, w = 31, 15
    contents = ("random", "gradient", "noise")
    frames = np.stack([mk.inputs(h, w, c) for c in contents])
    for sub in mk.SUBSAMPLINGS:
        slot = 4096
        d_out, d_bytes, _ = _encode(ctx, frames, 90, sub, slot, stride=h * w + 37)
        _check(d_out, d_bytes, slot, [mk.case_name(h, w, c, 90, sub) for c in contents], f"strided s{sub}")


def test_slot_too_small_for_the_middle_frame(ctx):
    """Gradient, noise, constant at Q = 100: a slot that holds the outer two and not the noise.  The
    middle frame reports CG_E_CAPACITY and leaves its slot as it was; the neighbours are exact and
    nothing follows their last byte."""
    h, w = 20, 35
    contents = ("gradient", "noise", "constant")
    frames = np.stack([mk.inputs(h, w, c) for c in contents])
    for sub in mk.SUBSAMPLINGS:
        lens = [GOLDEN[mk.case_name(h, w, c, 100, sub)]["length"] for c in contents]
        assert lens[1] > max(lens[0], lens[2]) + 1
        for slot in (max(lens[0], lens[2]), lens[1] - 1):
            d_out, d_bytes, _ = _encode(ctx, frames, 100, sub, slot)
            names = [mk.case_name(h, w, c, 100, sub) for c in contents]
            _check(d_out, d_bytes, slot, [names[0], None, names[2]], f"slot {slot} s{sub}")
        d_out, d_bytes, _ = _encode(ctx, frames, 100, sub, lens[1])       # exactly enough
        _check(d_out, d_bytes, lens[1], names, f"slot {lens[1]} s{sub}")


def test_interval_larger_than_a_round_and_than_the_window(ctx):
    """16 x 1100 at 4:4:4: one restart interval has more blocks than the entropy workgroup has
    lanes, and with 0/255 noise at Q = 100 it is longer than the window of it the workgroup holds in
    LDS, so both the rounds of blocks and the moving window run.  Both from the library's constants."""
    h, w = 16, 1100
    threads, stage_bytes = cgamd.image_jpeg_enc_limits()
    assert -(-w // 8) * 3 > threads
    frames = np.stack([mk.inputs(h, w, "noise"), mk.inputs(h, w, "random")])
    longest = max(len(iv) for iv in ref.intervals(frames[0], 100, 0))
    print(f"lanes {threads}, window {stage_bytes} B, blocks per interval {-(-w // 8) * 3}, longest interval {longest} B")
    assert longest > stage_bytes
    slot = cgamd.image_jpeg_bound(w, h, 0)
    d_out, d_bytes, _ = _encode(ctx, frames, 100, 0, slot)
    _check(d_out, d_bytes, slot, [mk.case_name(h, w, c, 100, 0) for c in ("noise", "random")], "16x1100")


def test_two_contexts_on_two_streams_at_once(ctx):
    """The scratch is one set per context: two contexts, each on a stream of the caller's, enqueued
    back to back and read after one synchronisation."""
    torch, _ = _torch()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = np.stack([mk.inputs(150, 40, c) for c in mk.CONTENTS])
    b = np.stack([mk.inputs(88, 24, c) for c in mk.CONTENTS])
    slot_a, slot_b = cgamd.image_jpeg_bound(40, 150, 2), cgamd.image_jpeg_bound(24, 88, 0)
    with cgamd.Context(0) as other:
        d_a, d_b = _frames_dev(a), _frames_dev(b)
        ra = _encode(ctx, a, 75, 2, slot_a, stream=s1.cuda_stream, d_in=d_a)
        rb = _encode(other, b, 90, 0, slot_b, stream=s2.cuda_stream, d_in=d_b)
        _check(ra[0], ra[1], slot_a, [mk.case_name(150, 40, c, 75, 2) for c in mk.CONTENTS], "stream 1")
        _check(rb[0], rb[1], slot_b, [mk.case_name(88, 24, c, 90, 0) for c in mk.CONTENTS], "stream 2")


def test_scratch_reuse_smaller_then_larger(ctx):
    for (h, w, sub) in [(8, 8, 0), (150, 40, 2), (8, 8, 0), (16, 1100, 0), (2, 3, 2)]:
        frames = np.stack([mk.inputs(h, w, "random")])
        slot = cgamd.image_jpeg_bound(w, h, sub)
        d_out, d_bytes, _ = _encode(ctx, frames, 50, sub, slot)
        _check(d_out, d_bytes, slot, [mk.case_name(h, w, "random", 50, sub)], f"{h}x{w}")


def test_host_memory_form(ctx):
    for (h, w, content, q, sub) in [(17, 33, "random", 75, 2), (88, 24, "noise", 100, 0), (1, 1, "constant", 10, 2)]:
        want = GOLDEN[mk.case_name(h, w, content, q, sub)]
        data = ctx.image_encode_jpeg(mk.inputs(h, w, content), q, sub)
        assert (len(data), _sha(data)) == (want["length"], want["sha256"])


def test_refusals(ctx):
    torch, dev = _torch()
    t = torch.zeros(4096, dtype=torch.int64, device=dev)
    p = t.data_ptr()
    for kw in [dict(width=0), dict(height=65536), dict(quality=0), dict(quality=101), dict(subsampling=1),
               dict(n_frames=-1), dict(d_argb=0), dict(d_out=0), dict(d_bytes=0), dict(d_bytes=p + 4), dict(frame_stride=63)]:
        a = dict(d_argb=p, width=8, height=8, n_frames=1, d_out=p + 1024, slot_bytes=1024, d_bytes=p + 8192, quality=75,
                 subsampling=0, frame_stride=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.image_encode_jpeg_device(**a)
    ctx.image_encode_jpeg_device(p, 8, 8, 0, p + 1024, 1024, p + 8192)    # no frames: nothing happens
    torch.cuda.synchronize()
    assert not t.cpu().numpy().any()


def test_nothing_live_after_destroy():
    base = cgamd.debug_live()
    with cgamd.Context(0) as c:
        frames = np.stack([mk.inputs(17, 33, "random")])
        slot = cgamd.image_jpeg_bound(33, 17, 2)
        d_out, d_bytes, _ = _encode(c, frames, 75, 2, slot)
        _check(d_out, d_bytes, slot, [mk.case_name(17, 33, "random", 75, 2)], "own context")
        assert c.image_encode_jpeg(frames[0], 75, 2) == bytes(d_out.cpu().numpy()[:int(d_bytes.cpu()[0])])
        assert cgamd.debug_live() != base
    assert cgamd.debug_live() == base


def test_library_decodes_its_own_products_as_the_oracle_does(ctx):
    for sub in mk.SUBSAMPLINGS:
        data = ctx.image_encode_jpeg(mk.inputs(17, 33, "random"), 90, sub)
        got, want = ctx.decode_jpeg(data), oracle.jpeg_decode(data)
        assert got.shape == want.shape == (17, 33, 3) and np.array_equal(got, want)
