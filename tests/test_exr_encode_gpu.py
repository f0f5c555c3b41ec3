"""GPU: the device EXR encoder (cg_image_encode_exr_device, cg_image_encode_exr) against the hashes
of tests/golden/exr_enc_cases.json, files that the independent reader accepts
(tests/test_exr_encode.py holds the host encoder and the numpy restatement to the same hashes
without a GPU).  Output buffers are pre-filled with 0xA5, and every byte that is not part of a file
must still hold it afterwards."""
import hashlib
import json
import os

import numpy as np
import pytest

import cgamd
import exr_enc_ref as ref
import make_exr_enc_cases as mk

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "exr_enc_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
GROUPS = mk.groups()
FILL = 0xA5
TAIL = 256
DEF = mk.DEFAULT


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _frames_dev(frames, stride=0, gap_value=123.25):
    """float32 pictures (n, H, W, 4) on the device, `stride` pixels apart (0: packed), as an int32 tensor (the bits)."""
    torch, dev = _torch()
    n, h, w, _ = frames.shape
    stride = stride or h * w
    buf = np.full((n, stride, 4), gap_value, np.float32)
    buf[:, :h * w] = frames.reshape(n, h * w, 4)
    t = torch.from_numpy(buf.view(np.int32).reshape(-1).copy()).to(dev)
    torch.cuda.synchronize()
    return t


def _encode(ctx, frames, prm, slot_bytes, alpha=1.0, stride=0, stream=None, d_in=None):
    """One device call: (the output tensor of n slots and a tail, d_bytes, the input).  Not synchronised."""
    torch, dev = _torch()
    n, h, w, _ = frames.shape
    d_in = d_in if d_in is not None else _frames_dev(frames, stride)
    d_out = torch.full((n * slot_bytes + TAIL,), FILL, dtype=torch.uint8, device=dev)
    d_bytes = torch.full((n,), -777, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.image_encode_exr_device(d_in.data_ptr(), w, h, n, d_out.data_ptr(), slot_bytes, d_bytes.data_ptr(), prm[0], prm[1], prm[2],
                                alpha, frame_stride=stride, stream=stream)
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


def _names(h, w, contents, prm):
    return [mk.case_name(h, w, c, *prm) for c in contents]


def _by_alpha(contents):
    """The contents of a group split by the alpha scale their goldens were made with: one call each."""
    out = {}
    for c in contents:
        out.setdefault(mk.alpha_of(c), []).append(c)
    return out.items()


@pytest.mark.parametrize("size", list(mk.SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_matches_goldens(ctx, size):
    """Every case: the contents of a (size, channels, type, compression) are the frames of a call
    (the picture-like patch, whose alpha scale is 1/9, in a call of its own)."""
    h, w = size
    for (gh, gw, *prm), contents in GROUPS.items():
        if (gh, gw) != size:
            continue
        for alpha, part in _by_alpha(contents):
            frames = np.stack([mk.inputs(h, w, c, prm[1]) for c in part])
            slot = cgamd.image_exr_bound(w, h, prm[0], prm[1])
            d_out, d_bytes, _ = _encode(ctx, frames, prm, slot, alpha)
            _check(d_out, d_bytes, slot, _names(h, w, part, prm), f"{prm}")


def test_the_specials_frame_on_the_device(ctx):
    """The device conversion meets every special value, in every component and both types: the
    reader returns numpy's halves, and the floats bit for bit."""
    px = mk.inputs(17, 5, "specials")
    for typ in (ref.HALF, ref.FLOAT):
        for comp in (ref.NONE, ref.ZIP):
            data = ctx.image_encode_exr(px, ref.RGBA, typ, comp, 1.0)
            mk.accepted(data, px, ref.RGBA, typ, comp, 1.0)


def test_the_big_cases_cross_the_kernels_limits():
    threads, window = cgamd.image_exr_enc_limits()
    assert 16 * 7 * 8 < threads < 16 * 9 * 8
    _, notes = ref.info(mk.inputs(20, 900, "patch"), alpha_scale=mk.PATCH_ALPHA)
    assert not notes[0]["raw"] and notes[0]["bytes"] > window
    assert GOLDEN[mk.case_name(40, 65, "mixed", *DEF)]["raw_chunks"] == 1


def test_nine_frames_cross_the_scratch_chunk(ctx):
    """9 frames: the context's scratch holds 8, so the call runs two chunks."""
    h, w = 33, 7
    pool = [c for c in GROUPS[(h, w) + DEF] if c != "patch"]
    contents = [pool[k % len(pool)] for k in range(9)]
    frames = np.stack([mk.inputs(h, w, c) for c in contents])
    slot = cgamd.image_exr_bound(w, h, ref.RGBA, ref.HALF)
    d_out, d_bytes, _ = _encode(ctx, frames, DEF, slot)
    _check(d_out, d_bytes, slot, _names(h, w, contents, DEF), "9 frames")


def test_frame_stride_with_gap_pixels(ctx):
    h, w = 17, 5
    contents = ("specials", "hgrad", "noise")
    for prm in (DEF, (ref.RGB, ref.FLOAT, ref.ZIP), (ref.RGBA, ref.FLOAT, ref.NONE)):
        frames = np.stack([mk.inputs(h, w, c, prm[1]) for c in contents])
        slot = 2048
        d_out, d_bytes, _ = _encode(ctx, frames, prm, slot, stride=h * w + 37)
        _check(d_out, d_bytes, slot, _names(h, w, contents, prm), f"strided {prm}")


def test_slot_too_small_for_the_middle_frame(ctx):
    """Gradient, noise, constant: a slot that holds the outer two and not the noise.  The middle
    frame reports CG_E_CAPACITY and leaves its slot as it was; the neighbours are exact and nothing
    follows their last byte."""
    h, w = 40, 65
    contents = ("hgrad", "noise", "constant")
    frames = np.stack([mk.inputs(h, w, c) for c in contents])
    names = _names(h, w, contents, DEF)
    lens = [GOLDEN[n]["length"] for n in names]
    assert lens[1] > max(lens[0], lens[2]) + 1
    for slot in (max(lens[0], lens[2]), lens[1] - 1):
        d_out, d_bytes, _ = _encode(ctx, frames, DEF, slot)
        _check(d_out, d_bytes, slot, [names[0], None, names[2]], f"slot {slot}")
    d_out, d_bytes, _ = _encode(ctx, frames, DEF, lens[1])       # exactly enough
    _check(d_out, d_bytes, lens[1], names, f"slot {lens[1]}")
    # NONE: every file has the bound's length; one byte less refuses all three
    prm = (ref.RGBA, ref.HALF, ref.NONE)
    h, w = 17, 5
    frames = np.stack([mk.inputs(h, w, c) for c in contents])
    bound = cgamd.image_exr_bound(w, h, ref.RGBA, ref.HALF)
    d_out, d_bytes, _ = _encode(ctx, frames, prm, bound - 1)
    _check(d_out, d_bytes, bound - 1, [None, None, None], "NONE, a byte short")


def test_two_contexts_on_two_streams_at_once(ctx):
    """The scratch is one set per context: two contexts, each on a stream of the caller's, enqueued
    back to back and read after one synchronisation."""
    torch, _ = _torch()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pa, pb = DEF, (ref.RGB, ref.FLOAT, ref.ZIP)
    ca = [c for c in GROUPS[(40, 65) + pa] if c != "patch"]
    cb = [c for c in GROUPS[(33, 7) + pb] if c != "patch"]
    a = np.stack([mk.inputs(40, 65, c, pa[1]) for c in ca])
    b = np.stack([mk.inputs(33, 7, c, pb[1]) for c in cb])
    slot_a, slot_b = cgamd.image_exr_bound(65, 40, pa[0], pa[1]), cgamd.image_exr_bound(7, 33, pb[0], pb[1])
    with cgamd.Context(0) as other:
        d_a, d_b = _frames_dev(a), _frames_dev(b)
        ra = _encode(ctx, a, pa, slot_a, stream=s1.cuda_stream, d_in=d_a)
        rb = _encode(other, b, pb, slot_b, stream=s2.cuda_stream, d_in=d_b)
        _check(ra[0], ra[1], slot_a, _names(40, 65, ca, pa), "stream 1")
        _check(rb[0], rb[1], slot_b, _names(33, 7, cb, pb), "stream 2")


def test_scratch_reuse_larger_then_smaller_and_back(ctx):
    for (h, w) in [(40, 65), (1, 1), (20, 900), (1, 2), (40, 65)]:
        frames = np.stack([mk.inputs(h, w, "hgrad")])
        slot = cgamd.image_exr_bound(w, h, ref.RGBA, ref.HALF)
        d_out, d_bytes, _ = _encode(ctx, frames, DEF, slot)
        _check(d_out, d_bytes, slot, _names(h, w, ["hgrad"], DEF), f"{h}x{w}")


def test_host_memory_form_equals_the_host_function(ctx):
    for (h, w, content, prm) in [(33, 7, "patch", (ref.RGB, ref.HALF, ref.ZIP)), (17, 1400, "noise", (ref.RGBA, ref.FLOAT, ref.ZIP)),
                                 (1, 1, "constant", DEF), (17, 1400, "patch", (ref.RGBA, ref.FLOAT, ref.ZIP)),
                                 (33, 7, "specials", (ref.RGBA, ref.HALF, ref.NONE))]:
        px, alpha = mk.inputs(h, w, content, prm[1]), mk.alpha_of(content)
        want = GOLDEN[mk.case_name(h, w, content, *prm)]
        data = ctx.image_encode_exr(px, *prm, alpha)
        assert (len(data), _sha(data)) == (want["length"], want["sha256"])
        assert data == cgamd.image_encode_exr_host(px, *prm, alpha)


def test_refusals_and_no_frames(ctx):
    torch, dev = _torch()
    t = torch.zeros(4096, dtype=torch.int64, device=dev)
    p = t.data_ptr()
    for kw in [dict(width=0), dict(height=65536), dict(channels=2), dict(channels=5), dict(type=0), dict(type=3), dict(compression=1),
               dict(compression=4), dict(alpha_scale=float("inf")), dict(alpha_scale=float("nan")), dict(n_frames=-1), dict(d_rgba=0),
               dict(d_rgba=p + 8), dict(d_out=0), dict(d_bytes=0), dict(d_bytes=p + 16384 + 4), dict(frame_stride=63)]:
        a = dict(d_rgba=p, width=8, height=8, n_frames=1, d_out=p + 2048, slot_bytes=2048, d_bytes=p + 16384, channels=ref.RGBA,
                 type=ref.HALF, compression=ref.ZIP, alpha_scale=1.0, frame_stride=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.image_encode_exr_device(**a)
    ctx.image_encode_exr_device(p, 8, 8, 0, p + 2048, 2048, p + 16384)    # no frames: nothing happens
    torch.cuda.synchronize()
    assert not t.cpu().numpy().any()


def test_nothing_live_after_destroy():
    base = cgamd.debug_live()
    with cgamd.Context(0) as c:
        frames = np.stack([mk.inputs(33, 7, "hgrad")])
        slot = cgamd.image_exr_bound(7, 33, ref.RGBA, ref.HALF)
        d_out, d_bytes, _ = _encode(c, frames, DEF, slot)
        _check(d_out, d_bytes, slot, _names(33, 7, ["hgrad"], DEF), "own context")
        assert c.image_encode_exr(frames[0]) == bytes(d_out.cpu().numpy()[:int(d_bytes.cpu()[0])])
        assert cgamd.debug_live() != base
    assert cgamd.debug_live() == base
