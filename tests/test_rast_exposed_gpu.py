"""GPU: cg_rast_draw_exposed(_device) -- a rasteriser key script drawn, exposed and tone mapped on
the device -- against the restated chain: tests/rast_picture_ref.py's pictures at the oracle's own
rand() chain, hdr_ref's histograms and exposure_chunked over them, the restated rasteriser pack.
Every comparison is on bit patterns, tolerance 0.

The script has 17 frames (two full chunks of 8 and one frame more) with a light move, colour-mode
switches and a camera move; runs of 1, 8, 9 and 17 frames are its prefixes, so one set of restated
pictures serves every case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cgamd
import hdr_ref
import rast_big_scenes as sc
import rast_picture_ref as pref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FC0DEAD
W, H, FOCAL = 66, 42, 36.0
START = 12_000_000
#        light moves -> <- mode 1, 2 ->  camera moves ->      <- mode 1 again
MODES = [0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0, 1, 0, 2, 0, 0, 1]
f32 = lambda x: float(np.float32(x))   # noqa: E731


def _script():
    out = []
    for k, mode in enumerate(MODES):
        light = (f32(0.1 * min(k, 3) - 0.1), -0.5, f32(-0.1 * min(k, 2)), 1.0)
        cam = (f32(0.05 * max(k - 7, 0)), 0.0, f32(-3.001 + 0.15 * max(k - 7, 0)), 1.0)
        out.append(cgamd.rast_params(W, H, FOCAL, cam=cam, light=light, indirect_first=f32(0.15 if k == 0 else 0.2),
                                     colour_mode=mode, rand_offset=START if k == 0 else 0))
    return out


@functools.lru_cache(maxsize=None)
def _restated():
    """(pictures float32[17, H*W, 4], histograms, records, the index each frame starts at + the
    closing one, shaded fragments) from the oracle alone."""
    pics, hists, recs, offs, shaded, off = [], [], [], [], [], START
    for p in _script():
        q = sc.oracle_params(p)
        q.rand_offset = off
        rgba, full, checks = pref.picture(q)
        assert pref.clean(checks), checks
        h, r = hdr_ref.stats_of(rgba.reshape(-1, 4))
        pics.append(rgba.reshape(-1, 4)), hists.append(h), recs.append(r), offs.append(off)
        shaded.append(full["n_shaded"] if p.colour_mode else -1)
        if p.colour_mode:
            off += 3 * full["n_shaded"]
    pics = np.stack(pics)
    pics.setflags(write=False)
    return pics, np.stack(hists), recs, offs + [off], shaded


def _torch():
    import torch
    return torch


def _sentinel(words):
    torch = _torch()
    t = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()              # the library works on the context's own stream
    return t


def _host(t, dtype=np.uint32):
    _torch().cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at {bad[:4]}: {got[bad[:4]]} != {want[bad[:4]]}"


EXPO = dict(permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16)


def _want(n, rate, prev, op, white2):
    pics, hists, _, offs, shaded = _restated()
    scales = hdr_ref.exposure_chunked(hists[:n], rate=rate, prev=prev, **EXPO)
    frames = np.stack([pref.pack(pics[f], scales[f], op, white2) for f in range(n)])
    return frames, scales, offs[:n + 1], shaded[:n]


def _device_run(ctx, n, rate, prev, op, white2, stride=0):
    px = W * H
    st = stride or px
    d_argb, d_scales, d_info = _sentinel(n * st), _sentinel(n), _sentinel(6 * (n + 1))
    d_prev = None
    if prev is not None:
        d_prev = _torch().tensor([prev], dtype=_torch().float32, device="cuda")
        _torch().cuda.synchronize()
    ctx.rast_draw_exposed_device(_script()[:n], d_argb.data_ptr(), d_scales.data_ptr(),
                                 cgamd.hdr_params(rate=rate, **EXPO), d_info.data_ptr(),
                                 d_prev=d_prev.data_ptr() if d_prev is not None else None, op=op, white2=white2,
                                 frame_stride=stride)
    return (_host(d_argb).reshape(n, st), _host(d_scales, np.float32), _host(d_info).view(cgamd.RAST_SEQ_DTYPE))


CASES = [   # frames, rate, previous scale, curve, white2
    (1, 1.0, None, hdr_ref.TONE_LINEAR, 1.0),
    (8, 0.25, 2.0, hdr_ref.TONE_REINHARD, 1.0),
    (9, 0.25, None, hdr_ref.TONE_REINHARD_WHITE, 6.25),
    (17, 0.25, 0.5, hdr_ref.TONE_REINHARD, 1.0),
    (17, 1.0, None, hdr_ref.TONE_LINEAR, 1.0),
]


def _check(got, n, rate, prev, op, white2, what):
    frames, scales, info = got
    want_frames, want_scales, offs, shaded = _want(n, rate, prev, op, white2)
    assert [int(x) for x in info["rand_offset"]] == offs, what
    assert [int(x) for x in info["n_shaded"]] == shaded + [-1], what
    assert not info["status"].any(), what
    _same(scales, want_scales, f"{what}: scales")
    for f in range(n):
        _same(frames[f, :W * H], want_frames[f], f"{what}: frame {f}")


@pytest.mark.parametrize("n,rate,prev,op,white2", CASES)
def test_exposed_device_matches_the_restated_chain(ctx, n, rate, prev, op, white2):
    ctx.rast_set_scene()
    stride = W * H + 19 if n == 9 else 0
    got = _device_run(ctx, n, rate, prev, op, white2, stride)
    _check(got, n, rate, prev, op, white2, f"{n} frames")
    if stride:
        assert (got[0][:, W * H:] == SENTINEL).all()                  # the gap of a stride is never written
    if n == 17:   # the chain did something: scales differ between frames, frames differ from the plain ones
        assert len(set(got[1].tolist())) > 3
        assert (got[0][16] != pref.pack(_restated()[0][16], 1.0)).any()


@pytest.mark.parametrize("n,rate,prev,op,white2", CASES[1:4])
def test_exposed_host_form_equals_the_device_form(ctx, n, rate, prev, op, white2):
    ctx.rast_set_scene()
    frames, scales, info, rc = ctx.rast_draw_exposed(_script()[:n], rate=rate, prev=prev, op=op, white2=white2, **EXPO)
    assert rc == cgamd.CG_OK
    _check((frames.reshape(n, -1), scales, info), n, rate, prev, op, white2, f"host form, {n} frames")


def test_exposed_compact_route_gives_the_dense_frames_and_scales(ctx):
    ctx.rast_set_scene()
    n, rate, prev, op, white2 = CASES[3]
    ctx.rast_set_route_limit(1)
    try:
        got = _device_run(ctx, n, rate, prev, op, white2)
        assert ctx.rast_scratch_info()["route"] == cgamd.RAST_ROUTE_COMPACT
    finally:
        ctx.rast_set_route_limit(0)
    _check(got, n, rate, prev, op, white2, "compact route")


def test_exposed_second_call_allocates_nothing():
    with cgamd.Context(0) as c:
        c.rast_set_scene()
        n, rate, prev, op, white2 = CASES[3]
        _device_run(c, n, rate, prev, op, white2)
        first = c.rast_scratch_info()["bytes"]
        assert first >= 8 * W * H * 16                               # the chunk's float frames are counted
        got = _device_run(c, n, rate, prev, op, white2)
        assert c.rast_scratch_info()["bytes"] == first
        _check(got, n, rate, prev, op, white2, "second call")
        _device_run(c, 3, rate, prev, op, white2)                    # fewer frames: nothing grows either
        assert c.rast_scratch_info()["bytes"] == first


def test_histogram_records_of_float_frames(ctx):
    """cg_hdr_histogram_device, unchanged, on the float sequence: the border is uncovered, pixels
    whose luminance is not positive are dark."""
    ctx.rast_set_scene()
    n, px = 9, W * H
    pics, hists, recs, _, _ = _restated()
    d_rgba, d_info = _sentinel(4 * n * px), _sentinel(6 * (n + 1))
    ctx.rast_draw_sequence_picture_device(_script()[:n], d_rgba.data_ptr(), d_info=d_info.data_ptr())
    d_hist, d_stats = _sentinel(n * 256), _sentinel(n * 8)
    ctx.hdr_histogram_device(d_rgba.data_ptr(), 4, px, n, d_hist.data_ptr(), d_stats.data_ptr())
    _same(_host(d_rgba), pics[:n], "float frames")
    assert np.array_equal(_host(d_hist).reshape(n, 256), hists[:n])
    got = _host(d_stats).view(cgamd.HDR_STATS_DTYPE)
    for f in range(n):
        assert {k: int(got[f][k]) for k in recs[f]} == recs[f], f
        assert int(got[f]["n_uncovered"]) == 2 * W + 2 * H - 4
    assert sum(r["n_dark"] for r in recs[:n]) > 0                    # dark pixels are in play


def test_exposed_flagged_frame(ctx):
    """A rand() stream too small for the larger colour frames: a flagged frame is the all-uncovered
    picture -- an empty histogram, t = 1.0 clamped, ARGB 0 -- the device form still returns CG_OK and
    the host form CG_E_CAPACITY after delivering everything."""
    ctx.rast_set_scene()
    n, rate, op, white2 = 17, 0.25, hdr_ref.TONE_REINHARD, 1.0
    pics, hists, _, offs, shaded = _restated()
    cap = min(s for s in shaded[:n] if s > 0)       # the frames before the camera moves fit, the closer ones do not
    flagged = [s > cap for s in shaded[:n]]
    assert any(flagged) and sum(flagged) < sum(s > 0 for s in shaded[:n])
    h = hists[:n].copy()
    h[flagged] = 0
    scales = hdr_ref.exposure_chunked(h, rate=rate, prev=None, **EXPO)
    try:
        ctx.rast_set_rand_capacity(cap)
        frames, got_scales, info = _device_run(ctx, n, rate, None, op, white2)
        hf, hs, hi, rc = ctx.rast_draw_exposed(_script()[:n], rate=rate, op=op, white2=white2, **EXPO)
    finally:
        ctx.rast_set_rand_capacity(0)
    assert rc == cgamd.CG_E_CAPACITY
    assert [int(x) for x in info["status"]] == [cgamd.CG_E_CAPACITY if f else 0 for f in flagged] + [0]
    assert [int(x) for x in info["rand_offset"]] == offs[:n + 1]
    _same(got_scales, scales, "scales with flagged frames")
    _same(hs, scales, "host scales with flagged frames")
    assert hi.tobytes() == info.tobytes()
    for f in range(n):
        want = np.zeros(W * H, np.uint32) if flagged[f] else pref.pack(pics[f], scales[f], op, white2)
        _same(frames[f], want, f"frame {f}")
        _same(hf[f], want, f"host frame {f}")


LANES_CHILD = """
import sys
sys.path[:0] = [{pkg!r}, {oracle!r}, {tests!r}]
import numpy as np
import cgamd
import test_rast_exposed_gpu as t
with cgamd.Context(0) as c:
    c.rast_set_scene()
    frames, scales, info, rc = c.rast_draw_exposed(t._script(), rate=0.25, prev=0.5, op=1, **t.EXPO)
    assert rc == 0
    np.savez({out!r}, frames=frames, scales=scales, info=info)
"""


def test_exposed_frames_do_not_depend_on_the_lanes(tmp_path):
    """CG_RAST_SEQ_LANES is read once a process: a child with one lane (every frame on the call's
    own stream) delivers the frames, scales and records of the default six."""
    out = str(tmp_path / "lanes1.npz")
    env = dict(os.environ, CG_RAST_SEQ_LANES="1")
    code = LANES_CHILD.format(pkg=os.path.join(ROOT, "computer-graphics_amd"), oracle=os.path.join(ROOT, "oracle"),
                              tests=os.path.join(ROOT, "tests"), out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    n, rate, prev, op, white2 = CASES[3]
    _check((z["frames"].reshape(n, -1), z["scales"], z["info"]), n, rate, prev, op, white2, "one lane")


def test_exposed_argument_errors(ctx):
    inv, nos = f"({cgamd.CG_E_INVALID})", f"({cgamd.CG_E_NOSCENE})"
    buf = _sentinel(4 * W * H)
    ps = _script()[:2]
    ok = cgamd.hdr_params(**EXPO)

    def rc(fn):
        with pytest.raises(RuntimeError) as e:
            fn()
        return str(e.value)
    args = (buf.data_ptr(), buf.data_ptr())
    with cgamd.Context(0) as fresh:
        assert nos in rc(lambda: fresh.rast_draw_exposed_device(ps, *args, ok, buf.data_ptr()))
        assert nos in rc(lambda: fresh.rast_draw_exposed(ps))
    ctx.rast_set_scene()
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, *args, cgamd.hdr_params(permille=1001), buf.data_ptr()))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, *args, cgamd.hdr_params(rate=1.5), buf.data_ptr()))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, *args, ok, buf.data_ptr(), op=9))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, *args, ok, buf.data_ptr(), op=hdr_ref.TONE_REINHARD_WHITE,
                                                          white2=0.0))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, *args, ok, None))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, None, buf.data_ptr(), ok, buf.data_ptr()))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device(ps, *args, ok, buf.data_ptr(), frame_stride=W * H - 1))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device([ps[0], cgamd.rast_params(W, H + 1, FOCAL)], *args, ok,
                                                          buf.data_ptr()))
    assert inv in rc(lambda: ctx.rast_draw_exposed_device([cgamd.rast_params(W, H, FOCAL, colour_mode=3)], *args, ok,
                                                          buf.data_ptr()))
    ctx.rast_draw_exposed_device([], *args, ok, buf.data_ptr())       # no frames: nothing written
    assert (_host(buf) == SENTINEL).all()
