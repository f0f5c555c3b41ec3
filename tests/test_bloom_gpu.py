"""GPU: the bloom kernels (cg_bloom.hip) and the exposed calls with bloom.

Every comparison is on bit patterns, tolerance 0, against tests/bloom_ref.py, which tests/test_bloom.py
pins by hand without a GPU.  Output buffers are pre-filled with a NaN pattern no kernel writes, and the
words between strided frames must still hold it afterwards.

* cg_hdr_bloom_device and cg_hdr_bloom_pack_device over the contract's size list and the sizes
  around the kernels' tiles, levels 1, 2 and 6, three frames a call with gaps of huge values and NaN
  between them, per-frame scales from device memory; special scales; more frames than one batch of
  scratch; a second call into the same outputs at another size; the refusals;
* cg_rt_render_exposed_bloom(_device) on the lattice, yawed-lattice and large-scene routes and
  cg_rast_draw_exposed_bloom(_device) on the dense and compact routes, 11 frames (two chunks),
  against bloom_ref applied to the float frames of the existing float calls under
  hdr_ref.exposure_chunked's scales; bloom NULL and intensity 0; the host forms; plain frames after."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bloom_ref as bref
import cgamd
import hdr_ref
import oracle
import rt_radiance_ref as rref
from cgamd import P
from test_hdr_gpu import SENTINEL, _dev, _host, _pixels, _plain, _radiance_frames, _sentinel, _torch

pytestmark = pytest.mark.gpu

F = np.float32
CG_E_INVALID = -1
# The blur kernel's tile is 32 x 8 pixels of a level (kBloomTW x kBloomTH, cg_bloom.hip), and W_k =
# (W_{k-1} + 1) / 2.  Frames whose level 1 is a tile less a pixel (31 x 7: 61 x 13 and 62 x 14), exactly
# a tile (32 x 8: 63 x 15 and 64 x 16) and a tile and a pixel (33 x 9: 65 x 17); and the same for level 2
# (31 x 7: 121 x 25 and 124 x 28; 32 x 8: 127 x 31 and 128 x 32; 33 x 9: 129 x 33).  Levels 1 and 2 run here.
TILE_SIZES = [(61, 13), (62, 14), (63, 15), (64, 16), (65, 17), (121, 25), (124, 28), (127, 31), (128, 32), (129, 33)]
TILE_LEVELS = {(31, 7), (32, 8), (33, 9)}
assert {bref.level_sizes(w, h, 1)[0] for w, h in TILE_SIZES[:5]} == TILE_LEVELS
assert {bref.level_sizes(w, h, 2)[1] for w, h in TILE_SIZES[5:]} == TILE_LEVELS
PARAMS = [(1.0, 64.0, 0.25), (0.0, 2.0 ** 64, 2.0 ** 32), (0.5, 0.5, 1.5)]   # threshold, cap, intensity
RULES_OPS = list(itertools.product((bref.RULE_RT, bref.RULE_RAST),
                                   (hdr_ref.TONE_LINEAR, hdr_ref.TONE_REINHARD, hdr_ref.TONE_REINHARD_WHITE)))
WHITE2 = 7.5


def _frames(rng, nf, W, H):
    """nf frames float32[nf, H, W, 4] of test_hdr_gpu's pixels, each with one ordinary bright pixel."""
    fr = np.stack([_pixels(rng, W * H, 4).reshape(H, W, 4) for _ in range(nf)])
    for f in range(nf):
        fr[f].reshape(-1, 4)[rng.integers(0, W * H)] = (3.0, 7.0, 1.5, 1.0)
    return fr


def _run(ctx, frames, scales, bloom, rule, op, gaps=(5, 3, 7), out=None):
    """Both device calls over frames float32[nf, H, W, 4]: (pyramids float32[nf, total + gap, 4] as
    bits, argb uint32[nf, px + gap], the device outputs)."""
    nf, H, W, _ = frames.shape
    px, total = W * H, bref.layout(W, H, bloom.levels)[3]
    sgap, pgap, dgap = gaps
    src = np.empty((nf, px + sgap, 4), np.float32)
    src[:, :, 0::2] = 3.0e38                                  # between frames: huge, NaN, covered
    src[:, :, 1] = np.nan
    src[:, :, 3] = 1.0
    src[:, :px] = frames.reshape(nf, px, 4)
    d_src, d_scales = _dev(src), _dev(np.asarray(scales, np.float32))
    d_pyr, d_argb = out if out is not None else (_sentinel(nf * (total + pgap) * 4), _sentinel(nf * (px + dgap)))
    ctx.hdr_bloom_device(d_src.data_ptr(), W, H, nf, d_scales.data_ptr(), bloom, d_pyr.data_ptr(),
                         src_stride=px + sgap if sgap else 0, pyr_stride=total + pgap if pgap else 0)
    ctx.hdr_bloom_pack_device(d_src.data_ptr(), d_pyr.data_ptr(), W, H, nf, d_scales.data_ptr(), bloom, d_argb.data_ptr(),
                              rule, op, WHITE2, src_stride=px + sgap if sgap else 0,
                              pyr_stride=total + pgap if pgap else 0, dst_stride=px + dgap if dgap else 0)
    pyr = _host(d_pyr)[:nf * (total + pgap) * 4].reshape(nf, total + pgap, 4)
    argb = _host(d_argb)[:nf * (px + dgap)].reshape(nf, px + dgap)
    return pyr, argb, (d_pyr, d_argb)


def _check(pyr, argb, frames, scales, bloom, rule, op, what, prior=None):
    """The device outputs against the restatement; returns whether any U_1 holds a positive value.
    The words between frames hold the sentinel, or what `prior` (the outputs before the call) held."""
    nf, H, W, _ = frames.shape
    px, total = W * H, bref.layout(W, H, bloom.levels)[3]
    lit = False
    for f in range(nf):
        want_pyr, want_px = bref.frame(frames[f], scales[f], bloom.levels, bloom.threshold, bloom.cap, bloom.intensity,
                                       rule, op, WHITE2)
        got = pyr[f, :total].reshape(-1)
        bad = np.flatnonzero(got != want_pyr.view(np.uint32).reshape(-1))
        assert bad.size == 0, f"{what} frame {f}: {bad.size} pyramid words, first {bad[:4]}"
        bad = np.flatnonzero(argb[f, :px] != want_px.reshape(-1))
        assert bad.size == 0, f"{what} frame {f}: {bad.size} pixels, first {bad[:4]}"
        lit = lit or bool((want_pyr[:bref.layout(W, H, 1)[3], :3] > 0).any())
    gap_pyr, gap_argb = (SENTINEL, SENTINEL) if prior is None else (prior[0][:, total:], prior[1][:, px:])
    assert (pyr[:, total:] == gap_pyr).all() and (argb[:, px:] == gap_argb).all(), f"{what}: a gap was written"
    return lit


@pytest.mark.parametrize("W,H", bref.SIZES + TILE_SIZES, ids=[f"{w}x{h}" for w, h in bref.SIZES + TILE_SIZES])
def test_kernels_match_the_restatement(ctx, W, H):
    rng = np.random.default_rng(7000 * W + H)
    frames = _frames(rng, 3, W, H)
    scales = np.array([1.0, 0.37, 5.5], np.float32)
    for i, levels in enumerate((1, 2, 6)):
        thr, cap, inten = PARAMS[(i + W + H) % 3]
        rule, op = RULES_OPS[(2 * i + W + H) % 6]
        bloom = cgamd.hdr_bloom_params(levels, thr, cap, inten)
        pyr, argb, _ = _run(ctx, frames, scales, bloom, rule, op)
        assert _check(pyr, argb, frames, scales, bloom, rule, op, f"{W}x{H} levels {levels}"), "a comparison of zeros"


@pytest.mark.parametrize("rule,op", RULES_OPS)
def test_every_rule_and_curve(ctx, rule, op):
    rng = np.random.default_rng(91)
    frames = _frames(rng, 2, 33, 17)
    frames[0, 2:6, 3:9, :3] = rng.random((4, 6, 3), np.float32) * F(6.0)
    frames[0, 2:6, 3:9, 3] = 1.0
    scales = np.array([1.0, 0.6], np.float32)
    bloom = cgamd.hdr_bloom_params(3)
    pyr, argb, _ = _run(ctx, frames, scales, bloom, rule, op)
    assert _check(pyr, argb, frames, scales, bloom, rule, op, f"rule {rule} op {op}")
    # the host function gives the kernel's words
    assert np.array_equal(cgamd.hdr_bloom(frames[0], 1.0, bloom).view(np.uint32), pyr[0, :pyr.shape[1] - 3])


def test_special_scales_and_unpadded_frames(ctx):
    """Scales of +inf, a negative, NaN and 0 give finite pyramids; strides of 0 mean the planes themselves."""
    rng = np.random.default_rng(17)
    frames = _frames(rng, 5, 65, 63)
    scales = np.array([np.inf, -2.0, np.nan, 0.0, 1.0], np.float32)
    bloom = cgamd.hdr_bloom_params(4, 0.5, 2.0 ** 64, 2.0 ** 32)
    pyr, argb, _ = _run(ctx, frames, scales, bloom, bref.RULE_RT, hdr_ref.TONE_REINHARD, gaps=(0, 0, 0))
    assert _check(pyr, argb, frames, scales, bloom, bref.RULE_RT, hdr_ref.TONE_REINHARD, "special scales")
    assert np.isfinite(pyr.view(np.float32)).all()


def test_more_frames_than_one_batch_of_scratch(ctx):
    """19 frames: the unblurred planes are scratch for 8 frames at a time."""
    rng = np.random.default_rng(23)
    frames = _frames(rng, 19, 33, 17)
    scales = (F(0.25) + F(0.125) * np.arange(19)).astype(np.float32)
    bloom = cgamd.hdr_bloom_params(3, 0.25, 8.0, 0.5)
    pyr, argb, _ = _run(ctx, frames, scales, bloom, bref.RULE_RAST, hdr_ref.TONE_LINEAR)
    assert _check(pyr, argb, frames, scales, bloom, bref.RULE_RAST, hdr_ref.TONE_LINEAR, "19 frames")


def test_level_with_more_tile_rows_than_a_grid_holds(ctx):
    """1 x 1,048,600: level 1 has 65,538 rows of blur tiles, more than the 65,535 a grid dimension
    holds, so workgroups stride over them."""
    rng = np.random.default_rng(31)
    frames = _frames(rng, 1, 1, 1048600)
    frames[0, ::4099, 0, :] = (3.0, 7.0, 1.5, 1.0)
    scales = np.array([1.25], np.float32)
    bloom = cgamd.hdr_bloom_params(2, 1.0, 64.0, 0.25)
    pyr, argb, _ = _run(ctx, frames, scales, bloom, bref.RULE_RT, hdr_ref.TONE_REINHARD)
    assert _check(pyr, argb, frames, scales, bloom, bref.RULE_RT, hdr_ref.TONE_REINHARD, "1 x 1048600")


def test_second_call_at_another_size_and_context_balance():
    """One context of its own: a large size, then a small one into the same outputs (scratch reused
    downward), then a larger one (scratch grows); closing it leaves as many live resources as before."""
    live = cgamd.debug_live
    before = live()
    rng = np.random.default_rng(29)
    scales = np.array([1.0, 0.37, 5.5], np.float32)
    bloom = cgamd.hdr_bloom_params(6)
    with cgamd.Context(0) as c:
        out = None
        for W, H in ((130, 67), (5, 4), (64, 16), (259, 129)):
            frames = _frames(rng, 3, W, H)
            if out is not None and (W, H) == (259, 129):
                out = None                                    # larger than the outputs of the first call
            prior = None
            if out is not None:                               # what the outputs hold, in this call's strides
                total = bref.layout(W, H, 6)[3]
                prior = (_host(out[0])[:3 * (total + 3) * 4].reshape(3, total + 3, 4).copy(),
                         _host(out[1])[:3 * (W * H + 7)].reshape(3, W * H + 7).copy())
            pyr, argb, out = _run(c, frames, scales, bloom, bref.RULE_RT, hdr_ref.TONE_REINHARD, out=out)
            assert _check(pyr, argb, frames, scales, bloom, bref.RULE_RT, hdr_ref.TONE_REINHARD, f"{W}x{H}", prior)
        _torch()[0].cuda.synchronize()
    assert live() == before


def test_device_refusals(ctx):
    lib = ctx.lib
    W, H, nf = 8, 8, 2
    total = bref.layout(W, H, 4)[3]
    d_src, d_pyr, d_argb, d_s = _sentinel(nf * W * H * 4), _sentinel(nf * total * 4), _sentinel(nf * W * H), _dev(np.ones(2, np.float32))

    def bloom(src=d_src.data_ptr(), w=W, h=H, n=nf, ss=0, s=d_s.data_ptr(), pyr=d_pyr.data_ptr(), ps=0, params=True, **kw):
        p = cgamd.hdr_bloom_params(**kw)
        return lib.cg_hdr_bloom_device(ctx.h, P(src), w, h, n, ss, P(s), C.byref(p) if params else None, P(pyr), ps, None)

    def pack(src=d_src.data_ptr(), pyr=d_pyr.data_ptr(), w=W, h=H, n=nf, ss=0, ps=0, s=d_s.data_ptr(), rule=0, op=0,
             white2=1.0, dst=d_argb.data_ptr(), ds=0, params=True, **kw):
        p = cgamd.hdr_bloom_params(**kw)
        return lib.cg_hdr_bloom_pack_device(ctx.h, P(src), P(pyr), w, h, n, ss, ps, P(s), C.byref(p) if params else None,
                                            rule, op, white2, P(dst), ds, None)
    bad = [dict(levels=0), dict(levels=7), dict(threshold=-1.0), dict(threshold=float("nan")), dict(cap=0.0),
           dict(cap=float("nan")), dict(cap=2.0 ** 65), dict(intensity=-1.0), dict(intensity=float("nan")),
           dict(intensity=2.0 ** 33)]
    for call in (bloom, pack):
        assert call() == 0
        for kw in bad:
            assert call(**kw) == CG_E_INVALID, kw
        assert call(params=False) == CG_E_INVALID
        assert call(src=None) == CG_E_INVALID and call(pyr=None) == CG_E_INVALID and call(s=None) == CG_E_INVALID
        assert call(src=d_src.data_ptr() + 8) == CG_E_INVALID and call(pyr=d_pyr.data_ptr() + 4) == CG_E_INVALID
        assert call(s=d_s.data_ptr() + 2) == CG_E_INVALID
        assert call(w=0) == CG_E_INVALID and call(h=-1) == CG_E_INVALID and call(n=-1) == CG_E_INVALID
        assert call(ss=W * H - 1) == CG_E_INVALID and call(ps=total - 1) == CG_E_INVALID
    assert pack(dst=None) == CG_E_INVALID and pack(dst=d_argb.data_ptr() + 2) == CG_E_INVALID
    assert pack(ds=W * H - 1) == CG_E_INVALID
    assert pack(rule=2) == CG_E_INVALID and pack(op=3) == CG_E_INVALID and pack(op=2, white2=0.0) == CG_E_INVALID
    assert lib.cg_hdr_bloom_device(None, P(d_src.data_ptr()), W, H, nf, 0, P(d_s.data_ptr()),
                                   C.byref(cgamd.hdr_bloom_params()), P(d_pyr.data_ptr()), 0, None) == CG_E_INVALID
    # n_frames == 0: CG_OK, nothing touched
    sent = _sentinel(64)
    assert bloom(n=0, src=None, pyr=sent.data_ptr(), s=None) == 0
    assert pack(n=0, src=None, pyr=None, s=None, dst=sent.data_ptr()) == 0
    assert (_host(sent) == SENTINEL).all()


# ---- the exposed calls --------------------------------------------------------------------------

N_FRAMES, W, H, FOCAL = 11, 96, 64, 64.0
KW = dict(permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16, rate=0.5)
RT = {   # name: (scene, R, route, tone op, white2, bloom parameters)
    "room": ("room", None, "lattice", hdr_ref.TONE_REINHARD, 1.0, dict()),            # the defaults, threshold 1.0
    "room_yaw": ("room", rref.YAW, "lattice_yaw", hdr_ref.TONE_REINHARD_WHITE, 6.0, dict(levels=6, threshold=0.5, intensity=0.5)),
    "rand300": ("rand300", None, "big_lattice", hdr_ref.TONE_LINEAR, 1.0, dict(levels=2, threshold=0.25, cap=4.0, intensity=1.0)),
}


def _rt_script(name):
    R = RT[name][1]
    Rm = (C.c_float * 16)(*R) if R is not None else None
    cams = [cgamd.rt_camera(W, H, FOCAL, (float(F(0.02 * f)), 0.0, float(F(-3.0 + 0.03 * f)), 1.0), Rm)
            for f in range(N_FRAMES)]
    lights = [rref.light_array([((0.0, -0.5, -0.7, 1.0), (float(F(14.0 + 9.0 * f)),) * 3)]) for f in range(N_FRAMES)]
    return cams, lights


def _want_frames(rad, scales, bloom, rule, op, white2):
    return [bref.frame(r.reshape(H, W, 4), s, bloom.levels, bloom.threshold, bloom.cap, bloom.intensity, rule, op, white2)[1]
            .reshape(-1) for r, s in zip(rad, scales)]


@pytest.mark.parametrize("per_frame", [True, False], ids=["sequence", "frames"])
@pytest.mark.parametrize("name", list(RT))
def test_rt_exposed_bloom_matches_the_restatement(ctx, name, per_frame):
    scene, _, route, op, white2, bkw = RT[name]
    sc = rref.scene(scene)
    sc.set(ctx)
    cams, lights = _rt_script(name)
    assert cgamd.rt_route(cams[0], sc.n, sc.n_sph, 1) == route and cgamd.rt_route(cams[-1], sc.n, sc.n_sph, 1) == route
    L = lights if per_frame else lights[0]
    px, gap = W * H, 13
    before = _plain(ctx, cams[0], lights[0])
    rad = _radiance_frames(ctx, cams, lights, per_frame)
    hists = np.stack([hdr_ref.stats_of(r)[0] for r in rad])
    want_s = hdr_ref.exposure_chunked(hists, **KW)
    params, bloom = cgamd.hdr_params(**KW), cgamd.hdr_bloom_params(**bkw)
    want = _want_frames(rad, want_s, bloom, bref.RULE_RT, op, white2)

    def device(b, stride=0):
        d_argb, d_s = _sentinel(N_FRAMES * (stride or px)), _sentinel(N_FRAMES + 1)
        ctx.rt_render_exposed_bloom_device(cams, d_argb.data_ptr(), d_s.data_ptr(), params, b, lights=L,
                                           per_frame_lights=per_frame, op=op, white2=white2, frame_stride=stride)
        return _host(d_argb).reshape(N_FRAMES, stride or px), _host(d_s)
    got, got_s = device(bloom, px + gap)
    assert np.array_equal(got_s[:N_FRAMES], want_s.view(np.uint32)) and got_s[N_FRAMES] == SENTINEL
    assert (got[:, px:] == SENTINEL).all()
    for f in range(N_FRAMES):
        bad = np.flatnonzero(got[f, :px] != want[f])
        assert bad.size == 0, f"frame {f}: {bad.size} pixels, first {bad[:4]}"
    # the existing exposed call: its scales, and its frames for bloom NULL and intensity 0
    d_argb, d_s = _sentinel(N_FRAMES * px), _sentinel(N_FRAMES)
    ctx.rt_render_exposed_device(cams, d_argb.data_ptr(), d_s.data_ptr(), params, lights=L, per_frame_lights=per_frame,
                                 op=op, white2=white2)
    plain, plain_s = _host(d_argb).reshape(N_FRAMES, px), _host(d_s)
    assert np.array_equal(plain_s, got_s[:N_FRAMES])
    for b in (None, cgamd.hdr_bloom_params(**dict(bkw, intensity=0.0))):
        f0, s0 = device(b)
        assert np.array_equal(f0, plain) and np.array_equal(s0[:N_FRAMES], plain_s)
    assert (got[:, :px] != plain).any(), "bloom changes the frames"
    # the host form is the device form
    hf, hs = ctx.rt_render_exposed_bloom(cams, bloom, L, per_frame, op=op, white2=white2, **KW)
    assert np.array_equal(hs.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(hf.reshape(N_FRAMES, px), got[:, :px])
    hf, hs = ctx.rt_render_exposed_bloom(cams, None, L, per_frame, op=op, white2=white2, **KW)
    assert np.array_equal(hf.reshape(N_FRAMES, px), plain)
    # plain frames afterwards: unchanged, and the oracle's for the reference scene
    assert np.array_equal(_plain(ctx, cams[0], lights[0]), before)
    if name == "room":
        cam = cgamd.rt_camera(W, H, FOCAL)
        assert np.array_equal(_plain(ctx, cam, None), oracle.rt_draw(oracle.rt_params(W, H, FOCAL)).reshape(-1))


def test_rt_exposed_bloom_refusals(ctx):
    rref.scene("room").set(ctx)
    lib = ctx.lib
    cam = cgamd.rt_camera(32, 30, 30.0)
    cams = (cgamd.RtCamera * 2)(cam, cam)
    lights = cgamd.default_lights()
    d_argb, d_s = _sentinel(2 * 32 * 30), _sentinel(2)
    host_argb, host_s = np.zeros(2 * 32 * 30, np.uint32), np.zeros(2, np.float32)
    p = cgamd.hdr_params()

    def dev(**kw):
        b = cgamd.hdr_bloom_params(**kw)
        return lib.cg_rt_render_exposed_bloom_device(ctx.h, lights, 1, cams, 2, 0, C.byref(p), None, 0, 1.0, C.byref(b),
                                                     P(d_argb.data_ptr()), 0, P(d_s.data_ptr()), None)

    def host(**kw):
        b = cgamd.hdr_bloom_params(**kw)
        return lib.cg_rt_render_exposed_bloom(ctx.h, lights, 1, cams, 2, 0, C.byref(p), None, 0, 1.0, C.byref(b),
                                              host_argb.ctypes.data_as(P), 0, host_s.ctypes.data_as(P), None)
    for call in (dev, host):
        assert call() == 0
        for kw in (dict(levels=0), dict(levels=7), dict(threshold=-1.0), dict(cap=float("nan")), dict(cap=0.0),
                   dict(intensity=2.0 ** 33), dict(intensity=float("nan"))):
            assert call(**kw) == CG_E_INVALID, kw
    _torch()[0].cuda.synchronize()


# the rasteriser: 11 frames with a light move, colour modes 1 and 2, a camera move
RAST_MODES = [0, 0, 0, 1, 1, 2, 2, 0, 0, 1, 0]
RAST_START = 12_000_000
f32 = lambda x: float(np.float32(x))   # noqa: E731


def _rast_script():
    out = []
    for k, mode in enumerate(RAST_MODES):
        light = (f32(0.1 * min(k, 3) - 0.1), -0.5, f32(-0.1 * min(k, 2)), 1.0)
        cam = (f32(0.05 * max(k - 7, 0)), 0.0, f32(-3.001 + 0.15 * max(k - 7, 0)), 1.0)
        out.append(cgamd.rast_params(W, H, FOCAL, cam=cam, light=light, indirect_first=f32(0.15 if k == 0 else 0.2),
                                     colour_mode=mode, rand_offset=RAST_START if k == 0 else 0))
    return out


def _rast_pictures(ctx):
    """The float frames and records of the existing float sequence call."""
    n, px = N_FRAMES, W * H
    d_rgba, d_info = _sentinel(4 * n * px), _sentinel(6 * (n + 1))
    ctx.rast_draw_sequence_picture_device(_rast_script(), d_rgba.data_ptr(), d_info=d_info.data_ptr())
    return _host(d_rgba, np.float32).reshape(n, px, 4).copy(), _host(d_info).view(cgamd.RAST_SEQ_DTYPE).copy()


def _rast_check(ctx, route, op, white2, bkw):
    n, px, gap = N_FRAMES, W * H, 11
    pics, info = _rast_pictures(ctx)
    assert ctx.rast_scratch_info()["route"] == route
    hists = np.stack([hdr_ref.stats_of(r)[0] for r in pics])
    want_s = hdr_ref.exposure_chunked(hists, **KW)
    params, bloom = cgamd.hdr_params(**KW), cgamd.hdr_bloom_params(**bkw)
    want = _want_frames(pics, want_s, bloom, bref.RULE_RAST, op, white2)

    def device(b, stride=0):
        d_argb, d_s, d_info = _sentinel(n * (stride or px)), _sentinel(n + 1), _sentinel(6 * (n + 1))
        ctx.rast_draw_exposed_bloom_device(_rast_script(), d_argb.data_ptr(), d_s.data_ptr(), params, b, d_info.data_ptr(),
                                           op=op, white2=white2, frame_stride=stride)
        return _host(d_argb).reshape(n, stride or px), _host(d_s), _host(d_info).view(cgamd.RAST_SEQ_DTYPE)
    got, got_s, got_info = device(bloom, px + gap)
    assert np.array_equal(got_s[:n], want_s.view(np.uint32)) and got_s[n] == SENTINEL
    assert (got[:, px:] == SENTINEL).all()
    assert got_info.tobytes() == info.tobytes()              # the rand() index passed from chunk to chunk
    for f in range(n):
        bad = np.flatnonzero(got[f, :px] != want[f])
        assert bad.size == 0, f"frame {f}: {bad.size} pixels, first {bad[:4]}"
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert (got[:, :px].reshape(n, H, W)[:, border] == 0).all()    # the border the reference never writes
    d_argb, d_s, d_i = _sentinel(n * px), _sentinel(n), _sentinel(6 * (n + 1))
    ctx.rast_draw_exposed_device(_rast_script(), d_argb.data_ptr(), d_s.data_ptr(), params, d_i.data_ptr(), op=op, white2=white2)
    plain, plain_s = _host(d_argb).reshape(n, px), _host(d_s)
    assert np.array_equal(plain_s, got_s[:n])
    for b in (None, cgamd.hdr_bloom_params(**dict(bkw, intensity=0.0))):
        f0, s0, _ = device(b)
        assert np.array_equal(f0, plain) and np.array_equal(s0[:n], plain_s)
    assert (got[:, :px] != plain).any(), "bloom changes the frames"
    hf, hs, hi, rc = ctx.rast_draw_exposed_bloom(_rast_script(), bloom, op=op, white2=white2, **KW)
    assert rc == cgamd.CG_OK and hi.tobytes() == info.tobytes()
    assert np.array_equal(hs.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(hf.reshape(n, px), got[:, :px])
    return pics, info


def test_rast_exposed_bloom_dense_route(ctx):
    ctx.rast_set_scene()
    _rast_check(ctx, cgamd.RAST_ROUTE_DENSE, hdr_ref.TONE_REINHARD, 1.0, dict())
    # a plain Draw afterwards is still the oracle's frame
    d = _sentinel(W * H)
    ctx.rast_draw_device(cgamd.rast_params(W, H, FOCAL), d.data_ptr())
    assert np.array_equal(_host(d), oracle.rast_draw(oracle.rast_params(W, H, FOCAL))[0].reshape(-1))


def test_rast_exposed_bloom_compact_route(ctx):
    ctx.rast_set_scene()
    ctx.rast_set_route_limit(1)
    try:
        _rast_check(ctx, cgamd.RAST_ROUTE_COMPACT, hdr_ref.TONE_REINHARD_WHITE, 6.25, dict(levels=6, threshold=0.5, intensity=0.5))
    finally:
        ctx.rast_set_route_limit(0)


def test_rast_exposed_bloom_refusals(ctx):
    ctx.rast_set_scene()
    buf = _sentinel(4 * W * H)
    ps = _rast_script()[:2]
    ok = cgamd.hdr_params(**KW)
    for kw in (dict(levels=0), dict(levels=7), dict(threshold=-1.0), dict(cap=0.0), dict(cap=float("nan")),
               dict(intensity=2.0 ** 33), dict(intensity=float("nan"))):
        with pytest.raises(RuntimeError, match=rf"\({CG_E_INVALID}\)"):
            ctx.rast_draw_exposed_bloom_device(ps, buf.data_ptr(), buf.data_ptr(), ok, cgamd.hdr_bloom_params(**kw), buf.data_ptr())
        with pytest.raises(RuntimeError, match=rf"\({CG_E_INVALID}\)"):
            ctx.rast_draw_exposed_bloom(ps, cgamd.hdr_bloom_params(**kw))
    ctx.rast_draw_exposed_bloom_device([], buf.data_ptr(), buf.data_ptr(), ok, cgamd.hdr_bloom_params(), buf.data_ptr())
    assert (_host(buf) == SENTINEL).all()                          # no frames: nothing written


def test_rast_exposed_bloom_flagged_frame(ctx):
    """A rand() stream too small for the larger colour frames: a flagged frame is the all-uncovered
    picture, so its bright pass is dark and its ARGB 0; the host form returns CG_E_CAPACITY."""
    ctx.rast_set_scene()
    _, info = _rast_pictures(ctx)
    shaded = [int(s) for s in info["n_shaded"][:N_FRAMES]]
    cap = min(s for s in shaded if s > 0)
    flagged = [s > cap for s in shaded]
    assert any(flagged)
    n, px = N_FRAMES, W * H
    bloom, params = cgamd.hdr_bloom_params(), cgamd.hdr_params(**KW)
    try:
        ctx.rast_set_rand_capacity(cap)
        pics, info = _rast_pictures(ctx)
        d_argb, d_s, d_info = _sentinel(n * px), _sentinel(n), _sentinel(6 * (n + 1))
        ctx.rast_draw_exposed_bloom_device(_rast_script(), d_argb.data_ptr(), d_s.data_ptr(), params, bloom, d_info.data_ptr(),
                                           op=hdr_ref.TONE_REINHARD)
        got, got_s, got_info = _host(d_argb).reshape(n, px), _host(d_s), _host(d_info).view(cgamd.RAST_SEQ_DTYPE)
        hf, hs, hi, rc = ctx.rast_draw_exposed_bloom(_rast_script(), bloom, op=hdr_ref.TONE_REINHARD, **KW)
    finally:
        ctx.rast_set_rand_capacity(0)
    assert rc == cgamd.CG_E_CAPACITY
    assert [int(x) != 0 for x in got_info["status"][:n]] == flagged
    hists = np.stack([hdr_ref.stats_of(r)[0] for r in pics])
    want_s = hdr_ref.exposure_chunked(hists, **KW)
    assert np.array_equal(got_s, want_s.view(np.uint32)) and np.array_equal(hs.view(np.uint32), got_s)
    want = _want_frames(pics, want_s, bloom, bref.RULE_RAST, hdr_ref.TONE_REINHARD, 1.0)
    for f in range(n):
        assert np.array_equal(got[f], want[f]), f
        assert not flagged[f] or not got[f].any()
    assert np.array_equal(hf.reshape(n, px), got)
