"""GPU: the exposure chain's kernels (cg_hdr.hip) and cg_rt_render_exposed(_device).

Every comparison is on bit patterns (.view(np.uint32)), tolerance 0, against tests/hdr_ref.py, which
tests/test_hdr.py pins by hand without a GPU.  Output buffers are pre-filled with a NaN pattern no
kernel writes.

* histogram and frame record: plane sizes around the wave, the workgroup step and its tail, 3 and 4
  channels, random and special pixels, frames with a gap of huge values between them, 65,536 pixels
  in one bin, d_stats NULL, a second call into the same outputs;
* the exposure kernel against cg_hdr_exposure, with d_prev NULL and inside an earlier d_scales;
* the pack on random and special pixels with every tone curve, and against cg_rt_render_device;
* cg_rt_render_exposed_device on the lattice, yawed-lattice and large-scene routes, 11 frames (two
  chunks), against hdr_ref applied to the CG_PIX_RGBA_F32 frames of the plain frame calls; the host
  form; plain frames around it; the error returns."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import hdr_ref as ref
import rt_radiance_ref as rref
from cgamd import PIX_RGBA_F32, P

pytestmark = pytest.mark.gpu

CG_E_INVALID, CG_E_NOSCENE = -1, -4
SENTINEL = 0x7FC0DEAD
F = np.float32


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    """A numpy array's bytes on the device, as int32 words."""
    torch, dev = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).to(dev)
    torch.cuda.synchronize()          # the library works on the context's own stream
    return t


def _sentinel(words):
    torch, dev = _torch()
    t = torch.full((words,), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    return t


def _host(t, dtype=np.uint32):
    torch, _ = _torch()
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


# ---- histogram ----------------------------------------------------------------------------------

W_VALUES = np.array([0.0, -0.0, 1.0, 9.0, np.nan, -1.0], np.float32)


def _edge_pixels():
    """Pixels (0, 0, z) whose luminance 0.0722f * z is exactly a bin edge or one of its neighbours
    (a product by a constant cannot reach every float: those that are reached are kept)."""
    out = []
    for e in ref.bin_edge(np.arange(ref.BINS)):
        for target in (np.nextafter(e, F(0)), e, np.nextafter(e, F(np.inf))):
            z = F(target / F(0.0722))
            for _ in range(4):
                z = np.nextafter(z, F(0))
            for _ in range(9):
                if F(F(0.0722) * z) == target:
                    out.append((0.0, 0.0, z))
                    break
                z = np.nextafter(z, F(np.inf))
    return np.array(out, np.float32)


_EDGE = []


def _pixels(rng, n, ch):
    """n pixels: random bit patterns, positive random values, the special values in each channel,
    exact edges; w from W_VALUES."""
    if not len(_EDGE):
        _EDGE.append(_edge_pixels())
        L = ref.luminance(*_EDGE[0].T)
        assert np.isin(ref.bin_edge(np.arange(ref.BINS)), L).sum() > 128      # exact edges are among them
    sp = ref.special_luminances()
    px = ref.random_floats(rng, n * 3).reshape(n, 3)
    kind = rng.integers(0, 5, n)
    pos = ref.from_bits(ref.bits(ref.random_floats(rng, n * 3)) & np.uint32(0x7FFFFFFF)).reshape(n, 3)
    px[kind == 1] = pos[kind == 1]
    k2 = np.flatnonzero(kind == 2)
    px[k2] = np.stack([rng.choice(sp, len(k2)), rng.choice(sp, len(k2)), rng.choice(sp, len(k2))], axis=1)
    k3 = np.flatnonzero(kind == 3)
    px[k3] = _EDGE[0][rng.integers(0, len(_EDGE[0]), len(k3))]
    k4 = np.flatnonzero(kind == 4)                        # grey pixels of moderate size: counted, every bin
    g = ref.from_bits(rng.integers(0x33000000, 0x4A000000, len(k4)).astype(np.uint32))
    px[k4] = np.stack([g, g, g], axis=1)
    if ch == 3:
        return px
    return np.concatenate([px, rng.choice(W_VALUES, n)[:, None]], axis=1).astype(np.float32)


def _run_histogram(ctx, planes, gap, stats=True, out=None):
    """planes float32[n_frames, n, ch] with `gap` pixels of huge values between frames -> (hist
    uint32[n_frames, 256], records, the device outputs)."""
    nf, n, ch = planes.shape
    buf = np.full((nf, n + gap, ch), 3.0e38, np.float32)
    if ch == 4:
        buf[:, :, 3] = 1.0
    buf[:, :n] = planes
    d_px = _dev(buf)
    d_hist, d_stats = out if out is not None else (_sentinel(nf * 256), _sentinel(nf * 8))
    ctx.hdr_histogram_device(d_px.data_ptr(), ch, n, nf, d_hist.data_ptr(), d_stats.data_ptr() if stats else None,
                             frame_stride=n + gap)
    return _host(d_hist).reshape(nf, 256), _host(d_stats).view(cgamd.HDR_STATS_DTYPE), (d_hist, d_stats)


def _check_histogram(hist, recs, planes, what):
    for f, plane in enumerate(planes):
        want_h, want_r = ref.stats_of(plane)
        assert np.array_equal(hist[f], want_h), f"{what} frame {f}: bins {np.flatnonzero(hist[f] != want_h)[:8]}"
        if recs is not None:
            got = {k: int(recs[f][k]) for k in want_r}
            assert got == want_r, f"{what} frame {f}"
            assert not recs[f]["pad"].any()


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_histogram_matches_the_restatement(ctx, n, ch):
    rng = np.random.default_rng(1000 * ch + n)
    planes = np.stack([_pixels(rng, n, ch) for _ in range(3)])
    hist, recs, out = _run_histogram(ctx, planes, gap=5)
    _check_histogram(hist, recs, planes, f"n {n} ch {ch}")
    assert hist.sum() > 0 or n < 63
    # a second call into the same outputs does not accumulate
    hist2, recs2, _ = _run_histogram(ctx, planes, gap=5, out=out)
    _check_histogram(hist2, recs2, planes, f"n {n} ch {ch} (second call)")
    # without a record: the same bins, d_stats untouched
    hist3, recs3, _ = _run_histogram(ctx, planes, gap=5, stats=False)
    _check_histogram(hist3, None, planes, f"n {n} ch {ch} (no record)")
    assert (recs3.view(np.uint32) == SENTINEL).all()


def test_histogram_of_one_bin(ctx):
    """65,536 pixels in one bin: all identical, and all different within the bin."""
    rng = np.random.default_rng(7)
    n = 65536
    same = np.tile(np.array([1, 1, 1, 1], np.float32), (n, 1))
    g = ref.from_bits(rng.integers(0x3F800000, 0x3F880000, n).astype(np.uint32))     # luminance g * 1.0f: bin 128
    spread = np.stack([g, g, g, np.ones(n, np.float32)], axis=1)
    planes = np.stack([same, spread])
    hist, recs, _ = _run_histogram(ctx, planes, gap=0)
    _check_histogram(hist, recs, planes, "one bin")
    assert hist[0, 128] == n and hist[0].sum() == n
    assert np.count_nonzero(hist[1]) <= 2 and hist[1].sum() == n
    hist, recs, _ = _run_histogram(ctx, planes[:, :, :3].copy(), gap=3)
    _check_histogram(hist, recs, planes[:, :, :3], "one bin, 3 channels")


# ---- exposure -----------------------------------------------------------------------------------

def test_exposure_kernel_equals_the_host_function(ctx):
    for hists, kw, prev in ref.exposure_cases():
        n = len(hists)
        params = cgamd.hdr_params(**kw)
        d_hist = _dev(hists)
        d_s = _sentinel(2 * n + 1)
        base = d_s.data_ptr()
        if prev is not None:
            d_prev = _dev(np.array([prev], np.float32))
            ctx.hdr_exposure_device(d_hist.data_ptr(), n, params, base, d_prev=d_prev.data_ptr())
        else:
            ctx.hdr_exposure_device(d_hist.data_ptr(), n, params, base)
        first = _host(d_s)[:n].copy()
        want = cgamd.hdr_exposure(hists, params, prev=prev)
        assert np.array_equal(first, want.view(np.uint32)), (kw, prev)
        assert np.array_equal(want.view(np.uint32), ref.exposure(hists, prev=prev, **kw).view(np.uint32))
        # d_prev inside the earlier call's d_scales: its last element, the outputs right behind it
        ctx.hdr_exposure_device(d_hist.data_ptr(), n, params, base + 4 * n, d_prev=base + 4 * (n - 1))
        got = _host(d_s)
        assert np.array_equal(got[:n], first)
        want2 = cgamd.hdr_exposure(hists, params, prev=float(first.view(np.float32)[n - 1]))
        assert np.array_equal(got[n:2 * n], want2.view(np.uint32)), (kw, "prev inside d_scales")
        assert got[2 * n] == SENTINEL


def test_exposure_kernel_over_more_frames_than_one_pass(ctx):
    """600 frames: three passes of the kernel's 256-frame stage, the chain running through them."""
    rng = np.random.default_rng(11)
    hists = ref.random_histograms(rng, 600)
    params = cgamd.hdr_params(permille=950, target=0.5, scale_min=2.0 ** -14, scale_max=2.0 ** 14, rate=0.3)
    d_hist, d_s = _dev(hists), _sentinel(601)
    ctx.hdr_exposure_device(d_hist.data_ptr(), 600, params, d_s.data_ptr())
    got = _host(d_s)
    assert np.array_equal(got[:600], cgamd.hdr_exposure(hists, params).view(np.uint32)) and got[600] == SENTINEL


# ---- pack ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", [ref.TONE_LINEAR, ref.TONE_REINHARD, ref.TONE_REINHARD_WHITE])
def test_pack_matches_the_restatement(ctx, op):
    rng = np.random.default_rng(20 + op)
    n, nf, sgap, dgap = 1031, 3, 3, 7
    planes = np.stack([_pixels(rng, n, 4) for _ in range(nf)])
    planes[0, :64, :3] = rng.random((64, 3), np.float32) * F(3.0)          # ordinary radiance too
    scales = np.array([1.0, 0.37, 5.5], np.float32)
    src = np.full((nf, n + sgap, 4), 3.0e38, np.float32)
    src[:, :n] = planes
    d_src, d_scales, d_out = _dev(src), _dev(scales), _sentinel(nf * (n + dgap))
    ctx.rt_tonemap_pack_device(d_src.data_ptr(), n, nf, d_scales.data_ptr(), d_out.data_ptr(), op, 7.5,
                               src_stride=n + sgap, dst_stride=n + dgap)
    got = _host(d_out).reshape(nf, n + dgap)
    assert (got[:, n:] == SENTINEL).all()
    for f in range(nf):
        want = ref.pack(planes[f], scales[f], op, 7.5)
        bad = np.flatnonzero(got[f, :n] != want)
        assert bad.size == 0, (f, planes[f, bad[0]], hex(got[f, bad[0]]), hex(want[bad[0]]))


def _rows(H):
    """Rows of a whole frame as the plain frame calls store it (padded to the default stripe)."""
    return cgamd.load().cg_rt_shard_rows(H, None)


def _room(ctx):
    rref.scene("room").set(ctx)
    return rref.scene("room")


def test_linear_pack_of_scale_one_is_the_plain_frame(ctx):
    torch, dev = _torch()
    _room(ctx)
    cam = cgamd.rt_camera(96, 60, 60.0)
    n, padded = 96 * 60, 96 * _rows(60)
    rad, plain, out = _sentinel(padded * 4), _sentinel(padded), _sentinel(n)
    ones = _dev(np.ones(1, np.float32))
    ctx.rt_render_frames_device([cam], rad.data_ptr(), pix_format=PIX_RGBA_F32)
    ctx.rt_render_device(cam, plain.data_ptr())
    ctx.rt_tonemap_pack_device(rad.data_ptr(), n, 1, ones.data_ptr(), out.data_ptr())
    assert np.array_equal(_host(out), _host(plain)[:n])
    assert (_host(plain)[:n] != 0x80000000).sum() > n // 4


# ---- cg_rt_render_exposed_device ----------------------------------------------------------------

N_FRAMES = 11
EXPOSED = {   # name: (scene, width, height, focal, R, route, tone op, white2)
    "room": ("room", 96, 60, 60.0, None, "lattice", ref.TONE_LINEAR, 1.0),
    "room_yaw": ("room", 96, 60, 60.0, rref.YAW, "lattice_yaw", ref.TONE_REINHARD_WHITE, 6.0),
    "rand200": ("rand200", 64, 64, 64.0, None, "big_lattice", ref.TONE_REINHARD, 1.0),
}
KW = dict(permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16, rate=0.5)


def _script(name):
    scene, W, H, focal, R, route, op, white2 = EXPOSED[name]
    Rm = (C.c_float * 16)(*R) if R is not None else None
    cams = [cgamd.rt_camera(W, H, focal, (float(F(0.02 * f)), 0.0, float(F(-3.0 + 0.03 * f)), 1.0), Rm)
            for f in range(N_FRAMES)]
    lights = [rref.light_array([((0.0, -0.5, -0.7, 1.0), (float(F(14.0 + 9.0 * f)),) * 3)]) for f in range(N_FRAMES)]
    return cams, lights, op, white2


def _radiance_frames(ctx, cams, lights, per_frame):
    W, H = cams[0].width, cams[0].height
    padded = W * _rows(H)
    buf = _sentinel(len(cams) * padded * 4)
    if per_frame:
        ctx.rt_render_sequence_device(cams, lights, buf.data_ptr(), pix_format=PIX_RGBA_F32)
    else:
        ctx.rt_render_frames_device(cams, buf.data_ptr(), lights=lights[0], pix_format=PIX_RGBA_F32)
    return _host(buf, np.float32).reshape(len(cams), padded, 4)[:, :W * H].copy()


def _plain(ctx, cam, lights):
    out = _sentinel(cam.width * _rows(cam.height))
    ctx.rt_render_device(cam, out.data_ptr(), lights=lights)
    return _host(out)[:cam.width * cam.height].copy()


@pytest.mark.parametrize("per_frame", [True, False], ids=["sequence", "frames"])
@pytest.mark.parametrize("name", list(EXPOSED))
def test_exposed_frames_match_the_restatement(ctx, name, per_frame):
    scene, W, H = EXPOSED[name][:3]
    sc = rref.scene(scene)
    sc.set(ctx)
    cams, lights, op, white2 = _script(name)
    assert cgamd.rt_route(cams[0], sc.n, sc.n_sph, 1) == EXPOSED[name][5]
    assert cgamd.rt_route(cams[-1], sc.n, sc.n_sph, 1) == EXPOSED[name][5]
    px, gap = W * H, 13
    before = _plain(ctx, cams[0], lights[0])
    rad = _radiance_frames(ctx, cams, lights, per_frame)
    hists = np.stack([ref.stats_of(r)[0] for r in rad])
    want_s = ref.exposure_chunked(hists, **KW)
    assert hists.sum() > px // 4
    if per_frame:
        assert len(set(want_s.tolist())) > 3                            # a script that does adapt
    d_argb, d_s = _sentinel(N_FRAMES * (px + gap)), _sentinel(N_FRAMES + 1)
    params = cgamd.hdr_params(**KW)
    ctx.rt_render_exposed_device(cams, d_argb.data_ptr(), d_s.data_ptr(), params, lights=lights if per_frame else lights[0],
                                 per_frame_lights=per_frame, op=op, white2=white2, frame_stride=px + gap)
    got_s = _host(d_s)
    got = _host(d_argb).reshape(N_FRAMES, px + gap)
    assert np.array_equal(got_s[:N_FRAMES], want_s.view(np.uint32)), (got_s[:N_FRAMES].view(np.float32), want_s)
    assert got_s[N_FRAMES] == SENTINEL and (got[:, px:] == SENTINEL).all()
    for f in range(N_FRAMES):
        want = ref.pack(rad[f], want_s[f], op, white2)
        bad = np.flatnonzero(got[f, :px] != want)
        assert bad.size == 0, f"frame {f}: {bad.size} pixels, first {bad[:4]}"
    assert want_s[8] == want_s[7]                                       # a chunk's first frame shows the scale before it
    # the host form is the device form
    hf, hs = ctx.rt_render_exposed(cams, lights if per_frame else lights[0], per_frame, op=op, white2=white2, **KW)
    assert np.array_equal(hs.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(hf.reshape(N_FRAMES, px), got[:, :px])
    # a previous scale, on the device and on the host
    d_prev = _dev(np.array([0.03125], np.float32))
    ctx.rt_render_exposed_device(cams[:3], d_argb.data_ptr(), d_s.data_ptr(), params, lights=lights[:3] if per_frame else lights[0],
                                 per_frame_lights=per_frame, d_prev=d_prev.data_ptr(), op=op, white2=white2)
    want_p = ref.exposure_chunked(hists[:3], prev=0.03125, **KW)
    assert np.array_equal(_host(d_s)[:3], want_p.view(np.uint32))
    assert np.array_equal(_host(d_argb)[:px], ref.pack(rad[0], F(0.03125), op, white2))
    _, hs = ctx.rt_render_exposed(cams[:3], lights[:3] if per_frame else lights[0], per_frame, prev=0.03125, op=op,
                                  white2=white2, **KW)
    assert np.array_equal(hs.view(np.uint32), want_p.view(np.uint32))
    # plain frames around it are unchanged
    assert np.array_equal(_plain(ctx, cams[0], lights[0]), before)
    if name == "room" and per_frame:
        sat = lambda a: int((((a >> 16) & 255 == 255) | ((a >> 8) & 255 == 255) | (a & 255 == 255)).sum())
        print(f"pixels with a channel of 255: exposed {sat(got[0, :px])}, plain {sat(before)}, scale {want_s[0]}")
        assert sat(got[0, :px]) < sat(before), "exposure leaves fewer saturated pixels than the plain frame"


def test_exposed_before_a_scene_and_bad_arguments(ctx):
    _room(ctx)
    lib = ctx.lib
    cam = cgamd.rt_camera(32, 30, 30.0)
    cams = (cgamd.RtCamera * 2)(cam, cam)
    lights = cgamd.default_lights()
    n = 32 * 30
    d_argb, d_s, d_hist, d_rad = _sentinel(2 * n), _sentinel(4), _sentinel(512), _sentinel(2 * n * 4)
    host_argb, host_s = np.zeros(2 * n, np.uint32), np.zeros(2, np.float32)

    def exposed(ctx_=ctx, n_frames=2, op=0, white2=1.0, argb=d_argb.data_ptr(), scales=d_s.data_ptr(), stride=0,
                cams_=cams, **kw):
        p = cgamd.hdr_params(**kw)
        return lib.cg_rt_render_exposed_device(ctx_.h, lights, 1, cams_, n_frames, 0, C.byref(p), None, op, white2,
                                               P(argb), stride, P(scales), None)

    def exposed_host(ctx_=ctx, n_frames=2, op=0, white2=1.0, argb=host_argb, scales=host_s, stride=0, **kw):
        p = cgamd.hdr_params(**kw)
        return lib.cg_rt_render_exposed(ctx_.h, lights, 1, cams, n_frames, 0, C.byref(p), None, op, white2,
                                        argb.ctypes.data_as(P) if argb is not None else None, stride,
                                        scales.ctypes.data_as(P) if scales is not None else None, None)
    bad_params = [dict(permille=-1), dict(permille=1001), dict(rate=-0.5), dict(rate=1.5), dict(scale_min=2.0, scale_max=1.0)]
    for call in (exposed, exposed_host):
        assert call() == 0
        for kw in bad_params:
            assert call(**kw) == CG_E_INVALID, kw
        assert call(op=3) == CG_E_INVALID and call(op=-1) == CG_E_INVALID
        assert call(op=2, white2=0.0) == CG_E_INVALID and call(op=2, white2=-1.0) == CG_E_INVALID
        assert call(op=1, white2=0.0) == 0                              # white2 is not used
        assert call(stride=n - 1) == CG_E_INVALID
        assert call(n_frames=-1) == CG_E_INVALID
        assert call(argb=None) == CG_E_INVALID and call(scales=None) == CG_E_INVALID
    assert exposed(scales=d_s.data_ptr() + 2) == CG_E_INVALID           # misaligned
    other = (cgamd.RtCamera * 2)(cam, cgamd.rt_camera(32, 31, 30.0))
    assert exposed(cams_=other) == CG_E_INVALID                         # one size a call
    # n_frames == 0: CG_OK, nothing touched
    assert exposed(n_frames=0, argb=None, scales=None) == 0
    sent = _sentinel(8)
    assert exposed(n_frames=0, argb=sent.data_ptr(), scales=sent.data_ptr()) == 0
    assert (_host(sent) == SENTINEL).all()

    hist = lambda ch=4, px=d_rad.data_ptr(), npx=n, nf=2, stride=0, h=d_hist.data_ptr(): lib.cg_hdr_histogram_device(
        ctx.h, P(px), ch, npx, nf, stride, P(h), None, None)
    assert hist() == 0
    assert hist(ch=2) == CG_E_INVALID and hist(ch=5) == CG_E_INVALID
    assert hist(px=None) == CG_E_INVALID and hist(h=None) == CG_E_INVALID
    assert hist(px=d_rad.data_ptr() + 4) == CG_E_INVALID                # 4-float pixels: 16-byte aligned
    assert hist(ch=3, px=d_rad.data_ptr() + 4) == 0
    assert hist(ch=3, px=d_rad.data_ptr() + 2) == CG_E_INVALID
    assert hist(stride=n - 1) == CG_E_INVALID and hist(nf=-1) == CG_E_INVALID
    assert hist(nf=0, px=None, h=None) == 0
    expo = lambda nf=2, h=d_hist.data_ptr(), s=d_s.data_ptr(), prev=None, **kw: lib.cg_hdr_exposure_device(
        ctx.h, P(h), nf, C.byref(cgamd.hdr_params(**kw)), P(prev) if prev else None, P(s), None)
    assert expo() == 0
    for kw in bad_params:
        assert expo(**kw) == CG_E_INVALID, kw
    assert expo(h=None) == CG_E_INVALID and expo(s=None) == CG_E_INVALID and expo(nf=-1) == CG_E_INVALID
    assert expo(s=d_s.data_ptr() + 1) == CG_E_INVALID and expo(prev=d_s.data_ptr() + 2) == CG_E_INVALID
    assert expo(nf=0, h=None, s=None) == 0
    assert lib.cg_hdr_exposure_device(ctx.h, P(d_hist.data_ptr()), 2, None, None, P(d_s.data_ptr()), None) == CG_E_INVALID
    pack = lambda op=0, w2=1.0, src=d_rad.data_ptr(), npx=n, nf=2, ss=0, s=d_s.data_ptr(), dst=d_argb.data_ptr(), ds=0: \
        lib.cg_rt_tonemap_pack_device(ctx.h, P(src), npx, nf, ss, P(s), op, w2, P(dst), ds, None)
    assert pack() == 0
    assert pack(op=3) == CG_E_INVALID and pack(op=2, w2=0.0) == CG_E_INVALID and pack(op=2, w2=float("nan")) == CG_E_INVALID
    assert pack(src=None) == CG_E_INVALID and pack(dst=None) == CG_E_INVALID and pack(s=None) == CG_E_INVALID
    assert pack(src=d_rad.data_ptr() + 8) == CG_E_INVALID
    assert pack(ss=n - 1) == CG_E_INVALID and pack(ds=n - 1) == CG_E_INVALID and pack(nf=-1) == CG_E_INVALID
    assert pack(nf=0, src=None, dst=None, s=None) == 0
    torch, _ = _torch()
    torch.cuda.synchronize()
    with cgamd.Context(0) as fresh:
        assert exposed(ctx_=fresh) == CG_E_NOSCENE
        assert exposed_host(ctx_=fresh) == CG_E_NOSCENE
