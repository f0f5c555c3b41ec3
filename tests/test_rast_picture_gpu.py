"""GPU: the rasteriser's float picture (CG_PIX_RGBA_F32) and its pack.

Every comparison is on bit patterns, tolerance 0.  The expected picture is tests/rast_picture_ref.py's
restatement over the oracle's planes (tests/test_rast_picture.py holds its self-checks on the CPU);
output buffers are pre-filled with a NaN pattern no kernel writes.

* cg_rast_draw_picture against the restatement, and LINEAR at scale 1 of the device picture against
  cg_rast_draw, with its depth and shadow planes: 3x3 (one interior pixel), 66x10, 67x45, 96x64 and
  130x136 (widths that are no multiple of the 64-pixel tile, heights that are no multiple of 8, 17
  tile rows), colour modes 0-2, indirect_first 0.15 and 0.2, a yawed R, on the dense route and on
  the compact route (cg_rast_set_route_limit(ctx, 1)); the reference's grill and woven-wood JPEGs;
  a caller's room and boxes at 96x48;
* cg_rast_draw_sequence_picture_device: 9 frames of mixed modes on lanes, the records of
  cg_rast_draw_sequence_device, every frame its single-frame picture at the chained index, the gap
  of a frame stride untouched; with a small rand() capacity a flagged frame is all zeros and the
  later frames stay exact;
* cg_rast_tonemap_pack_device against cg_rast_pack_pixel on rendered and synthetic planes."""
import functools

import numpy as np
import pytest

import cgamd
import hdr_ref
import oracle
import rast_big_scenes as sc
import rast_picture_ref as pref

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD
F = np.float32
f32 = lambda x: float(np.float32(x))   # noqa: E731


def _torch():
    import torch
    return torch


def _sentinel(words):
    torch = _torch()
    t = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()              # the library works on the context's own stream
    return t


def _dev(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype=np.uint32):
    _torch().cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at {bad[:4]}: {got[bad[:4]]} != {want[bad[:4]]}"


# ---- single frames ------------------------------------------------------------------------------

YAW = 0.35
FRAMES = {   # name: (W, H, focal, rast_params keywords)
    "3x3": (3, 3, 2.0, {}),
    "66x10": (66, 10, 12.0, {}),
    "67x45": (67, 45, 40.0, {}),
    "67x45-indirect": (67, 45, 40.0, dict(indirect_first=f32(0.15), cam=(0.2, -0.1, -2.6, 1.0))),
    "96x64": (96, 64, 48.0, {}),
    "96x64-mode1": (96, 64, 48.0, dict(colour_mode=1, rand_offset=12_000_000)),
    "96x64-mode2": (96, 64, 48.0, dict(colour_mode=2, rand_offset=12_000_017)),
    "67x45-mode1": (67, 45, 40.0, dict(colour_mode=1, rand_offset=5)),
    "96x64-yaw": (96, 64, 48.0, dict(yaw=YAW)),
    "130x136": (130, 136, 70.0, {}),
}


def _params(name):
    W, H, focal, kw = FRAMES[name]
    kw = dict(kw)
    if "yaw" in kw:
        kw["R"] = cgamd.yaw_matrix(kw["yaw"])
    return cgamd.rast_params(W, H, focal, **kw)


def _oracle_params(p, setting=0, boxes=0):
    po = sc.oracle_params(p)
    po.setting, po.setting_boxes = setting, boxes
    return po


@functools.lru_cache(maxsize=None)
def _expected(name):
    rgba, full, checks = pref.picture(_oracle_params(_params(name)))
    assert pref.clean(checks), checks
    rgba.setflags(write=False)
    return rgba, full


def _check_frame(ctx, p, want_rgba, what):
    """cg_rast_draw_picture against the restatement; the device picture with its depth and shadow
    planes, packed LINEAR at scale 1, against cg_rast_draw."""
    W, H = p.width, p.height
    got, _ = ctx.rast_draw_picture(p)
    _same(got, want_rgba, f"{what}: picture")
    argb, depth, shadow, _ = ctx.rast_draw(p)
    d_rgba, d_depth, d_shadow, d_argb = (_sentinel(4 * W * H), _sentinel(W * H), _sentinel(W * H), _sentinel(W * H))
    ctx.rast_draw_picture_device(p, d_rgba.data_ptr(), d_depth.data_ptr(), d_shadow.data_ptr())
    d_one = _dev(np.array([1.0], np.float32))
    ctx.rast_tonemap_pack_device(d_rgba.data_ptr(), W * H, 1, d_one.data_ptr(), d_argb.data_ptr())
    _same(_host(d_rgba), want_rgba, f"{what}: device picture")
    _same(_host(d_argb), argb, f"{what}: LINEAR at scale 1 against cg_rast_draw")
    _same(_host(d_depth), depth, f"{what}: depth")
    _same(_host(d_shadow), shadow, f"{what}: shadow")
    assert not _host(d_argb).reshape(H, W)[0].any() and not _host(d_argb).reshape(H, W)[:, -1].any()   # border 0


@pytest.fixture(params=["dense", "compact"])
def routed(ctx, request):
    ctx.rast_set_scene()
    ctx.rast_set_route_limit(1 if request.param == "compact" else 0)
    yield ctx, cgamd.RAST_ROUTE_COMPACT if request.param == "compact" else cgamd.RAST_ROUTE_DENSE
    ctx.rast_set_route_limit(0)


@pytest.mark.parametrize("name", list(FRAMES))
def test_picture_matches_the_restatement(routed, name):
    ctx, route = routed
    p = _params(name)
    _check_frame(ctx, p, _expected(name)[0], name)
    assert ctx.rast_scratch_info()["route"] == route


@pytest.fixture(scope="module")
def real_maps():
    import make_golden as mg
    return {k: oracle.jpeg_decode(v) for k, v in mg.texture_jpegs().items()}


@pytest.mark.parametrize("setting,boxes", [(2, 0), (0, 3)])
def test_textured_picture(routed, real_maps, setting, boxes):
    """The grill room (its transparent texels give depth 0 without an owner) and woven-wood boxes."""
    ctx, _ = routed
    p = cgamd.rast_params(96, 64, 48.0)
    oracle.rast_set_textures(real_maps)
    ctx.rast_set_textures(real_maps)
    try:
        want, full, checks = pref.picture(_oracle_params(p, setting, boxes))
        assert pref.clean(checks), checks
        plain = _expected("96x64")[0]
        assert (hdr_ref.bits(want) != hdr_ref.bits(plain)).mean() > 0.05        # the textures matter
        if setting == 2:
            assert (full["depth"] == 0).sum() > (_expected("96x64")[1]["depth"] == 0).sum() + 50
        ctx.rast_set_scene(*cgamd.rast_scene(setting, boxes))
        _check_frame(ctx, p, want, f"textures {setting}/{boxes}")
    finally:
        oracle.rast_set_textures(None)
        ctx.rast_set_textures(None)
        ctx.rast_set_scene()


def test_caller_mesh_picture(ctx):
    """A caller's room and 600 random boxes with their shadow volumes at 96x48: more than 4096
    input triangles, so the frame takes the compact route by itself."""
    W, H, focal = sc.BEYOND["W"], sc.BEYOND["H"], sc.BEYOND["focal"]
    room, nr, _, _ = cgamd.rast_scene()
    nb = 600
    boxes = cgamd.rast_random_scene(nb, 0.1, seed=0xB0C5)
    p = cgamd.rast_params(W, H, focal)
    want, full, checks = pref.picture(sc.oracle_params(p), scene=(room, nr, boxes, nb))
    assert pref.clean(checks) and checks["marked"] > 50, checks
    ctx.rast_set_scene(room, nr, boxes, nb)
    try:
        _check_frame(ctx, p, want, "caller mesh")
        assert ctx.rast_scratch_info()["route"] == cgamd.RAST_ROUTE_COMPACT
    finally:
        ctx.rast_set_scene()


# ---- sequences ----------------------------------------------------------------------------------

SEQ_W, SEQ_H, SEQ_F = 67, 45, 40.0
SEQ_MODES = [0, 1, 2, 0, 1, 1, 2, 0, 2]
SEQ_START = 12_000_000


def _seq_params(start=SEQ_START):
    out = []
    for k, mode in enumerate(SEQ_MODES):
        out.append(cgamd.rast_params(SEQ_W, SEQ_H, SEQ_F, cam=(0.0, 0.0, f32(-3.001 + 0.2 * k), 1.0),
                                     light=(f32(0.1 * (k % 3) - 0.1), -0.5, 0.0, 1.0), colour_mode=mode,
                                     rand_offset=start if k == 0 else 0))
    return out


def _draw_float_sequence(ctx, ps, stride):
    n = len(ps)
    d_rgba, d_info = _sentinel(4 * n * stride), _sentinel(6 * (n + 1))
    ctx.rast_draw_sequence_picture_device(ps, d_rgba.data_ptr(), frame_stride=stride, d_info=d_info.data_ptr())
    return _host(d_rgba).reshape(n, stride, 4), _host(d_info).view(cgamd.RAST_SEQ_DTYPE)


def _draw_argb_sequence(ctx, ps):
    n, px = len(ps), ps[0].width * ps[0].height
    d_argb, d_info = _sentinel(n * px), _sentinel(6 * (n + 1))
    ctx.rast_draw_sequence_device(ps, d_argb.data_ptr(), d_info=d_info.data_ptr())
    return _host(d_argb).reshape(n, px), _host(d_info).view(cgamd.RAST_SEQ_DTYPE)


def test_float_sequence(routed):
    ctx, _ = routed
    ps = _seq_params()
    n, px = len(ps), SEQ_W * SEQ_H
    stride = px + 37
    frames, info = _draw_float_sequence(ctx, ps, stride)
    argb, want_info = _draw_argb_sequence(ctx, ps)
    assert info.tobytes() == want_info.tobytes()                      # the same records
    assert not info["status"].any() and int(info["rand_offset"][n]) > SEQ_START
    assert (frames[:, px:] == SENTINEL).all()                         # the gap of a stride is never written
    for f, p in enumerate(ps):
        q = cgamd.rast_params(SEQ_W, SEQ_H, SEQ_F, cam=(p.camera.x, p.camera.y, p.camera.z, p.camera.w),
                              light=(p.light_scene.x, p.light_scene.y, p.light_scene.z, p.light_scene.w),
                              colour_mode=p.colour_mode, rand_offset=int(info["rand_offset"][f]))
        single, _ = ctx.rast_draw_picture(q)
        _same(frames[f, :px], single, f"frame {f} against its single-frame picture")
        _same(pref.pack(frames[f, :px].view(np.float32), 1.0), argb[f], f"frame {f} packed against the ARGB sequence")
    # and against the restatement at the chained index, one frame of each mode
    for f in (0, 4, 8):
        q = sc.oracle_params(ps[f])
        q.rand_offset = int(info["rand_offset"][f])
        want, full, checks = pref.picture(q)
        assert pref.clean(checks), checks
        _same(frames[f, :px], want, f"frame {f} against the restatement")
        if SEQ_MODES[f]:
            assert int(info["n_shaded"][f]) == full["n_shaded"]


def test_float_sequence_flagged_frame_is_all_uncovered(ctx):
    """A rand() stream of 2000 fragments: the dense route flags the mode 1-2 frames that shade more,
    their float planes are all zeros (defined, not left as they were), the records and every
    other frame are those of the automatic capacity."""
    ctx.rast_set_scene()
    ps = _seq_params()
    px = SEQ_W * SEQ_H
    want_frames, want_info = _draw_float_sequence(ctx, ps, px)
    assert not want_info["status"].any()
    shaded = [int(x) for x in want_info["n_shaded"][:-1]]
    cap = sorted(s for s in shaded if s > 0)[len([s for s in shaded if s > 0]) // 2]   # a middle one: some fit, some do not
    try:
        ctx.rast_set_rand_capacity(cap)
        frames, info = _draw_float_sequence(ctx, ps, px)
    finally:
        ctx.rast_set_rand_capacity(0)
    flagged = [s > cap for s in shaded]
    assert any(flagged) and not all(f or s < 0 for f, s in zip(flagged, shaded))
    assert [int(x) for x in info["status"]] == [cgamd.CG_E_CAPACITY if f else 0 for f in flagged] + [0]
    assert np.array_equal(info["rand_offset"], want_info["rand_offset"])
    assert np.array_equal(info["n_shaded"], want_info["n_shaded"])
    for f in range(len(ps)):
        if flagged[f]:
            assert not frames[f].any(), f"flagged frame {f} is not all zeros"
        else:
            _same(frames[f], want_frames[f], f"frame {f} beside flagged frames")


# ---- the pack -----------------------------------------------------------------------------------

def _synthetic(rng, n):
    px = hdr_ref.random_floats(rng, 4 * n).reshape(n, 4)
    kind = rng.integers(0, 3, n)
    pos = hdr_ref.from_bits(rng.integers(0x33000000, 0x42000000, 3 * n).astype(np.uint32)).reshape(n, 3)
    px[kind == 1, :3] = pos[kind == 1]                                # moderate positive values
    px[kind == 2, :3] = -pos[kind == 2]                               # and negative ones
    px[:, 3] = rng.choice(np.array([0.0, -0.0, 1.0, 1.0, 1.0, np.nan, -1.0, np.inf, 9.0], np.float32), n)
    return px


@pytest.mark.parametrize("op,white2", [(hdr_ref.TONE_LINEAR, 1.0), (hdr_ref.TONE_REINHARD, 1.0),
                                       (hdr_ref.TONE_REINHARD_WHITE, 7.5)])
def test_pack_matches_pack_pixel(ctx, op, white2):
    """Three frames -- a rendered picture, synthetic pixels, the picture again -- with source and
    destination strides of their own and a scale per frame; the gaps stay untouched."""
    rng = np.random.default_rng(0x9AC + op)
    pic = np.asarray(_expected("67x45")[0]).reshape(-1, 4)
    n = len(pic)
    planes = np.stack([pic, _synthetic(rng, n), pic])
    scales = np.array([1.0, 0.37, 250.0], np.float32)
    for ss, ds in ((n, n), (n + 5, n + 11)):
        src = np.full((3, ss, 4), 3.0e38, np.float32)
        src[:, :n] = planes
        d_src, d_dst, d_scales = _dev(src), _sentinel(3 * ds), _dev(scales)
        ctx.rast_tonemap_pack_device(d_src.data_ptr(), n, 3, d_scales.data_ptr(), d_dst.data_ptr(), op, white2,
                                     src_stride=ss if ss != n else 0, dst_stride=ds if ds != n else 0)
        got = _host(d_dst).reshape(3, ds)
        assert (got[:, n:] == SENTINEL).all()
        for f in range(3):
            _same(got[f, :n], cgamd.rast_pack_pixel(planes[f], scales[f], op, white2), f"op {op} frame {f} stride {ss}/{ds}")
    # the border rule against the raytracer's pack on the same plane
    d_src, d_dst, d_scales = _dev(planes[0]), _sentinel(n), _dev(scales)
    ctx.rt_tonemap_pack_device(d_src.data_ptr(), n, 1, d_scales.data_ptr(), d_dst.data_ptr(), op, white2)
    rt = _host(d_dst).reshape(45, 67)
    assert (rt[0] == 0x80000000).all() and cgamd.rast_pack_pixel(planes[0], 1.0, op, white2).reshape(45, 67)[0].max() == 0


def test_picture_argument_errors(ctx):
    inv, nos = f"({cgamd.CG_E_INVALID})", f"({cgamd.CG_E_NOSCENE})"
    buf = _sentinel(4 * 64 * 48 + 8)
    p = cgamd.rast_params(64, 48, 32.0)

    def rc(fn):
        with pytest.raises(RuntimeError) as e:
            fn()
        return str(e.value)
    with cgamd.Context(0) as fresh:
        assert nos in rc(lambda: fresh.rast_draw_picture(p))
        assert nos in rc(lambda: fresh.rast_draw_picture_device(p, buf.data_ptr()))
    ctx.rast_set_scene()
    assert inv in rc(lambda: ctx.rast_draw_picture_device(p, buf.data_ptr() + 4))          # 16-byte alignment
    assert inv in rc(lambda: ctx.rast_draw_picture_device(p, None))
    assert inv in rc(lambda: ctx.rast_draw_picture(cgamd.rast_params(2, 48, 32.0)))
    assert inv in rc(lambda: ctx.rast_draw_sequence_picture_device([p, p], buf.data_ptr(), frame_stride=64 * 48 - 1,
                                                                   d_info=buf.data_ptr()))
    assert inv in rc(lambda: ctx.rast_draw_sequence_picture_device([p], buf.data_ptr(), d_info=None))
    assert inv in rc(lambda: ctx.rast_tonemap_pack_device(buf.data_ptr(), 16, 1, buf.data_ptr(), buf.data_ptr(), op=7))
    assert inv in rc(lambda: ctx.rast_tonemap_pack_device(buf.data_ptr(), 16, 1, buf.data_ptr(), buf.data_ptr(),
                                                          op=hdr_ref.TONE_REINHARD_WHITE, white2=0.0))
    ctx.rast_draw_sequence_picture_device([], buf.data_ptr(), d_info=buf.data_ptr())        # no frames: nothing written
    ctx.rast_tonemap_pack_device(buf.data_ptr(), 16, 0, buf.data_ptr(), buf.data_ptr())
    assert (_host(buf) == SENTINEL).all()
