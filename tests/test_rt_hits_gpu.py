"""GPU: per-pixel hit records and picking (cg_rt_hits, cg_rt_hits_device, cg_rt_pick), tolerance 0.

Every record plane is compared byte for byte with two references:
* cg_rt_probe_closest (the GPU's brute-force ClosestIntersection) on cg_rt_pixel_ray's rays, every
  pixel;
* the oracle's cgo_rt_closest on the same rays: every pixel of frames up to 64 x 48, a fixed sample
  of 2,048 pixels beyond.
The index and distance planes must agree with the record plane.  The ray geometry is also pinned
without the helper: a rendered pixel is black exactly when all nine sub-ray planes miss it.

Small route (n_tris <= 64: rt_hits_small_kernel), the boundary at 64 / 65 triangles, the large
route (a hits-only pass of the binned path) over the cameras of test_rt_big_gpu.py with the pools
sized and forced to overflow, ties and degenerate triangles, stripe shards with padding rows,
cg_rt_pick, and the absence of side effects on later frames.  Sub-rays: all nine, except the
640 x 160 camera (corner, centre, corner: 0, 4, 8)."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import oracle
from test_rt_big_gpu import CASES, PITCH, YAW

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
BLACK = 0x80000000
CG_E_INVALID, CG_E_NOSCENE = -1, -4
ALL9 = tuple(range(9))


class Scene:
    """A scene for the library (cgamd.Tri, cgamd.Sphere) and the same bytes for the oracle."""

    def __init__(self, tris, n, sph=None):
        self.tris, self.n, self.sph = tris, n, sph
        self.otris = (oracle.RtTri * max(n, 1)).from_buffer_copy(bytes(tris)[:max(n, 1) * 76])
        self.osph = oracle.Sphere.from_buffer_copy(bytes(sph)) if sph is not None else None

    def set(self, ctx):
        ctx.rt_set_scene(self.tris, self.n, self.sph, 1 if self.sph is not None else 0)

    def oracle_record(self, lib, start, d):
        ci = oracle.Isect()                     # zeros: the fields a miss leaves alone
        lib.cgo_rt_closest(oracle.V4(*start), oracle.V4(*d), self.otris, self.n,
                           C.byref(self.osph) if self.osph is not None else None,
                           1 if self.osph is not None else 0, C.byref(ci), None)
        return bytes(ci)


def _reference_scene():
    tris, n, sph = cgamd.rt_scene()
    return Scene(tris, n, sph)


def _random(n, sph=None, total=None):
    """The first n triangles of random_scene(total or n, 0x5EED)."""
    return Scene(cgamd.random_scene(total or n, 0x5EED), n, sph)


def _array_scene(a, sph=None):
    n = len(a)
    return Scene((cgamd.Tri * n).from_buffer_copy(np.ascontiguousarray(a, np.float32).tobytes()), n, sph)


@pytest.fixture(scope="module")
def restore(ctx):
    yield ctx
    _reference_scene().set(ctx)


def _cam(W, H, focal, cam=(0.0, 0.0, -3.0, 1.0), R=None):
    return cgamd.rt_camera(W, H, focal, tuple(cam), (C.c_float * 16)(*R) if R is not None else None)


def _case_cam(case):
    cfg = dict(dict(width=64, height=48, focal=48.0, cam=[0, 0, -3.0, 1]), **CASES[case])
    return _cam(cfg["width"], cfg["height"], cfg["focal"], cfg["cam"], cfg["R"])


def _sample(npix):
    if npix <= 64 * 48:
        return np.arange(npix)
    return np.sort(np.random.default_rng(0x5EED).choice(npix, 2048, replace=False))


def _index_of(rec):
    miss = ~(rec["distance"] < FLT_MAX)
    idx = np.where(rec["sphereIndex"] >= 0, -1 - rec["sphereIndex"], rec["triangleIndex"]).astype(np.int32)
    # a triangle hit has sphereIndex -1 and a sphere hit triangleIndex -1
    return np.where(miss, np.int32(cgamd.HIT_NONE), idx)


def _check_planes(ctx, scene, cam, sub, planes=None):
    """The three planes of (cam, sub) against both references; returns (isect, index, distance)."""
    isect, index, dist = planes if planes is not None else ctx.rt_hits(cam, sub)
    npix = cam.width * cam.height
    starts, dirs = cgamd.rt_pixel_rays(cam, sub)
    ref, hit = ctx.rt_probe_closest_np(starts, dirs)
    a, b = isect.view(np.uint8).reshape(npix, 28), ref.view(np.uint8).reshape(npix, 28)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"sub-ray {sub}: {bad.size} records differ from the probe, first {bad[:4]}: " \
                          f"{isect[bad[:2]]} vs {ref[bad[:2]]}"
    assert np.array_equal(index, _index_of(isect)), f"sub-ray {sub}: index plane"
    assert np.array_equal(dist.view(np.uint32), isect["distance"].view(np.uint32)), f"sub-ray {sub}: distance plane"
    assert np.array_equal(hit != 0, index != cgamd.HIT_NONE)
    miss = isect[index == cgamd.HIT_NONE]
    assert all(m.tobytes() == np.array([((0, 0, 0, 0), FLT_MAX, 0, 0)], cgamd.ISECT_DTYPE).tobytes() for m in miss[:8])
    olib = oracle.load()
    for p in _sample(npix):
        want = scene.oracle_record(olib, starts[p].tolist(), dirs[p].tolist())
        assert isect[p].tobytes() == want, f"sub-ray {sub} pixel {p}: {isect[p]} vs the oracle's " \
                                           f"{np.frombuffer(want, cgamd.ISECT_DTYPE)}"
    return isect, index, dist


# ---- errors ----------------------------------------------------------------
def test_argument_errors(restore):
    ctx, lib = restore, cgamd.load()
    cam = _cam(64, 48, 48.0)
    n = 64 * 48
    rec, idx = np.zeros(n, cgamd.ISECT_DTYPE), np.zeros(n, np.int32)
    one, hit = np.zeros(1, cgamd.ISECT_DTYPE), C.c_int()
    P = C.c_void_p
    pone = C.cast(one.ctypes.data, C.POINTER(cgamd.Isect))
    with cgamd.Context(0) as fresh:             # no scene yet
        assert lib.cg_rt_hits(fresh.h, C.byref(cam), 4, rec.ctypes.data_as(P), None, None) == CG_E_NOSCENE
        assert lib.cg_rt_hits_device(fresh.h, C.byref(cam), 4, None, None, P(16), None, None) == CG_E_NOSCENE
        assert lib.cg_rt_pick(fresh.h, C.byref(cam), 1, 1, 4, pone, C.byref(hit)) == CG_E_NOSCENE
    _reference_scene().set(ctx)
    for sub in (-1, 9):
        assert lib.cg_rt_hits(ctx.h, C.byref(cam), sub, rec.ctypes.data_as(P), None, None) == CG_E_INVALID
        assert lib.cg_rt_hits_device(ctx.h, C.byref(cam), sub, None, None, P(16), None, None) == CG_E_INVALID
        assert lib.cg_rt_pick(ctx.h, C.byref(cam), 1, 1, sub, pone, C.byref(hit)) == CG_E_INVALID
    assert lib.cg_rt_hits(ctx.h, C.byref(cam), 4, None, None, None) == CG_E_INVALID
    assert lib.cg_rt_hits_device(ctx.h, C.byref(cam), 4, None, None, None, None, None) == CG_E_INVALID
    for x, y in [(-1, 0), (64, 0), (0, -1), (0, 48)]:
        assert lib.cg_rt_pick(ctx.h, C.byref(cam), x, y, 4, pone, C.byref(hit)) == CG_E_INVALID
    # any one plane alone is a valid call
    assert lib.cg_rt_hits(ctx.h, C.byref(cam), 4, None, idx.ctypes.data_as(P), None) == 0
    assert (idx != cgamd.HIT_NONE).any()


# ---- small route -----------------------------------------------------------
@pytest.mark.parametrize("rot", ["identity", "yaw", "pitch"])
@pytest.mark.parametrize("W,H,focal", [(64, 48, 48.0), (320, 256, 256.0)])
def test_small_route_reference_scene(restore, W, H, focal, rot):
    scene = _reference_scene()
    scene.set(restore)
    cam = _cam(W, H, focal, R={"identity": None, "yaw": YAW, "pitch": PITCH}[rot])
    kinds = set()
    for sub in ALL9:
        _, index, _ = _check_planes(restore, scene, cam, sub)
        kinds |= set(np.unique(index).tolist())
    assert -1 in kinds and len([k for k in kinds if k >= 0]) >= 10        # the sphere and many triangles
    if W == 64:
        assert cgamd.HIT_NONE in kinds                                     # and rays past the open front


@pytest.mark.parametrize("which", ["reference", "random500"])
def test_black_pixels_are_the_pixels_all_nine_sub_rays_miss(restore, which):
    """The ray geometry without cg_rt_pixel_ray: every colour is >= 0.15 and the indirect light 0.5,
    so one hit among a pixel's nine sub-rays already gives a channel >= 255 * 0.15 * 0.5 / 9 > 2."""
    scene = _reference_scene() if which == "reference" else _random(500)
    scene.set(restore)
    cam = _cam(64, 48, 48.0)
    argb, _ = restore.rt_render(cam)
    any_hit = np.zeros(64 * 48, bool)
    for sub in ALL9:
        any_hit |= restore.rt_hits(cam, sub, isect=False, distance=False)[1] != cgamd.HIT_NONE
    assert np.array_equal(argb == BLACK, ~any_hit)
    assert any_hit.any() and not any_hit.all()


@pytest.mark.parametrize("n", [64, 65])
def test_route_boundary(restore, n):
    """The first 64 / 65 triangles of one random scene: the last scene of the per-pixel kernel and
    the first of the binned path."""
    scene = _random(n, total=500)
    scene.set(restore)
    cam = _cam(64, 48, 48.0)
    seen = set()
    for sub in ALL9:
        seen |= set(np.unique(_check_planes(restore, scene, cam, sub)[1]).tolist())
    assert len([k for k in seen if k >= 0]) >= 5
    info = restore.rt_scratch_info()
    if n == 65:
        assert info["listed"] > 0 and info["overflows"] == 0, info


# ---- large route -----------------------------------------------------------
BIG_CAMS = ["lat_1", "yawlat_1", "pix_pitch_1", "inside_lat_1", "vertex_plane_lat_1", "inside_lat_wide"]


@pytest.fixture(scope="module")
def big(restore):
    scene = _random(500)
    scene.set(restore)
    return restore, scene


@pytest.mark.parametrize("case", BIG_CAMS)
@pytest.mark.parametrize("stress", ["sized", "pools_overflow", "sorted_overflow"])
def test_large_route_matches_both_references(big, case, stress):
    ctx, scene = big
    scene.set(ctx)                      # other tests of the module change the scene
    cam = _case_cam(case)
    hits = 0
    try:
        if stress == "pools_overflow":
            ctx.rt_set_pool_caps(1, 1, 1, 1)
        elif stress == "sorted_overflow":
            ctx.rt_set_pool_caps(1 << 20, 1 << 20, 1 << 20, 64)
        for sub in (ALL9 if cam.width == 64 else (0, 4, 8)):
            hits += int((_check_planes(ctx, scene, cam, sub)[1] >= 0).sum())
        info = ctx.rt_scratch_info()
    finally:
        ctx.rt_set_pool_caps(0, 0, 0)
    assert hits > 100                                                     # the frame does see the cloud
    if stress == "sized":
        assert info["overflows"] == 0 and info["listed"] > 0, info
    else:
        assert info["overflows"] >= 1, info


@pytest.mark.parametrize("case", ["lat_1", "pix_pitch_1"])
def test_large_route_with_the_sphere(restore, case):
    scene = _random(500, sph=cgamd.rt_scene()[2])
    scene.set(restore)
    cam = _case_cam(case)
    kinds = set()
    for sub in ALL9:
        kinds |= set(np.unique(_check_planes(restore, scene, cam, sub)[1]).tolist())
    assert -1 in kinds and any(k >= 0 for k in kinds)


def test_large_route_lists_span_several_chunks(restore):
    """5,000 triangles at 136 x 40: a bin's list is built from five 1,024-triangle chunks."""
    scene = _random(5000)
    scene.set(restore)
    cam = _cam(136, 40, 40.0)
    for sub in ALL9:
        _, index, _ = _check_planes(restore, scene, cam, sub)
    assert (index >= 1024).any() and (index >= 4096).any()
    assert restore.rt_scratch_info()["overflows"] == 0


# ---- ties and degenerate input --------------------------------------------
def _edge_scene(n):
    """random_scene(n) with, written over its first triangles: a backdrop held twice (indices 3 and
    7: every ray that reaches it ties), a triangle of zero area, one with a NaN vertex, and one in
    the plane z = cam.z = -3 beside the eye."""
    a = np.frombuffer(bytes(cgamd.random_scene(n, 0x5EED)), np.float32).reshape(n, 19).copy()
    v = lambda k: a[k, 0:12].reshape(3, 4)                               # noqa: E731
    v(3)[:, :3] = [[-5, -5, 1.5], [5, -5, 1.5], [0, 5, 1.5]]
    a[7] = a[3]
    v(4)[1], v(4)[2] = v(4)[0].copy(), v(4)[0].copy()                    # a point
    v(5)[1, 0] = np.nan
    v(6)[:, :3] = [[0.5, -1, -3], [2, -1, -3], [1, 1, -3]]
    return _array_scene(a)


@pytest.mark.parametrize("n", [40, 500])         # the per-pixel kernel and the binned path
def test_ties_and_degenerate_triangles(restore, n):
    scene = _edge_scene(n)
    scene.set(restore)
    cam = _cam(64, 48, 48.0)
    for sub in ALL9:
        isect, index, _ = _check_planes(restore, scene, cam, sub)
        assert (index == 3).sum() > 64 * 48 // 2 and not (index == 7).any()      # the lower index keeps the tie
        assert not np.isin(index, [4, 5, 6]).any()
    for p in (0, 64 * 24 + 32, 64 * 48 - 1, 64 * 10 + 50):                       # the pick's tie rule
        rec, hit = restore.rt_pick(cam, p % 64, p // 64, 8)
        assert rec[0].tobytes() == isect[p].tobytes() and hit == (index[p] != cgamd.HIT_NONE)
    assert int(isect[0]["triangleIndex"]) == 3


# ---- shards ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["reference", "random500"])
def test_two_stripe_shards_give_the_frame(restore, which):
    import torch
    scene = _reference_scene() if which == "reference" else _random(500)
    scene.set(restore)
    W, H, sh = 64, 44, 8                                  # 6 stripes (the last of 4 rows), 3 per rank
    cam = _cam(W, H, 48.0)
    whole = restore.rt_hits(cam, 4)
    dev = torch.device("cuda", 0)
    rows = 24
    got = np.zeros(H * W, cgamd.ISECT_DTYPE), np.zeros(H * W, np.int32), np.zeros(H * W, np.float32)
    for rank in range(2):
        d_rec = torch.full((rows * W * 28,), 0x55, dtype=torch.uint8, device=dev)
        d_idx = torch.full((rows * W,), 7, dtype=torch.int32, device=dev)
        d_dst = torch.full((rows * W,), -1.0, dtype=torch.float32, device=dev)
        restore.rt_hits_device(cam, 4, cgamd.RtShard(rank, 2, sh, 0, 0, 0, 0), d_rec.data_ptr(), d_idx.data_ptr(),
                               d_dst.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        rec = d_rec.cpu().numpy().view(cgamd.ISECT_DTYPE).reshape(rows, W)
        idx, dst = d_idx.cpu().numpy().reshape(rows, W), d_dst.cpu().numpy().reshape(rows, W)
        for L in range(rows):
            k = L // sh
            y = (k * 2 + rank) * sh + L % sh
            if y < H:
                got[0][y * W:(y + 1) * W], got[1][y * W:(y + 1) * W], got[2][y * W:(y + 1) * W] = rec[L], idx[L], dst[L]
            else:                                          # padding rows of the last stripe: misses
                assert (idx[L] == cgamd.HIT_NONE).all() and (dst[L] == FLT_MAX).all()
                assert rec[L].tobytes() == np.array([((0, 0, 0, 0), FLT_MAX, 0, 0)] * W, cgamd.ISECT_DTYPE).tobytes()
    for a, b in zip(got, whole):
        assert a.tobytes() == b.tobytes()
    # the frame is not empty (the cloud's triangles are ~0.02 wide: only some centre rays meet one)
    assert (whole[1] != cgamd.HIT_NONE).sum() >= 10


# ---- pick ------------------------------------------------------------------
def test_pick_equals_the_plane(big):
    ctx, scene = big
    scene.set(ctx)
    cam = _case_cam("lat_1")
    isect, index, _ = ctx.rt_hits(cam, 4)
    px = np.random.default_rng(7).choice(64 * 48, 256, replace=False)
    for p in px:
        rec, hit = ctx.rt_pick(cam, int(p) % 64, int(p) // 64, 4)
        assert rec[0].tobytes() == isect[p].tobytes(), (p, rec, isect[p])
        assert hit == (index[p] != cgamd.HIT_NONE)
    assert (index[px] == cgamd.HIT_NONE).any() and (index[px] >= 0).any()


def test_pick_on_a_scene_its_grid_strides_over(restore):
    """40,000 triangles: more than the 32,768 one pass of the pick kernel's workgroups covers."""
    scene = _random(40000)
    scene.set(restore)
    cam = _cam(64, 48, 48.0)
    isect, index, _ = restore.rt_hits(cam, 4)
    starts, dirs = cgamd.rt_pixel_rays(cam, 4)
    ref, _ = restore.rt_probe_closest_np(starts, dirs)
    assert isect.tobytes() == ref.tobytes()
    assert (index >= 32768).any()                          # winners beyond the first stride
    late = np.flatnonzero(index >= 32768)[:16]
    for p in list(late) + list(np.random.default_rng(11).choice(64 * 48, 48, replace=False)):
        rec, hit = restore.rt_pick(cam, int(p) % 64, int(p) // 64, 4)
        assert rec[0].tobytes() == isect[p].tobytes(), (p, rec, isect[p])


# ---- no side effects -------------------------------------------------------
@pytest.mark.parametrize("which", ["reference", "random500"])
def test_render_hits_render(restore, which):
    scene = _reference_scene() if which == "reference" else _random(500)
    scene.set(restore)
    cam, yawed = _cam(64, 48, 48.0), _cam(64, 48, 48.0, R=YAW)
    before = restore.rt_render(cam)[0]
    restore.rt_hits(yawed, 2)
    restore.rt_hits(cam, 4)
    restore.rt_pick(cam, 10, 10, 4)
    after = restore.rt_render(cam)[0]
    assert np.array_equal(before, after) and (before != BLACK).any()


def test_hits_is_the_first_call_on_a_fresh_scene(restore):
    """Nothing has rendered this scene: the hits call itself sizes the pools."""
    scene = _random(700)
    scene.set(restore)
    cam = _cam(64, 48, 48.0)
    planes = restore.rt_hits(cam, 4)
    info, demand = restore.rt_scratch_info(), restore.rt_pool_demand()
    assert info["overflows"] == 0 and info["listed"] > 0 and info["capacity"] >= info["listed"], info
    assert demand["sup"] > 0 and demand["bin"] > 0 and demand["sorted"] > 0 and demand["sbin"] == 0, demand
    _check_planes(restore, scene, cam, 4, planes)
    ref = oracle.rt_draw(oracle.rt_params(64, 48, 48.0), scene=(scene.otris, scene.n, None, 0))
    assert np.array_equal(restore.rt_render(cam)[0], ref)                 # and a frame after it is right
