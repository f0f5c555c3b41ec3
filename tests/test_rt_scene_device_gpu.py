"""GPU: cg_rt_set_scene_device -- a scene installed from device memory, its bounds and grid built by
cg_rt_grid.hip -- against cg_rt_set_scene of the same bytes (the host builder is the checker).
Everything compares at tolerance 0: grids as bytes, frames as uint32 on every pixel."""
import ctypes as C
import os

import numpy as np
import pytest

import cgamd
import make_golden as mg
import oracle

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024          # elements per workgroup of the builder's scans (cg_rt_grid.hip kScanTile)
L0 = [[0.0, -0.5, -0.7, 1.0], [14.0, 14.0, 14.0]]
YAW = mg.yaw_R(np.float32(0.0) - np.float32(0.174533))


def _pitch(a):
    """Rotation about x (column-major m[4 c + r]), float32 cos/sin."""
    c, sn = float(np.cos(np.float32(a), dtype=np.float32)), float(np.sin(np.float32(a), dtype=np.float32))
    m = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    m[1 * 4 + 1], m[1 * 4 + 2], m[2 * 4 + 1], m[2 * 4 + 2] = c, sn, -sn, c
    return m


PITCH = _pitch(0.15)


@pytest.fixture(scope="module")
def gctx():
    """A context of this module's own: its scenes and caps never reach the session's shared one."""
    c = cgamd.Context(0)
    yield c
    c.close()


def _dev(tris):
    """The ctypes triangle array's bytes as a device tensor (float32 [n, 19])."""
    import torch
    n = len(tris)
    return torch.frombuffer(bytearray(bytes(tris)), dtype=torch.float32).reshape(n, 19).cuda()


def _tris_of(a):
    """float32 [n, 19] -> (cgamd.Tri array, n)."""
    a = np.ascontiguousarray(a, np.float32)
    return (cgamd.Tri * a.shape[0]).from_buffer_copy(a.tobytes()), a.shape[0]


def _rows(n, seed=0x5EED):
    return np.frombuffer(bytes(cgamd.random_scene(n, seed)), np.float32).reshape(n, 19).copy()


def _set_normals(a, ks):
    """ComputeNormal (TestModelH.h:96-105) in float32 for rows ks (NaN for zero area)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in ks:
            t = a[k, 0:12].reshape(3, 4)
            e1, e2 = t[1, :3] - t[0, :3], t[2, :3] - t[0, :3]
            c = np.cross(e2, e1).astype(np.float32)
            a[k, 12:15] = c / np.float32(np.sqrt(np.float32((c * c).sum())))
            a[k, 15] = 1.0


def _install(ctx, form, tris, n, sph=None, n_sph=0):
    if form == "host":
        ctx.rt_set_scene(tris, n, sph, n_sph)
        return None
    d = _dev(tris) if n else None
    ctx.rt_set_scene_device(d.data_ptr() if n else 0, n, sph, n_sph)
    if d is not None:
        d.zero_()          # on return the caller's buffer is no longer read
    return d


def _lights(area=False):
    lights = (cgamd.Light * 1)()
    lights[0].position = cgamd.Vec4(*L0[0])
    lights[0].colour = cgamd.Vec3(*L0[1])
    return cgamd.area_lights(lights[0], 0.1, 4) if area else lights


def _frame(ctx, W=96, H=54, focal=54.0, R=None, area=False, cam=(0.0, 0.0, -3.0, 1.0)):
    Rm = (C.c_float * 16)(*R) if R is not None else None
    return ctx.rt_render(cgamd.rt_camera(W, H, focal, cam, Rm), _lights(area))[0]


def _grids_equal(a, b, what):
    assert (a is None) == (b is None), f"{what}: one form has a grid, the other none"
    if a is None:
        return
    for k in ("res", "lo", "start", "tris"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what}: {k} {a[k].shape} {b[k].shape}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs at {np.flatnonzero(a[k] != b[k])[:5]}"
    assert np.float32(a["h"]).tobytes() == np.float32(b["h"]).tobytes(), what


def _both_grids(ctx, tris, n, what):
    _install(ctx, "host", tris, n)
    gh = ctx.rt_grid()
    hinfo = ctx.rt_grid_info()
    _install(ctx, "device", tris, n)
    gd = ctx.rt_grid()
    dinfo = ctx.rt_grid_info()
    _grids_equal(gd, gh, what)
    assert gh is not None and gh["tris"].size > 0, what
    assert hinfo["candidates"] == 0 and dinfo["candidates"] >= dinfo["entries"] == gh["tris"].size
    assert dinfo["cells"] == gh["start"].size - 1 == hinfo["cells"] and dinfo["bytes"] > 0
    return gh


# ---- 1. grid equality on random scenes ----------------------------------------------------------
@pytest.mark.parametrize("n", [65, 500, 20000, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_grid_equals_host_grid_random_scene(gctx, n):
    g = _both_grids(gctx, cgamd.random_scene(n), n, f"random {n}")
    seg = np.diff(g["start"])
    assert seg.min() >= 0 and g["start"][-1] == g["tris"].size
    # every cell lists its triangles in ascending order
    asc = np.diff(g["tris"]) > 0
    inner = g["start"][1:-1]
    asc[inner[(inner > 0) & (inner < g["tris"].size)] - 1] = True        # steps from one cell to the next
    assert asc.all()


# ---- 2. long and awkward cells ---------------------------------------------------------------
def _copies_scene(m=3000):
    """m byte-identical copies of one small triangle and one far triangle that stretches the
    box: a few cells hold thousands of entries."""
    a = np.repeat(_rows(1), m + 1, axis=0)
    a[m, 0:12] = np.array([[30, 30, 30, 1], [31, 30, 30, 1], [30, 31, 30.5, 1]], np.float32).reshape(-1)
    _set_normals(a, [m])
    return a


def _degenerate_scene(n=500):
    """random_scene(n) with edge-case triangles over its first ones, as
    tests/test_rt_big_gpu.py::_degenerate_scene builds them (the eye-plane triangle beside the eye)."""
    a = _rows(n)
    v = lambda k: a[k, 0:12].reshape(3, 4)                               # noqa: E731
    p = v(1)[0].copy()
    v(1)[1], v(1)[2] = p, p                                              # a point
    v(2)[2, :3] = v(2)[0, :3] + np.float32(2) * (v(2)[1, :3] - v(2)[0, :3])   # collinear (float)
    v(3)[2, :3] = v(3)[0, :3] + np.float32(0.5) * (v(3)[1, :3] - v(3)[0, :3])
    v(4)[1] = v(4)[0]                                                    # repeated vertex
    v(5)[2, :3] = v(5)[1, :3] + np.float32(1e-6)                         # sliver
    v(6)[:, :3] = [[-5, -5, 1.5], [5, -5, 1.5], [0, 5, 1.5]]             # backdrop
    v(7)[:, :3] = [[0.5, -1, -3], [2, -1, -3], [1, 1, -3]]               # in the eye plane
    v(8)[:, :3] = [[-1, -1, -4], [1, -1, -4], [0, 1, -4]]                # behind the eye
    _set_normals(a, range(1, 9))
    return a


def _spanning_scene(n=200):
    """n triangles that each span the whole box: few cells, every triangle a candidate in all."""
    rng = np.random.default_rng(5)
    a = _rows(n)
    z = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    for k in range(n):
        a[k, 0:12] = np.array([[-1, -1, z[k, 0], 1], [1, -1, z[k, 1], 1], [0, 1, z[k, 2], 1]], np.float32).reshape(-1)
    a[0, 2], a[1, 2] = -1.0, 1.0                                          # the box is [-1, 1] in z too
    _set_normals(a, range(n))
    return a


def _flat_scene(n=300):
    a = _rows(n)
    a[:, [2, 6, 10]] = np.float32(0.5)                                    # all z equal
    _set_normals(a, range(n))
    return a


# copies_5000: a segment longer than the long sort's LDS tile (kSortLds = 4096): its global-memory path
AWKWARD = {"copies": _copies_scene, "copies_5000": lambda: _copies_scene(5000), "degenerate": _degenerate_scene, "spanning": _spanning_scene, "flat_z": _flat_scene}


@pytest.mark.parametrize("name", list(AWKWARD))
def test_grid_and_frame_equal_awkward_scene(gctx, name):
    tris, n = _tris_of(AWKWARD[name]())
    _install(gctx, "host", tris, n)
    gh, fh = gctx.rt_grid(), _frame(gctx)
    _install(gctx, "device", tris, n)
    gd, fd, info = gctx.rt_grid(), _frame(gctx), gctx.rt_grid_info()
    _grids_equal(gd, gh, name)
    assert gh is not None
    assert np.array_equal(fd, fh), f"{name}: {(fd != fh).sum()} pixels differ"
    seg = np.diff(gh["start"])
    if name == "copies_5000":
        assert seg.max() >= 5000
    if name == "copies":
        assert seg.max() >= 3000                       # beyond a wave, and sorted by the long path
    if name == "spanning":
        assert info["candidates"] >= 64 * n and seg.size < 4096
    if name == "flat_z":
        assert gh["res"][2] == 1
    if "copies" not in name:                             # (one small triangle: a handful of pixels)
        assert (fh != 0x80000000).sum() > 50


# ---- 3. caps ----------------------------------------------------------------------------------
def test_caps_decline_the_grid(gctx):
    n = 500
    tris = cgamd.random_scene(n)
    frames = {}
    try:
        _install(gctx, "device", tris, n)
        info = gctx.rt_grid_info()
        E, B = info["entries"], info["candidates"]
        assert gctx.rt_grid() is not None and 0 < E <= B
        plain = _frame(gctx)
        for caps, host_has, dev_has in (((E, 0), True, True), ((E - 1, 0), False, False), ((0, B - 1), True, False)):
            gctx.rt_set_grid_caps(*caps)
            _install(gctx, "host", tris, n)
            assert (gctx.rt_grid() is not None) == host_has, caps
            frames[caps, "host"] = _frame(gctx)
            _install(gctx, "device", tris, n)
            assert (gctx.rt_grid() is not None) == dev_has, caps
            frames[caps, "device"] = _frame(gctx)
    finally:
        gctx.rt_set_grid_caps(0, 0)
    for key, f in frames.items():
        assert np.array_equal(f, plain), key
    assert (plain != 0x80000000).sum() > 50


# ---- 4. images -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair500(gctx):
    """The 500-triangle scene's frames under every camera, installed by each form (rendered once)."""
    n = 500
    tris = cgamd.random_scene(n)
    out = {}
    for form in ("host", "device"):
        _install(gctx, form, tris, n)
        for cam, R in (("unrotated", None), ("yawed", YAW), ("pitched", PITCH)):
            for area in (False, True):
                out[form, cam, area] = _frame(gctx, 157, 93, 93.0, R, area)
    return out


@pytest.mark.parametrize("area", [False, True])
@pytest.mark.parametrize("cam", ["unrotated", "yawed", "pitched"])
def test_frames_equal_host_installed(pair500, cam, area):
    a, b = pair500["device", cam, area], pair500["host", cam, area]
    assert np.array_equal(a, b), f"{(a != b).sum()} pixels differ"
    assert (a != 0x80000000).sum() > 100


def test_unrotated_frame_equals_oracle(pair500):
    cfg = dict(width=157, height=93, focal=93.0, cam=[0, 0, -3.0, 1], scene=dict(random=500, seed=0x5EED), R=None,
               lights=[L0])
    ref = oracle.rt_draw(mg.rt_params_of(cfg), scene=mg.rt_oracle_scene(cfg), threads=min(16, os.cpu_count() or 8))
    got = pair500["device", "unrotated", False]
    assert np.array_equal(got, ref), f"{(got != ref).sum()} pixels differ"


# ---- 5. the small scene (n <= 64: bounds only) ------------------------------------------------
def test_cornell_box_from_device_equals_reference_screenshot(gctx):
    tris, n, sph = cgamd.rt_scene()
    assert n == 28
    _install(gctx, "device", tris, n, sph, 1)
    assert gctx.rt_grid() is None
    cam = cgamd.rt_camera(320, 256, 256.0, (0.0, 0.0, mg.CAM_UP, 1.0))
    got = gctx.rt_render(cam, cgamd.default_lights())[0]
    ref = mg.screenshot_argb()
    assert ref.size == 81920 and abs(mg.CAM_UP + 2.9) < 1e-6
    assert np.array_equal(got, ref), f"{(got != ref).sum()} pixels differ"


# ---- 6. a moving scene without host copies ----------------------------------------------------
def test_moving_scene_on_one_stream(gctx):
    import torch
    n, W, H, steps = 500, 96, 54, 4
    dev = torch.device("cuda", 0)
    cam = cgamd.rt_camera(W, H, 54.0)
    lights = _lights()
    t = _dev(cgamd.random_scene(n))
    rng = np.random.default_rng(11)
    moves = torch.from_numpy(rng.uniform(-0.05, 0.05, (steps, n // 10, 1, 3)).astype(np.float32)).to(dev)
    out = torch.zeros(steps, W * H, dtype=torch.int32, device=dev)
    snaps = []
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for k in range(steps):
            sel = slice(k * (n // 10), (k + 1) * (n // 10))
            v = t[sel, 0:12].reshape(n // 10, 3, 4)
            v[:, :, :3] += moves[k]                       # a rigid translation per triangle; normals stay
            snaps.append(t.clone())
            arg = t.clone()
            gctx.rt_set_scene_device(arg.data_ptr(), n, None, 0, stream=s.cuda_stream)
            arg.zero_()                                   # the caller's buffer is no longer read
            gctx.rt_render_device(cam, out[k].data_ptr(), stream=s.cuda_stream, lights=lights)
    s.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    seen = set()
    for k in range(steps):
        tris, _ = _tris_of(snaps[k].cpu().numpy())
        gctx.rt_set_scene(tris, n, None, 0)
        want = gctx.rt_render(cam, lights)[0]
        assert np.array_equal(got[k], want), f"step {k}: {(got[k] != want).sum()} pixels differ"
        seen.add(want.tobytes())
    assert len(seen) == steps                             # the scene did move


# ---- 7. arguments -----------------------------------------------------------------------------
def test_arguments(gctx):
    lib, h = gctx.lib, gctx.h
    d = _dev(cgamd.random_scene(8))
    assert lib.cg_rt_set_scene_device(h, C.c_void_p(d.data_ptr()), -1, None, 0, None) == cgamd.CG_E_INVALID
    assert lib.cg_rt_set_scene_device(h, None, 5, None, 0, None) == cgamd.CG_E_INVALID
    assert lib.cg_rt_set_scene_device(h, C.c_void_p(d.data_ptr()), 8, None, 1, None) == cgamd.CG_E_INVALID
    assert lib.cg_rt_set_grid_caps(h, -1, 0) == cgamd.CG_E_INVALID
    _, _, sph = cgamd.rt_scene()
    cam = cgamd.rt_camera(96, 54, 54.0)
    gctx.rt_set_scene(None, 0, sph, 1)
    want = gctx.rt_render(cam, cgamd.default_lights())[0]
    gctx.rt_set_scene_device(0, 0, sph, 1)
    got = gctx.rt_render(cam, cgamd.default_lights())[0]
    assert gctx.rt_grid() is None
    assert np.array_equal(got, want) and (want != 0x80000000).sum() > 20
