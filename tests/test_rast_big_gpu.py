"""GPU: the rasteriser's compact route (cg_rast_big.hip) -- scratch and work that follow what the
frame covers -- against the oracle, on the reference scene and on meshes and clipped lists
(oracle.rast_draw(scene=...) / oracle.rast_draw_list: the oracle's own clip and fill, which
tests/test_ref_scene_sessions.py holds to the reference program on meshes), and beside it against
the dense route.  Every comparison covers all three planes on every pixel at tolerance 0: ARGB,
depth as float bits, shadow."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import oracle
import rast_big_scenes as sc

pytestmark = pytest.mark.gpu

DENSE, COMPACT = cgamd.RAST_ROUTE_DENSE, cgamd.RAST_ROUTE_COMPACT
NO_BOXES = (cgamd.RTri * 1)()


@pytest.fixture(scope="module")
def bctx():
    """A context of this module's own: the forced route and the custom scenes never reach the
    session's shared context."""
    c = cgamd.Context(0)
    yield c
    c.close()


def _same(got, ref, what):
    for nm, a, b in zip(("argb", "depth", "shadow"), got, ref):
        a = a.view(np.uint32) if a.dtype == np.float32 else a
        b = b.view(np.uint32) if b.dtype == np.float32 else b
        assert a.shape == b.shape
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what} {nm}: {bad.size} differ, first {bad[:5]} got {a[bad[:3]]} want {b[bad[:3]]}"


def _draw(ctx, route, p):
    ctx.rast_set_route(route)
    try:
        return ctx.rast_draw(p)
    finally:
        ctx.rast_set_route(-1)


def _render(ctx, route, tris, n, p, light):
    ctx.rast_set_route(route)
    try:
        return ctx.rast_render(tris, n, p, light)
    finally:
        ctx.rast_set_route(-1)


def _dense_of_prepared(ctx, p, room, nr, boxes, nb):
    """The library's other route on a mesh: clip on the host, render the list densely."""
    tris, n, light = cgamd.rast_prepare(p, room, nr, boxes, nb)
    return _render(ctx, DENSE, tris, n, p, light), n


# ---- 1. the reference scene, forced compact, against the oracle -------------------------------
CAMERAS = {
    "unrotated": dict(cam=(0.0, 0.0, -3.001, 1.0), yaw=0.0),
    "yawed": dict(cam=(0.2, 0.1, -2.4, 1.0), yaw=0.35),
    "in_short_box": dict(cam=(0.33, 0.70, -0.39, 1.0), yaw=0.0),   # the clip splits the most here
}


def _maps(seed=7):
    """Grill and woven maps as tests/test_rast_tex_gpu.py builds them."""
    rng = np.random.default_rng(seed)
    u = np.arange(1024)
    block = (((u[:, None] // 48) + (u[None, :] // 48)) % 2 == 0)
    speck = rng.random((1024, 1024)) < 0.1
    op = np.where(block ^ speck, 230, 40).astype(np.uint8)
    op3 = np.repeat(op[:, :, None], 3, axis=2)
    return {"grill": rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8),
            "grill_opacity": op3,
            "grill_normal": rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8),
            "woven": rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8),
            "woven_ao": rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8),
            "woven_opacity": op3[::-1].copy(),
            "woven_normal": rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)}


@pytest.fixture(scope="module")
def tex(bctx):
    maps = _maps()
    bctx.rast_set_textures(maps)
    oracle.rast_set_textures(maps)
    yield maps
    bctx.rast_set_textures(None)
    oracle.rast_set_textures(None)


def _reference_case(ctx, W, H, camera, ind, setting=0, boxes=0):
    cfg = CAMERAS[camera]
    F = 0.8 * W
    R = cgamd.yaw_matrix(cfg["yaw"]) if cfg["yaw"] else None
    p = cgamd.rast_params(W, H, F, cfg["cam"], R, indirect_first=ind, yaw=cfg["yaw"])
    po = oracle.rast_params(W, H, F, cfg["cam"], list(R) if R is not None else None, indirect_first=ind,
                            setting=setting, setting_boxes=boxes, yaw=cfg["yaw"])
    ref = oracle.rast_draw(po)
    ctx.rast_set_scene(*cgamd.rast_scene(setting, boxes))
    a, d, s, _ = _draw(ctx, COMPACT, p)
    info = ctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] > 0 and info["spans"] >= info["recs"] > 0
    _same((a, d, s), ref, f"{W}x{H} {camera} ind {ind} tex {setting}/{boxes}")
    return info


@pytest.mark.parametrize("ind", [0.15, 0.2])
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("W,H", [(320, 256), (157, 93)])
def test_reference_scene_matches_oracle(bctx, W, H, camera, ind):
    info = _reference_case(bctx, W, H, camera, ind)
    if camera == "in_short_box":
        assert info["tris"] > 150          # the clip did split (150 inputs)


@pytest.mark.parametrize("setting,boxes", [(2, 0), (3, 2)])
@pytest.mark.parametrize("W,H,camera,ind", [(320, 256, "yawed", 0.15), (157, 93, "unrotated", 0.2),
                                            (157, 93, "in_short_box", 0.15)])
def test_reference_scene_textured_matches_oracle(bctx, tex, W, H, camera, ind, setting, boxes):
    _reference_case(bctx, W, H, camera, ind, setting, boxes)


# ---- 2. beyond the old scene limit --------------------------------------------------------------
def test_beyond_the_old_limit(bctx):
    B = sc.BEYOND
    room = cgamd.rast_random_scene(B["n"], B["extent"], B["seed"])
    p = cgamd.rast_params(B["W"], B["H"], B["focal"])
    (ra, rd, rs, rst), n = _dense_of_prepared(bctx, p, room, B["n"], NO_BOXES, 0)
    assert n > 4096
    bctx.rast_set_scene(room, B["n"], NO_BOXES, 0)         # rejected before: more than 4,096 inputs
    a, d, s, st = bctx.rast_draw(p)                         # the automatic route
    info = bctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] == n
    _same((a, d, s), (ra, rd, rs), "6000-triangle room")
    _same((a, d, s), sc.oracle_scene_frame(p, room, B["n"], NO_BOXES, 0)[:3], "6000-triangle room against the oracle")
    assert (st.n_tris, st.n_spans) == (rst.n_tris, rst.n_spans) == (n, rst.n_spans)
    # a forced dense Draw of this scene fails as cg_rast_set_scene did
    with pytest.raises(RuntimeError, match="dense route"):
        _draw(bctx, DENSE, p)


# ---- 3. shadow volumes --------------------------------------------------------------------------
def test_shadow_volumes(bctx):
    W, H, F = 96, 48, 48.0
    room, nr, _, _ = cgamd.rast_scene()
    boxes = cgamd.rast_random_scene(700, 0.1, seed=0xB0C5)
    p = cgamd.rast_params(W, H, F)
    (ra, rd, rs, _), n = _dense_of_prepared(bctx, p, room, nr, boxes, 700)
    assert nr + 7 * 700 > 4096 and rs.any()                 # shadow marks are in play
    bctx.rast_set_scene(room, nr, boxes, 700)
    a, d, s, _ = bctx.rast_draw(p)
    info = bctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] == n
    _same((a, d, s), (ra, rd, rs), "700 boxes with shadow volumes")
    _same((a, d, s), sc.oracle_scene_frame(p, room, nr, boxes, 700)[:3], "700 boxes against the oracle")


# ---- 4. record order across the row-list passes' block boundaries ------------------------------
BATCH, CHUNK = None, None


def _block_sizes():
    global BATCH, CHUNK
    if BATCH is None:
        BATCH, CHUNK = cgamd.rast_row_blocks()
    return BATCH, CHUNK


@pytest.mark.parametrize("rows", [(8, 8), (5, 11)], ids=["one_row", "seven_rows"])
@pytest.mark.parametrize("which,form", [(b, f) for b in ("batch", "chunk") for f in ("B-1", "B", "B+1", "2B+1")])
def test_order_across_block_boundaries(bctx, which, form, rows):
    """Every triangle appears twice in a row with two colours, an exact depth tie that the later
    one must win, and all of them cover row 8.  With one row per triangle the list's triangles are
    the row-list passes' spans, so n sits exactly on the boundary."""
    B = dict(zip(("batch", "chunk"), _block_sizes()))[which]
    n = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[form]
    W, H, F = 64, 16, 32.0
    t = sc.camera_list(n, W, H, F, rows, np.random.default_rng(n))
    tris = sc.as_rtri(t)
    p = cgamd.rast_params(W, H, F)
    light = cgamd.Vec4(0.0, -0.5, 1.0, 1.0)
    ref = _render(bctx, DENSE, tris, n, p, light)
    got = _render(bctx, COMPACT, tris, n, p, light)
    info = bctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] == n
    assert info["spans"] == n * (rows[1] - rows[0] + 1)
    _same(got[:3], ref[:3], f"{which} {form} rows {rows}")
    _same(got[:3], sc.oracle_list_frame(p, tris, n, light)[:3], f"{which} {form} rows {rows} against the oracle")
    # the ties are real: swapping the two colours of every pair changes the frame
    sw = t.copy()
    k = np.arange(n - n % 2)
    sw["color"][k] = t["color"][k ^ 1]
    other = _render(bctx, COMPACT, sc.as_rtri(sw), n, p, light)
    assert (other[0] != got[0]).any()


# ---- 5. a row with 32,768 or more records -------------------------------------------------------
def test_long_row_takes_the_32_bit_state(bctx):
    n, W, H, F = 40000, 64, 8, 16.0
    t = sc.camera_list(n, W, H, F, (3, 3), np.random.default_rng(5))
    tris = sc.as_rtri(t)
    p = cgamd.rast_params(W, H, F)
    light = cgamd.Vec4(0.0, -0.5, 1.0, 1.0)
    ref = _render(bctx, DENSE, tris, n, p, light)
    got = _render(bctx, COMPACT, tris, n, p, light)
    info = bctx.rast_scratch_info()
    # one span a triangle, all on row 3: that row alone holds the records
    assert info["spans"] == n and info["recs"] >= 32768
    assert got[1].reshape(H, W)[3].any() and not np.delete(got[1].reshape(H, W), 3, 0).any()
    _same(got[:3], ref[:3], "40,000 triangles on row 3")
    _same(got[:3], sc.oracle_list_frame(p, tris, n, light)[:3], "40,000 triangles on row 3 against the oracle")


# ---- 6. degenerate inputs -----------------------------------------------------------------------
def test_degenerate_scenes(bctx):
    W, H, F = 96, 48, 48.0
    p = cgamd.rast_params(W, H, F)
    room = cgamd.rast_random_scene(2000, 0.001, seed=3)
    cases = {
        "empty": (NO_BOXES, 0, p),
        "behind": (cgamd.rast_random_scene(500, 0.05, seed=4), 500,
                   cgamd.rast_params(W, H, F, cam=(0.0, 0.0, 5.0, 1.0))),
        "sub-pixel": (room, 2000, p),
    }
    for name, (r, nr, pp) in cases.items():
        bctx.rast_set_scene(r, nr, NO_BOXES, 0)
        ref = _draw(bctx, DENSE, pp)
        got = _draw(bctx, COMPACT, pp)
        info = bctx.rast_scratch_info()
        assert info["route"] == COMPACT
        if name != "sub-pixel":
            assert (info["tris"], info["spans"], info["recs"]) == (0, 0, 0), name
            assert got[3].n_tris == 0
        else:
            # triangles with no row at all and rows with rx <= lx: fewer records than spans,
            # fewer spans than three a triangle
            assert 0 < info["recs"] < info["spans"] < 3 * info["tris"]
        _same(got[:3], ref[:3], name)
        _same(got[:3], sc.oracle_scene_frame(pp, r, nr, NO_BOXES, 0)[:3], f"{name} against the oracle")
    # an empty list through cg_rast_render
    ref = _render(bctx, DENSE, NO_BOXES, 0, p, cgamd.Vec4(0, 0, 0, 1))
    got = _render(bctx, COMPACT, NO_BOXES, 0, p, cgamd.Vec4(0, 0, 0, 1))
    _same(got[:3], ref[:3], "empty list")
    _same(got[:3], sc.oracle_list_frame(p, NO_BOXES, 0, cgamd.Vec4(0, 0, 0, 1))[:3], "empty list against the oracle")


# ---- 7. scratch scales with the frame -----------------------------------------------------------
def test_scratch_scales_with_the_frame():
    W, H, F = 160, 60, 96.0
    chunk = cgamd.rast_row_blocks()[1]
    p = cgamd.rast_params(W, H, F)
    with cgamd.Context(0) as ctx:                           # fresh: nothing held from earlier frames
        need = []
        for n_in in (5000, 50000):
            ctx.rast_set_scene(cgamd.rast_random_scene(n_in, 0.02), n_in, NO_BOXES, 0)
            ctx.rast_draw(p, want_depth=False, want_shadow=False)
            info = ctx.rast_scratch_info()
            assert info["route"] == COMPACT and 0 < info["recs"] <= info["spans"]
            need.append(sc.scratch_need(n_in, info, W, H, chunk))
            # grow-only and exact: each buffer holds the larger of what the two frames needed
            bound = sum(max(f[k] for f in need) for k in need[0])
            print(f"n_in {n_in}: held {info['bytes']} B, bound {bound} B, dense formula {2560 * n_in * H} B, {info}")
            assert info["bytes"] <= bound
            assert info["bytes"] < 2560 * n_in * H
        assert need[1]["spans"] > need[0]["spans"] and need[1]["recs"] > need[0]["recs"]


# ---- 8. colour modes 1-2 are refused; frame runs on one stream ---------------------------------
def test_colour_mode_1_is_refused(bctx):
    bctx.rast_set_scene()
    with pytest.raises(RuntimeError, match="colour mode"):
        _draw(bctx, COMPACT, cgamd.rast_params(64, 48, 48.0, colour_mode=1))
    lib = cgamd.load()
    assert b"compact route" in lib.cg_last_error(bctx.h)
    _draw(bctx, DENSE, cgamd.rast_params(64, 48, 48.0, colour_mode=1))   # the dense route still renders it


def test_draw_frames_equals_single_draws(bctx):
    import torch
    W, H, F = 157, 93, 120.0
    bctx.rast_set_scene()
    ps = [cgamd.rast_params(W, H, F, cam=(0.1 * k, 0.0, -3.001 + 0.3 * k, 1.0), indirect_first=0.15 if k == 0 else 0.2)
          for k in range(3)]
    a = torch.zeros(3 * W * H, dtype=torch.int32, device="cuda")
    d = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    s = torch.zeros(3 * W * H, dtype=torch.int32, device="cuda")
    bctx.rast_set_route(COMPACT)
    try:
        bctx.rast_draw_frames_device(ps, a.data_ptr(), d.data_ptr(), s.data_ptr(),
                                     stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bctx.rast_scratch_info()["route"] == COMPACT
        for k in range(3):
            want = bctx.rast_draw(ps[k])
            o = slice(k * W * H, (k + 1) * W * H)
            got = (a[o].cpu().numpy().view(np.uint32), d[o].cpu().numpy(), s[o].cpu().numpy())
            _same(got, want[:3], f"frame {k}")
    finally:
        bctx.rast_set_route(-1)


def test_draw_sequence_runs_compact_frames_in_turn(bctx):
    """cg_rast_draw_sequence_device: colour mode 0 frames on the compact route, one after another on
    the caller's stream; the rand() call index passes through unchanged.  A colour mode 1 frame is
    refused there too."""
    import torch
    W, H, F, start = 157, 93, 120.0, 1234
    info_t = np.dtype([("rand_offset", "<u8"), ("n_shaded", "<i8"), ("status", "<i4"), ("pad", "<i4")])
    bctx.rast_set_scene()
    ps = [cgamd.rast_params(W, H, F, cam=(0.0, 0.05 * k, -3.001 + 0.2 * k, 1.0), rand_offset=start if k == 0 else 0)
          for k in range(3)]
    a = torch.zeros(3 * W * H, dtype=torch.int32, device="cuda")
    d = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    s = torch.zeros(3 * W * H, dtype=torch.int32, device="cuda")
    info = torch.full((3 * 4,), -1, dtype=torch.int64, device="cuda")
    bctx.rast_set_route(COMPACT)
    try:
        bctx.rast_draw_sequence_device(ps, a.data_ptr(), d.data_ptr(), s.data_ptr(), 0, info.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bctx.rast_scratch_info()["route"] == COMPACT
        rec = info.cpu().numpy().view(info_t)
        assert [int(x) for x in rec["rand_offset"]] == [start] * 4
        assert [int(x) for x in rec["n_shaded"]] == [-1] * 4 and not rec["status"].any()
        for k in range(3):
            want = bctx.rast_draw(ps[k])
            o = slice(k * W * H, (k + 1) * W * H)
            _same((a[o].cpu().numpy().view(np.uint32), d[o].cpu().numpy(), s[o].cpu().numpy()), want[:3], f"frame {k}")
        ps[1].colour_mode = 1
        with pytest.raises(RuntimeError, match="colour mode"):
            bctx.rast_draw_sequence_device(ps, a.data_ptr(), d.data_ptr(), s.data_ptr(), 0, info.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        bctx.rast_set_route(-1)


# ---- 9. hook hygiene ---------------------------------------------------------------------------
def test_automatic_route_is_dense_again(bctx):
    bctx.rast_set_scene()
    p = cgamd.rast_params(160, 120, 96.0)
    _draw(bctx, COMPACT, p)
    assert bctx.rast_scratch_info()["route"] == COMPACT
    a, d, s, st = bctx.rast_draw(p)                          # after cg_rast_set_route(-1)
    info = bctx.rast_scratch_info()
    assert info["route"] == DENSE and info["tris"] == st.n_tris > 0 and info["recs"] > 0
    _same((a, d, s), oracle.rast_draw(oracle.rast_params(160, 120, 96.0)), "dense again")
    with pytest.raises(RuntimeError):
        bctx.rast_set_route(2)
