"""GPU: colour modes 1-2 (the random-colour and night-vision modes) on the rasteriser's compact
route -- against the oracle on the reference scene, on meshes and on clipped lists
(oracle.rast_draw(scene=...) / oracle.rast_draw_list), and beside it against the dense route.
cg_rast_set_route_limit(ctx, 1) makes every frame with a non-empty list an automatic compact
frame, so the kernels are reached at small shapes.  Every comparison covers all three planes on
every pixel at tolerance 0 (ARGB, depth as float bits, shadow), plus n_shaded."""
import contextlib

import numpy as np
import pytest

import cgamd
import oracle
import rast_big_scenes as sc
from test_rast_big_gpu import CAMERAS, _maps, _same

pytestmark = pytest.mark.gpu

DENSE, COMPACT = cgamd.RAST_ROUTE_DENSE, cgamd.RAST_ROUTE_COMPACT
NO_BOXES = (cgamd.RTri * 1)()
LIGHT = cgamd.Vec4(0.0, -0.5, 1.0, 1.0)
BIG_OFFSET = 12_000_000          # past the marble noise's draws; the oracle walks rand() up to it


@pytest.fixture(scope="module")
def cctx():
    """A context of this module's own: the route limit never reaches the session's shared context."""
    c = cgamd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def compact_from(ctx, limit=1):
    ctx.rast_set_route_limit(limit)
    try:
        yield
    finally:
        ctx.rast_set_route_limit(0)


@contextlib.contextmanager
def forced(ctx, route):
    ctx.rast_set_route(route)
    try:
        yield
    finally:
        ctx.rast_set_route(-1)


def _dense_render(ctx, tris, n, p, light):
    with forced(ctx, DENSE):
        out = ctx.rast_render(tris, n, p, light)
    assert ctx.rast_scratch_info()["route"] == DENSE
    return out


def _compact_render(ctx, tris, n, p, light):
    with compact_from(ctx):
        out = ctx.rast_render(tris, n, p, light)
    assert ctx.rast_scratch_info()["route"] == COMPACT
    return out


def _dense_of_prepared(ctx, p, room, nr, boxes, nb):
    """The library's other route on a mesh: clip on the host, render the list densely."""
    tris, n, light = cgamd.rast_prepare(p, room, nr, boxes, nb)
    return _dense_render(ctx, tris, n, p, light), n


def _same_frame(got, ref, what):
    _same(got[:3], ref[:3], what)
    assert got[3].n_shaded == ref[3].n_shaded, f"{what}: n_shaded {got[3].n_shaded} != {ref[3].n_shaded}"


def _same_as_oracle(got, ora, what):
    """ora: rast_big_scenes.oracle_scene_frame / oracle_list_frame -- planes and the shaded count."""
    _same(got[:3], ora[:3], what + " against the oracle")
    if got[3].n_shaded >= 0:                                  # -1: a colour mode 0 frame does not count
        assert got[3].n_shaded == ora[3].n_shaded, f"{what}: n_shaded {got[3].n_shaded}, the oracle {ora[3].n_shaded}"


def test_route_limit_hook(cctx):
    lib = cgamd.load()
    assert lib.cg_rast_set_route_limit(cctx.h, -1) == cgamd.CG_E_INVALID
    assert b"cg_rast_set_route_limit" in lib.cg_last_error(cctx.h)
    cctx.rast_set_scene()
    p = cgamd.rast_params(64, 48, 48.0, colour_mode=1)
    with compact_from(cctx, 32 * 150):                       # the reference scene's capacity: not above it
        cctx.rast_draw(p)
        assert cctx.rast_scratch_info()["route"] == DENSE
    with compact_from(cctx, 32 * 150 - 1):
        cctx.rast_draw(p)
        assert cctx.rast_scratch_info()["route"] == COMPACT
        with forced(cctx, DENSE):                            # the forced route still wins
            cctx.rast_draw(p)
            assert cctx.rast_scratch_info()["route"] == DENSE
        with forced(cctx, COMPACT), pytest.raises(RuntimeError, match="colour mode"):
            cctx.rast_draw(p)                                # the hook is a colour-mode-0 switch
    cctx.rast_draw(p)
    assert cctx.rast_scratch_info()["route"] == DENSE        # limit 0: the default rule again


# ---- 1. the reference scene against the oracle -------------------------------------------------
def _reference_case(ctx, W, H, camera, mode, offset, setting=0, boxes=0):
    cfg = CAMERAS[camera]
    F = 0.8 * W
    R = cgamd.yaw_matrix(cfg["yaw"]) if cfg["yaw"] else None
    p = cgamd.rast_params(W, H, F, cfg["cam"], R, colour_mode=mode, rand_offset=offset, yaw=cfg["yaw"])
    po = oracle.rast_params(W, H, F, cfg["cam"], list(R) if R is not None else None, colour_mode=mode,
                            rand_offset=offset, setting=setting, setting_boxes=boxes, yaw=cfg["yaw"])
    ref = oracle.rast_draw(po)
    ctx.rast_set_scene(*cgamd.rast_scene(setting, boxes))
    with compact_from(ctx):
        a, d, s, st = ctx.rast_draw(p)
    info = ctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] > 0 and info["spans"] >= info["recs"] > 0
    _same((a, d, s), ref, f"{W}x{H} {camera} mode {mode} offset {offset} tex {setting}/{boxes}")
    assert 0 < st.n_shaded and np.count_nonzero(d) <= st.n_shaded
    return info


@pytest.mark.parametrize("offset", [0, BIG_OFFSET])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("W,H", [(320, 256), (157, 93)])
def test_reference_scene_matches_oracle(cctx, W, H, camera, mode, offset):
    info = _reference_case(cctx, W, H, camera, mode, offset)
    if camera == "in_short_box":
        assert info["tris"] > 150          # the clip did split (150 inputs)


def test_textured_scene_is_shaded_without_textures(cctx):
    """Modes 1-2 switch before the texture branches (:575-662): with the maps loaded and texture
    settings (2, 0) there is no opacity test and the frame draws rand() from the given index."""
    maps = _maps()
    cctx.rast_set_textures(maps)
    oracle.rast_set_textures(maps)
    try:
        _reference_case(cctx, 157, 93, "yawed", 1, BIG_OFFSET, setting=2, boxes=0)
    finally:
        cctx.rast_set_textures(None)
        oracle.rast_set_textures(None)


# ---- 2. beyond the dense limit, no hook ---------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_beyond_the_dense_limit(cctx, mode):
    B = sc.BEYOND
    room = cgamd.rast_random_scene(B["n"], B["extent"], B["seed"])
    p = cgamd.rast_params(B["W"], B["H"], B["focal"], colour_mode=mode, rand_offset=777)
    ref, n = _dense_of_prepared(cctx, p, room, B["n"], NO_BOXES, 0)
    assert n > 4096
    cctx.rast_set_scene(room, B["n"], NO_BOXES, 0)
    got = cctx.rast_draw(p)                                  # plain cg_rast_draw: the automatic route
    info = cctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] == n
    _same_frame(got, ref, f"6000-triangle room, mode {mode}")
    _same_as_oracle(got, sc.oracle_scene_frame(p, room, B["n"], NO_BOXES, 0), f"6000-triangle room, mode {mode}")
    assert got[3].n_shaded > 0


@pytest.mark.parametrize("mode", [1, 2])
def test_between_the_colour_limit_and_the_dense_limit(cctx, mode):
    """700 inputs: a list capacity of 22,400, within the dense route's 131,072 but beyond the 20,480
    slots its colour fill counts in LDS.  The automatic choice is the compact route in modes 1-2
    (before, such a frame failed with "colour count launch: invalid argument") and still the dense
    one in mode 0; a forced dense route says why it cannot."""
    W, H, F, n = 96, 48, 48.0, 700
    room = cgamd.rast_random_scene(n, 0.3, seed=0x70C)
    p = cgamd.rast_params(W, H, F, colour_mode=mode, rand_offset=31)
    assert cgamd.rast_route(32 * n) == DENSE
    cctx.rast_set_scene(room, n, NO_BOXES, 0)
    got = cctx.rast_draw(p)
    assert cctx.rast_scratch_info()["route"] == COMPACT
    _same_as_oracle(got, sc.oracle_scene_frame(p, room, n, NO_BOXES, 0), f"700-triangle room, mode {mode}")
    assert got[3].n_shaded > 0
    p0 = cgamd.rast_params(W, H, F)
    m0 = cctx.rast_draw(p0)
    assert cctx.rast_scratch_info()["route"] == DENSE
    _same_as_oracle(m0, sc.oracle_scene_frame(p0, room, n, NO_BOXES, 0), "700-triangle room, mode 0")
    with forced(cctx, DENSE), pytest.raises(RuntimeError, match="dense route: colour modes"):
        cctx.rast_draw(p)


# ---- 3. shadow volumes -------------------------------------------------------------------------
def test_shadow_volumes(cctx):
    """Shadow-volume records mark pixels but never shade: they draw no rand()."""
    W, H, F = 96, 48, 48.0
    room, nr, _, _ = cgamd.rast_scene()
    boxes = cgamd.rast_random_scene(700, 0.1, seed=0xB0C5)
    p = cgamd.rast_params(W, H, F, colour_mode=1, rand_offset=5)
    ref, n = _dense_of_prepared(cctx, p, room, nr, boxes, 700)
    assert nr + 7 * 700 > 4096 and ref[2].any()              # shadow marks are in play
    cctx.rast_set_scene(room, nr, boxes, 700)
    got = cctx.rast_draw(p)
    info = cctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] == n
    _same_frame(got, ref, "700 boxes with shadow volumes, mode 1")
    _same_as_oracle(got, sc.oracle_scene_frame(p, room, nr, boxes, 700), "700 boxes with shadow volumes, mode 1")


# ---- 4. numbering across segment and block boundaries ------------------------------------------
@pytest.mark.parametrize("which,form", [(b, f) for b in ("batch", "chunk") for f in ("B-1", "B", "B+1", "2B+1")])
def test_numbering_across_segments(cctx, which, form):
    """W = 200: four fill segments, the last 8 pixels wide; spans up to W wide, so one record
    passes in several segments and its fragments are numbered across them.  Every triangle is
    listed twice (an exact depth tie): both of a pair shade and both draw."""
    B = dict(zip(("batch", "chunk"), cgamd.rast_row_blocks()))[which]
    n = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[form]
    W, H, F = 200, 16, 32.0
    tris = sc.as_rtri(sc.camera_list(n, W, H, F, (5, 11), np.random.default_rng(n)))
    p = cgamd.rast_params(W, H, F, colour_mode=1, rand_offset=2 ** 32 + 5)
    ref = _dense_render(cctx, tris, n, p, LIGHT)
    got = _compact_render(cctx, tris, n, p, LIGHT)
    assert cctx.rast_scratch_info()["spans"] == n * 7
    _same_frame(got, ref, f"{which} {form}")
    # the oracle walks rand() call by call, so it checks the same list at a small index
    small = cgamd.rast_params(W, H, F, colour_mode=1, rand_offset=5)
    _same_as_oracle(_compact_render(cctx, tris, n, small, LIGHT), sc.oracle_list_frame(small, tris, n, LIGHT),
                    f"{which} {form} at rand() index 5")
    # ties shade twice: more fragments drew than the final frame shows
    assert got[3].n_shaded > np.count_nonzero(got[1])
    # the order matters: one fragment further along the stream, every colour changes
    p.rand_offset += 3
    other = _compact_render(cctx, tris, n, p, LIGHT)
    assert (other[0] != got[0]).any() and np.array_equal(other[1], got[1]) and np.array_equal(other[2], got[2])
    _same_frame(other, _dense_render(cctx, tris, n, p, LIGHT), f"{which} {form} offset + 3")


# ---- 5. a long row -----------------------------------------------------------------------------
def _row_list(n, W, H, F, seed=5):
    return sc.camera_list(n, W, H, F, (3, 3), np.random.default_rng(seed))


def test_long_row_at_the_dense_limit(cctx):
    """The dense checker keeps one 8-byte fragment counter per list entry in LDS
    (rast_fill_rand_kernel: max_recs * 8 bytes of dynamic LDS, max_recs = the list length), so it
    renders at most (LDS bytes a workgroup may take) / 8 triangles in mode 1: 20,480 with the
    MI355X's 160 KiB.  All of them lie on row 3."""
    import torch
    lds = torch.cuda.get_device_properties(0).shared_memory_per_block
    n, W, H, F = lds // 8, 64, 8, 16.0
    assert n >= 8192
    tris = sc.as_rtri(_row_list(n, W, H, F))
    p = cgamd.rast_params(W, H, F, colour_mode=1, rand_offset=9)
    ref = _dense_render(cctx, tris, n, p, LIGHT)
    got = _compact_render(cctx, tris, n, p, LIGHT)
    info = cctx.rast_scratch_info()
    assert info["spans"] == n and info["recs"] > 0.9 * n
    _same_frame(got, ref, f"{n} triangles on row 3")
    _same_as_oracle(got, sc.oracle_list_frame(p, tris, n, LIGHT), f"{n} triangles on row 3")


def test_long_row_beyond_the_dense_limit(cctx):
    n, W, H, F = 40000, 64, 8, 16.0
    t = _row_list(n, W, H, F)
    p0, p1 = cgamd.rast_params(W, H, F), cgamd.rast_params(W, H, F, colour_mode=1)
    got = _compact_render(cctx, sc.as_rtri(t), n, p1, LIGHT)
    info = cctx.rast_scratch_info()
    assert info["spans"] == n and info["recs"] >= 32768
    depth = got[1].reshape(H, W)
    assert got[3].n_shaded >= np.count_nonzero(depth[3]) > 0
    assert depth[3].any() and not np.delete(depth, 3, 0).any()
    # the z-buffer walk is mode 0's: half the list (even indices) gives equal depth and shadow planes
    half = sc.as_rtri(t[::2])
    m0 = _compact_render(cctx, half, n // 2, p0, LIGHT)
    m1 = _compact_render(cctx, half, n // 2, p1, LIGHT)
    _same(m1[1:3], m0[1:3], "half list, mode 1 against mode 0")
    assert (m1[0] != m0[0]).any()


# ---- 6. sequences ------------------------------------------------------------------------------
SEQ_MODES = [0, 1, 1, 2, 0, 2]


@pytest.fixture(scope="module")
def beyond_sequence(cctx):
    """The six frames' parameters and, rendered once, each frame alone at its chained offset."""
    B = sc.BEYOND
    room = cgamd.rast_random_scene(B["n"], B["extent"], B["seed"])
    cctx.rast_set_scene(room, B["n"], NO_BOXES, 0)
    start = 4321
    ps = [cgamd.rast_params(B["W"], B["H"], B["focal"], cam=(0.05 * k, 0.0, -3.001 + 0.1 * k, 1.0),
                            colour_mode=SEQ_MODES[k], rand_offset=start if k == 0 else 0) for k in range(6)]
    singles, offs, off = [], [], start
    for k in range(6):
        q = cgamd.rast_params(B["W"], B["H"], B["focal"], cam=(0.05 * k, 0.0, -3.001 + 0.1 * k, 1.0),
                              colour_mode=SEQ_MODES[k], rand_offset=off)
        one = cctx.rast_draw(q)
        assert cctx.rast_scratch_info()["route"] == COMPACT
        dense, _ = _dense_of_prepared(cctx, q, room, B["n"], NO_BOXES, 0)
        _same_frame(one, dense, f"frame {k} alone against the dense checker")
        singles.append(one)
        offs.append(off)
        assert (one[3].n_shaded == -1) == (SEQ_MODES[k] == 0)
        off += 3 * max(one[3].n_shaded, 0)
    return ps, singles, offs + [off]


def _check_records(rec, singles, offs):
    assert [int(x) for x in rec["rand_offset"]] == offs
    assert [int(x) for x in rec["n_shaded"]] == [s[3].n_shaded for s in singles] + [-1]
    assert not rec["status"].any()
    assert offs[1] == offs[0] and offs[2] > offs[1] and offs[5] == offs[4]      # mode 0 passes the index on


def test_sequence_device(cctx, beyond_sequence):
    import torch
    ps, singles, offs = beyond_sequence
    px = ps[0].width * ps[0].height
    a = torch.zeros(6 * px, dtype=torch.int32, device="cuda")
    d = torch.zeros(6 * px, dtype=torch.float32, device="cuda")
    s = torch.zeros(6 * px, dtype=torch.int32, device="cuda")
    info = torch.full((7 * 3,), -1, dtype=torch.int64, device="cuda")
    cctx.rast_set_rand_capacity(16)                          # ignored here: the stream follows each frame's S
    try:
        cctx.rast_draw_sequence_device(ps, a.data_ptr(), d.data_ptr(), s.data_ptr(), 0, info.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        cctx.rast_set_rand_capacity(0)
    assert cctx.rast_scratch_info()["route"] == COMPACT
    _check_records(info.cpu().numpy().view(cgamd.RAST_SEQ_DTYPE), singles, offs)
    for k in range(6):
        o = slice(k * px, (k + 1) * px)
        got = (a[o].cpu().numpy().view(np.uint32), d[o].cpu().numpy(), s[o].cpu().numpy())
        _same(got, singles[k][:3], f"device sequence frame {k} (mode {SEQ_MODES[k]})")


def test_sequence_host(cctx, beyond_sequence):
    ps, singles, offs = beyond_sequence
    px = ps[0].width * ps[0].height
    a, d, s, info, st = cctx.rast_draw_sequence(ps, want_depth=True, want_shadow=True, chunk=2)   # pageable memory
    _check_records(info, singles, offs)
    assert st.n_shaded == sum(max(x[3].n_shaded, 0) for x in singles)
    for k in range(6):
        o = slice(k * px, (k + 1) * px)
        _same((a[o], d[o], s[o]), singles[k][:3], f"host sequence frame {k} (mode {SEQ_MODES[k]})")


# ---- 7. degenerate inputs ----------------------------------------------------------------------
def test_degenerate_scenes(cctx):
    import torch
    W, H, F = 96, 48, 48.0
    cases = {
        # (an empty scene has list capacity 0, which no limit lies below: it stays on the dense route)
        "empty": (NO_BOXES, 0, (0.0, 0.0, -3.001, 1.0), None),
        "behind": (cgamd.rast_random_scene(500, 0.05, seed=4), 500, (0.0, 0.0, 5.0, 1.0), COMPACT),
        "sub-pixel": (cgamd.rast_random_scene(2000, 0.001, seed=3), 2000, (0.0, 0.0, -3.001, 1.0), COMPACT),
    }
    info_d = torch.full((2 * 3,), -1, dtype=torch.int64, device="cuda")
    a_d = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for name, (room, nr, cam, route) in cases.items():
        p0 = cgamd.rast_params(W, H, F, cam=cam)
        p1 = cgamd.rast_params(W, H, F, cam=cam, colour_mode=1, rand_offset=99)
        # (a dense Draw keeps its LDS counters per list slot, 32 an input: the checker renders the host-clipped list)
        ref, _ = _dense_of_prepared(cctx, p1, room, nr, NO_BOXES, 0)
        cctx.rast_set_scene(room, nr, NO_BOXES, 0)
        with compact_from(cctx):
            got = cctx.rast_draw(p1)
            info = cctx.rast_scratch_info()
            m0 = cctx.rast_draw(p0)
            cctx.rast_draw_sequence_device([p1], a_d.data_ptr(), None, None, 0, info_d.data_ptr())
            torch.cuda.synchronize()
        if route is not None:
            assert info["route"] == route, name
        _same_frame(got, ref, name)
        _same_as_oracle(got, sc.oracle_scene_frame(p1, room, nr, NO_BOXES, 0), name)
        rec = info_d.cpu().numpy().view(cgamd.RAST_SEQ_DTYPE)
        assert int(rec["n_shaded"][0]) == got[3].n_shaded and not rec["status"].any()
        assert int(rec["rand_offset"][1]) == 99 + 3 * got[3].n_shaded
        if name != "sub-pixel":
            assert got[3].n_shaded == 0 and int(rec["rand_offset"][1]) == 99      # the index passes on unchanged
            _same(got[:3], m0[:3], f"{name}: planes as mode 0's")
        else:
            assert got[3].n_shaded > 0 and 0 < info["recs"] < info["spans"]


# ---- 8. the state buffer changes format between the modes --------------------------------------
def test_mode_0_after_mode_1_on_one_context(cctx):
    W, H, F = 157, 93, 120.0
    cctx.rast_set_scene()
    p0, p1 = cgamd.rast_params(W, H, F, indirect_first=0.15), cgamd.rast_params(W, H, F, colour_mode=1)
    with forced(cctx, DENSE):
        ref0, ref1 = cctx.rast_draw(p0), cctx.rast_draw(p1)
    with compact_from(cctx):
        for k, (p, ref) in enumerate([(p1, ref1), (p0, ref0), (p1, ref1), (p0, ref0)]):
            got = cctx.rast_draw(p)
            assert cctx.rast_scratch_info()["route"] == COMPACT
            _same_frame(got, ref, f"frame {k}, mode {p.colour_mode}")


def test_mode_0_holds_no_colour_scratch():
    """The 16-byte state, the segment buffers and the stream belong to mode 1-2 frames alone, and
    cg_rast_scratch_info counts them."""
    W, H, F = 157, 93, 120.0
    with cgamd.Context(0) as ctx:
        ctx.rast_set_scene()
        ctx.rast_set_route_limit(1)
        ctx.rast_draw(cgamd.rast_params(W, H, F))
        before = ctx.rast_scratch_info()["bytes"]
        _, _, _, st = ctx.rast_draw(cgamd.rast_params(W, H, F, colour_mode=1))
        info = ctx.rast_scratch_info()
        # at least: 12 more bytes of state a pixel, 12 bytes of rand() values a fragment, 8 a record
        assert info["bytes"] >= before + 12 * W * H + 12 * st.n_shaded + 8 * info["recs"]
        ctx.rast_draw(cgamd.rast_params(W, H, F))
        assert ctx.rast_scratch_info()["bytes"] == info["bytes"]            # grow-only: mode 0 adds nothing
