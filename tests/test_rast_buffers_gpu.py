"""GPU: the rasteriser's HDR shade buffers, owner ids and picking (cg_rast_buffers.hip) on both
routes.  Every comparison covers every pixel at tolerance 0, floats compared as bits: the float
planes and the picture against the oracle's cgo_rast_draw, the owner's clip / pos against the
ordered z-buffer restated over the oracle's primitives (rast_owner_ref.owner_planes), tri against
host-only cg_rast_prepare counts (rast_owner_ref.input_of_clip).  The caller's list and the mesh
are drawn by the oracle too (oracle.rast_draw_list / oracle.rast_draw(scene=...))."""
import ctypes as C
import functools

import numpy as np
import pytest

import cgamd
import oracle
import rast_big_scenes as sc
import rast_owner_ref as ro
from test_rast_big_gpu import _maps
from test_rast_buffers import case_params

pytestmark = pytest.mark.gpu

DENSE, COMPACT = cgamd.RAST_ROUTE_DENSE, cgamd.RAST_ROUTE_COMPACT
ALL = tuple(n for n, _, _ in cgamd.RAST_PLANES)
NO_BOXES = (cgamd.RTri * 1)()
NONE = cgamd.RAST_OWNER_NONE


@pytest.fixture(scope="module")
def bctx():
    """A context of this module's own: routes, scenes and textures never reach the shared one."""
    c = cgamd.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, ref, names, what):
    for nm in names:
        a, b = _bits(got[nm]), _bits(ref[nm])
        assert a.shape == b.shape, f"{what} {nm}: shape {a.shape} against {b.shape}"
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, (f"{what} {nm}: {bad.size} pixels differ, first {bad[:5]} got {got[nm][bad[:2]]} "
                               f"want {ref[nm][bad[:2]]}")


def _on_route(ctx, route, call):
    """The reference scene is below the dense list capacity: a limit of 1 sends the automatic
    choice to the compact route (a forced route refuses colour modes 1-2)."""
    ctx.rast_set_route_limit(1 if route == COMPACT else 0)
    try:
        out = call()
        assert ctx.rast_scratch_info()["route"] == route
        return out
    finally:
        ctx.rast_set_route_limit(0)


@functools.lru_cache(maxsize=None)
def _oracle_frame(W, H, camera, ind=0.2, mode=0, offset=0, setting=0, boxes=0):
    """cgo_rast_draw with all six of its buffers (the C function, called directly)."""
    _, po = case_params(W, H, camera, ind, mode, offset, setting, boxes)
    npx = W * H
    out = {"argb": np.zeros(npx, np.uint32), "depth": np.zeros(npx, np.float32), "shadow": np.zeros(npx, np.int32),
           "screen": np.zeros((npx, 3), np.float32), "low": np.zeros((npx, 3), np.float32),
           "high": np.zeros((npx, 3), np.float32)}
    oracle.load().cgo_rast_draw(C.byref(po), *[out[k].ctypes.data_as(C.c_void_p) for k in
                                               ("argb", "depth", "shadow", "screen", "low", "high")], None)
    return out


@functools.lru_cache(maxsize=None)
def _owner_ref(W, H, camera):
    """clip / pos / tri of the untextured reference scene by the restated owner rule."""
    p, po = case_params(W, H, camera)
    tris, n, _ = oracle.rast_geometry(po)
    depth, shadow, clip, pos = ro.owner_planes(po, tris, n, W, H)
    src = ro.input_of_clip(p, *cgamd.rast_scene())
    assert src.size == n
    tri = np.where(clip >= 0, src[np.maximum(clip, 0)], NONE).astype(np.int32)
    return {"depth": depth, "shadow": shadow, "clip": clip, "pos": pos, "tri": tri}


# ---- 1. the reference scene against the oracle, untextured ---------------------------------------
SHAPES = [(67, 45), (200, 150), (96, 64)]   # 67: no multiple of the 64-pixel tile; 200: 3 tiles + a ragged one
CASES1 = [(W, H, cam, 0.2) for W, H in SHAPES for cam in ("unrotated", "in_short_box", "yawed")]
CASES1.append((96, 64, "yawed", 0.15))


@pytest.mark.parametrize("W,H,camera,ind", CASES1)
def test_reference_scene_matches_oracle_and_owner_rule(bctx, W, H, camera, ind):
    p, _ = case_params(W, H, camera, ind)
    ref, own = _oracle_frame(W, H, camera, ind), _owner_ref(W, H, camera)
    bctx.rast_set_scene(*cgamd.rast_scene())
    for route in (DENSE, COMPACT):
        got = _on_route(bctx, route, lambda: bctx.rast_draw_buffers(p))
        what = f"{W}x{H} {camera} ind {ind} route {route}"
        _same(got, ref, ("screen", "low", "high", "argb", "depth", "shadow"), what)
        _same(got, own, ("clip", "pos", "tri"), what)
        assert (got["clip"] >= 0).any()


# ---- 2. colour modes 1 and 2 ---------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 12_000_000])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("W,H,camera", [(67, 45, "in_short_box"), (96, 64, "unrotated")])
def test_colour_modes(bctx, W, H, camera, mode, offset):
    p0, _ = case_params(W, H, camera)
    p, _ = case_params(W, H, camera, 0.2, mode, offset)
    ref, own = _oracle_frame(W, H, camera, 0.2, mode, offset), _owner_ref(W, H, camera)
    bctx.rast_set_scene(*cgamd.rast_scene())
    for route in (DENSE, COMPACT):
        what = f"{W}x{H} {camera} mode {mode} offset {offset} route {route}"
        got = _on_route(bctx, route, lambda: bctx.rast_draw_buffers(p))
        _same(got, ref, ("screen", "argb", "depth", "shadow"), what)
        assert not got["low"].view(np.uint32).any() and not got["high"].view(np.uint32).any()
        # the owner does not depend on the colour mode
        mode0 = _on_route(bctx, route, lambda: bctx.rast_draw_buffers(p0, ("clip", "pos", "tri")))
        _same(got, mode0, ("clip", "pos", "tri"), what + " against mode 0")
        _same(got, own, ("clip", "pos", "tri"), what)


# ---- 3. texture modes 2 / 3: the transparent texel keeps the earlier owner ------------------------
@pytest.fixture(scope="module")
def tex(bctx):
    maps = _maps()
    bctx.rast_set_textures(maps)
    oracle.rast_set_textures(maps)
    yield maps
    bctx.rast_set_textures(None)
    oracle.rast_set_textures(None)


def test_textured_owner_is_a_genuine_fragment(bctx, tex):
    W, H, camera, setting, boxes = 96, 64, "unrotated", 2, 3
    p, _ = case_params(W, H, camera)
    ref = _oracle_frame(W, H, camera, 0.2, 0, 0, setting, boxes)
    scene = cgamd.rast_scene(setting, boxes)
    bctx.rast_set_scene(*scene)
    got = {r: _on_route(bctx, r, lambda: bctx.rast_draw_buffers(p)) for r in (DENSE, COMPACT)}
    for r in (DENSE, COMPACT):
        _same(got[r], ref, ("screen", "low", "high", "argb", "depth", "shadow"), f"textured route {r}")
    _same(got[COMPACT], got[DENSE], ALL, "textured compact against dense")
    g = got[DENSE]
    # the transparent-texel case: depth 0 under a pixel that an earlier fragment still owns
    zero_owned = (g["depth"] == 0) & (g["clip"] >= 0)
    assert zero_owned.sum() >= 1
    assert ((ref["depth"] == 0) & ref["screen"].any(axis=1)).sum() == 937
    # every owner is a fragment its triangle really draws there, pos bits equal
    tris, n, _ = cgamd.rast_prepare(p, *scene)
    src = ro.input_of_clip(p, *scene)
    lib = ro._lib()
    po = ro.oracle_params(p)
    checked = 0
    for t in np.unique(g["clip"][g["clip"] >= 0]):
        assert t < n and tris[t].color.x >= 0          # a shadow-volume triangle never owns
        lines = list(ro.triangle_lines(lib, po, tris[t]))
        frag = np.concatenate(lines)
        frag = frag[(frag["x"] >= 0) & (frag["x"] < W)]
        at = {int(f["y"]) * W + int(f["x"]): f["pos"] for f in frag}
        for o in np.flatnonzero(g["clip"] == t):
            assert o in at, f"triangle {t} draws no fragment at pixel {o}"
            assert np.array_equal(at[o].view(np.uint32), g["pos"][o].view(np.uint32)), (t, o)
            checked += 1
        assert (g["tri"][g["clip"] == t] == src[t]).all()
    assert checked == (g["clip"] >= 0).sum() > 0


# ---- 4. the caller's clipped list, 2- and 4-byte state, exact depth ties --------------------------
@pytest.mark.parametrize("n,route,state_bytes", [(33000, DENSE, 4), (600, DENSE, 2), (600, COMPACT, 2)])
def test_callers_list_with_ties(bctx, n, route, state_bytes):
    W, H, F = 96, 48, 48.0
    t = sc.camera_list(n, W, H, F, (20, 22), np.random.default_rng(n))
    tris = sc.as_rtri(t)
    p = cgamd.rast_params(W, H, F)
    light = cgamd.Vec4(0.0, -0.5, 1.0, 1.0)
    bctx.rast_set_route(route)
    try:
        got = bctx.rast_render_buffers(tris, n, p, light)
        assert bctx.rast_state_bytes() == state_bytes      # n >= 32768 forces the 4-byte state
        assert bctx.rast_scratch_info()["route"] == route
        a, d, s, _ = bctx.rast_render(tris, n, p, light)
    finally:
        bctx.rast_set_route(-1)
    depth, shadow, clip, pos = ro.owner_planes(p, tris, n, W, H)
    own = {"depth": depth, "shadow": shadow, "clip": clip, "pos": pos, "tri": clip}
    _same(got, own, ("clip", "pos", "tri", "depth", "shadow"), f"list of {n} route {route}")
    _same(got, {"argb": a, "depth": d, "shadow": s}, ("argb", "depth", "shadow"), f"list of {n} against rast_render")
    ora = oracle.rast_draw_list(sc.oracle_params(p), tris, n, light, buffers=True)
    _same(got, ora, ("screen", "low", "high", "argb", "depth", "shadow"), f"list of {n} route {route} against the oracle")
    # every triangle is listed twice in a row (an exact depth tie on every fragment): the later
    # twin, the odd index, always owns
    owned = got["clip"][got["clip"] >= 0]
    assert owned.size and (owned % 2 == 1).all()


# ---- 5. a mesh beyond the dense inputs ------------------------------------------------------------
def test_mesh_beyond_the_dense_inputs(bctx):
    B = sc.BEYOND
    room = cgamd.rast_random_scene(B["n"], B["extent"], B["seed"])
    p = cgamd.rast_params(B["W"], B["H"], B["focal"])
    tris, n, light = cgamd.rast_prepare(p, room, B["n"], NO_BOXES, 0)
    bctx.rast_set_route(DENSE)
    try:
        ref = bctx.rast_render_buffers(tris, n, p, light)
    finally:
        bctx.rast_set_route(-1)
    bctx.rast_set_scene(room, B["n"], NO_BOXES, 0)
    got = bctx.rast_draw_buffers(p)                     # the automatic route
    info = bctx.rast_scratch_info()
    assert info["route"] == COMPACT and info["tris"] == n > 4096
    src = ro.input_of_clip(p, room, B["n"], NO_BOXES, 0)
    ref["tri"] = np.where(ref["clip"] >= 0, src[np.maximum(ref["clip"], 0)], NONE).astype(np.int32)
    _same(got, ref, ALL, "6000-triangle room")
    ora = oracle.rast_draw(sc.oracle_params(p), scene=(room, B["n"], NO_BOXES, 0), buffers=True)
    _same(got, ora, ("screen", "low", "high", "argb", "depth", "shadow"), "6000-triangle room against the oracle")
    assert (got["clip"] >= 0).any()


# ---- 6. plumbing ----------------------------------------------------------------------------------
def test_each_plane_alone(bctx):
    W, H, camera = 67, 45, "in_short_box"
    p, _ = case_params(W, H, camera)
    bctx.rast_set_scene(*cgamd.rast_scene())
    for route in (DENSE, COMPACT):
        full = _on_route(bctx, route, lambda: bctx.rast_draw_buffers(p))
        for name in ALL:
            one = _on_route(bctx, route, lambda: bctx.rast_draw_buffers(p, (name,)))
            assert list(one) == [name]
            _same(one, full, (name,), f"{name} alone, route {route}")


def test_device_form_on_a_second_stream(bctx):
    import torch
    W, H, camera = 96, 64, "yawed"
    p, _ = case_params(W, H, camera)
    bctx.rast_set_scene(*cgamd.rast_scene())
    full = bctx.rast_draw_buffers(p)
    dev = torch.device("cuda:0")
    npx = W * H
    shapes = {"argb": (torch.int32, 1), "depth": (torch.float32, 1), "shadow": (torch.int32, 1),
              "screen": (torch.float32, 3), "low": (torch.float32, 3), "high": (torch.float32, 3),
              "clip": (torch.int32, 1), "tri": (torch.int32, 1), "pos": (torch.float32, 4)}
    planes = {k: torch.full((npx, c) if c > 1 else (npx,), 77, dtype=dt, device=dev) for k, (dt, c) in shapes.items()}
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    bctx.rast_draw_buffers_device(p, stream=st.cuda_stream, **{k: v.data_ptr() for k, v in planes.items()})
    st.synchronize()
    got = {k: v.cpu().numpy() for k, v in planes.items()}
    got["argb"] = got["argb"].view(np.uint32)
    _same(got, full, ALL, "device form")
    # the render form over a device list: tri = clip
    tris, n, light = cgamd.rast_prepare(p)
    d_tris = torch.frombuffer(bytearray(C.string_at(tris, n * 84)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    bctx.rast_render_buffers_device(d_tris.data_ptr(), n, p, light, stream=st.cuda_stream,
                                    clip=planes["clip"].data_ptr(), tri=planes["tri"].data_ptr(),
                                    screen=planes["screen"].data_ptr())
    st.synchronize()
    assert np.array_equal(planes["clip"].cpu().numpy(), full["clip"])
    assert np.array_equal(planes["tri"].cpu().numpy(), full["clip"])
    assert np.array_equal(planes["screen"].cpu().numpy().view(np.uint32), full["screen"].view(np.uint32))


def test_refusals_and_pick(bctx):
    W, H, camera = 96, 64, "unrotated"
    p, _ = case_params(W, H, camera)
    lib = bctx.lib
    none = cgamd.RastBuffers()
    with cgamd.Context(0) as fresh:                       # no scene yet
        b, _ = cgamd.rast_buffers_planes(p, ("clip",))
        assert lib.cg_rast_draw_buffers(fresh.h, C.byref(p), C.byref(b), None) == cgamd.CG_E_NOSCENE
        hit = C.c_int()
        assert lib.cg_rast_pick(fresh.h, C.byref(p), 1, 1, None, None, None, C.byref(hit)) == cgamd.CG_E_NOSCENE
    bctx.rast_set_scene(*cgamd.rast_scene())
    tris, n, light = cgamd.rast_prepare(p)
    assert lib.cg_rast_draw_buffers(bctx.h, C.byref(p), C.byref(none), None) == cgamd.CG_E_INVALID
    assert lib.cg_rast_draw_buffers_device(bctx.h, C.byref(p), C.byref(none), None) == cgamd.CG_E_INVALID
    assert lib.cg_rast_render_buffers(bctx.h, tris, n, C.byref(p), light, C.byref(none), None) == cgamd.CG_E_INVALID
    assert lib.cg_rast_render_buffers_device(bctx.h, None, 0, C.byref(p), light, C.byref(none), None) == cgamd.CG_E_INVALID
    hit = C.c_int()
    for x, y in ((-1, 0), (0, -1), (W, 0), (0, H)):
        assert lib.cg_rast_pick(bctx.h, C.byref(p), x, y, None, None, None, C.byref(hit)) == cgamd.CG_E_INVALID
    for route in (DENSE, COMPACT):
        full = _on_route(bctx, route, lambda: bctx.rast_draw_buffers(p, ("clip", "tri", "pos")))
        background = np.flatnonzero(full["clip"] == NONE)
        assert background.size
        rng = np.random.default_rng(50)
        pix = [(int(x), int(y)) for x, y in zip(rng.integers(0, W, 50), rng.integers(0, H, 50))]
        pix += [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (int(background[0] % W), int(background[0] // W))]
        hits = 0
        for x, y in pix:
            tri, clip, pos, hit = _on_route(bctx, route, lambda: bctx.rast_pick(p, x, y))
            o = y * W + x
            assert (tri, clip, hit) == (full["tri"][o], full["clip"][o], full["clip"][o] >= 0), (x, y)
            assert np.array_equal(pos.view(np.uint32), full["pos"][o].view(np.uint32)), (x, y)
            hits += hit
        assert 0 < hits < len(pix)
    # a pick in a colour mode names the same owner without drawing from the rand() stream
    p1, _ = case_params(W, H, camera, 0.2, 1, 0)
    x, y = W // 2, H // 2
    assert bctx.rast_pick(p1, x, y)[:2] == (full["tri"][y * W + x], full["clip"][y * W + x])
    # a plain Draw after the buffers calls is still the oracle's
    ref = _oracle_frame(W, H, camera)
    a, d, s, _ = bctx.rast_draw(p)
    _same({"argb": a, "depth": d, "shadow": s}, ref, ("argb", "depth", "shadow"), "rast_draw after buffers calls")
