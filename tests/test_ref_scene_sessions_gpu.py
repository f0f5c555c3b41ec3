"""GPU: the kernels on caller-supplied scenes, at states the reference programs themselves reached
on those scenes.

tests/golden/ref_scene_sessions.json holds, per frame of 18 scripted sessions of the reference's
raytracer and rasteriser on the scenes of tests/ref_scene_cases.py, the globals the program had and
the SHA-256 of every plane it drew (tests/golden/make_ref_scene_sessions.py).  The scenes are
regenerated here and checked against the recorded scene hash; every comparison is bit-exact
against the recorded plane hash.  On a mismatch the oracle renders the frame and the message gives
the count and the first differing pixels.

Nothing here reads the reference tree or oracle/_ref/."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import make_ref_sessions as mrs
import oracle
import rast_owner_ref as ro
import ref_scene_cases as cases
import ref_scene_states as rss

pytestmark = pytest.mark.gpu

RT_W, RT_H = mrs.SIZES["raytracer"]
RA_W, RA_H = mrs.SIZES["rasteriser"]
DENSE, COMPACT = cgamd.RAST_ROUTE_DENSE, cgamd.RAST_ROUTE_COMPACT
NONE = cgamd.RAST_OWNER_NONE


@pytest.fixture(scope="module")
def sctx():
    """A context of this module's own: scenes and routes never reach the shared one."""
    c = cgamd.Context(0)
    yield c
    c.close()


# ---- raytracer ---------------------------------------------------------------------------------

def _rt_cam(st):
    R = (C.c_float * 16)(*[float(x) for x in st["R"]])
    return cgamd.rt_camera(RT_W, RT_H, float(st["focal"][0]), rss.t4(st["cam"]), R, 0.5)


def _rt_lights(st):
    arr = (cgamd.Light * 1)()
    arr[0].position = cgamd.Vec4(*rss.t4(st["light"]))
    arr[0].colour = cgamd.Vec3(*rss.LIGHT_COLOUR)
    return arr


def _rt_check(name, k, got, what):
    want = rss.SESSIONS[name]["frames"][k]["argb"]
    if mrs.sha(got) != want:
        ref = oracle.rt_draw(rss.oracle_rt_params(rss.states(name)[k]), threads=8, scene=cases.rt_oracle_scene(name))
        note = "" if mrs.sha(ref) == want else " (the oracle differs from the reference here too)"
        pytest.fail(rss.diff_report(f"{name} frame {k} {what}", got, ref) + note)


@pytest.fixture
def rt_scene(sctx, request):
    name = request.param
    rss.check_scene(name)
    tris, n, sph, n_sph = cases.rt_library_scene(name)      # the C entry: Context.rt_set_scene takes one sphere
    sctx._check(sctx.lib.cg_rt_set_scene(sctx.h, tris, n, sph, n_sph), "cg_rt_set_scene")
    return sctx, name


@pytest.mark.parametrize("rt_scene", rss.RT, indirect=True)
def test_rt_render_at_recorded_states(rt_scene):
    ctx, name = rt_scene
    for k, st in enumerate(rss.states(name)):
        argb, _ = ctx.rt_render(_rt_cam(st), _rt_lights(st))
        _rt_check(name, k, argb, "rt_render")


@pytest.mark.parametrize("name", rss.RT)
def test_rt_route_is_the_one_the_case_is_for(name):
    """300 triangles take the large-scene kernels, 64 or fewer the small-scene ones; a frame with
    any yaw -- the tiny one after 'm' 'n' included -- the yaw form."""
    plain, yawed = cases.CASES[name]["routes"]
    n_tris, n_sph = (len(a) for a in cases.scene(name))
    assert (n_tris > 64) == plain.startswith("big_")
    seen = set()
    for k, st in enumerate(rss.states(name)):
        route = cgamd.rt_route(_rt_cam(st), n_tris, n_sph, 1)
        assert route == (yawed if st["yaw"][0] != 0 else plain), f"{name} frame {k}"
        seen.add(route)
    assert seen == {plain, yawed}, name


def _light_runs(sts):
    """Runs [a, b) of consecutive frames with the same light."""
    runs, a = [], 0
    for k in range(1, len(sts) + 1):
        if k == len(sts) or sts[k]["light"].tobytes() != sts[a]["light"].tobytes():
            runs.append((a, k))
            a = k
    return runs


@pytest.mark.parametrize("rt_scene", rss.RT, indirect=True)
def test_rt_frames_device_whole_session(rt_scene):
    """cg_rt_render_frames_device takes one light set for its frames: one call per session, or
    one per run of frames between the session's light moves."""
    import torch
    ctx, name = rt_scene
    sts = rss.states(name)
    npx = RT_W * RT_H
    stream = torch.cuda.Stream()
    for a, b in _light_runs(sts):
        buf = torch.zeros((b - a) * npx, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.rt_render_frames_device([_rt_cam(st) for st in sts[a:b]], buf.data_ptr(), stream=stream.cuda_stream,
                                    lights=_rt_lights(sts[a]))
        stream.synchronize()
        got = buf.cpu().numpy().view(np.uint32).reshape(b - a, npx)
        for k in range(a, b):
            _rt_check(name, k, got[k - a], "rt_render_frames_device")


@pytest.mark.parametrize("rt_scene", rss.RT, indirect=True)
def test_rt_sequence_device_whole_session(rt_scene):
    """One cg_rt_render_sequence_device call: per-frame lights, cameras, yaws and focal lengths."""
    import torch
    ctx, name = rt_scene
    sts = rss.states(name)
    npx = RT_W * RT_H
    buf = torch.zeros(len(sts) * npx, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.rt_render_sequence_device([_rt_cam(st) for st in sts], [_rt_lights(st) for st in sts], buf.data_ptr(),
                                  None, stream.cuda_stream)
    stream.synchronize()
    got = buf.cpu().numpy().view(np.uint32).reshape(len(sts), npx)
    for k in range(len(sts)):
        _rt_check(name, k, got[k], "rt_render_sequence_device")


# ---- rasteriser --------------------------------------------------------------------------------

def _rast_params(st, rand_offset=0):
    return cgamd.rast_params(RA_W, RA_H, float(st["focal"][0]), rss.t4(st["cam"]), [float(x) for x in st["R"]],
                             rss.t4(st["light"]), float(st["indirect"][0]), st["mode"], rand_offset,
                             float(st["yaw"][0]))


def _rast_check(name, k, planes, what):
    """planes: (argb, depth, shadow) of frame k"""
    fr = rss.SESSIONS[name]["frames"][k]
    names = ("argb", "depth", "shadow")
    bad = [nm for nm, a in zip(names, planes) if mrs.sha(a) != fr[nm]]
    if bad:
        *_, (_, a, d, s, _, off) = rss.oracle_rast_session(name, upto=k + 1)
        ref = dict(zip(names, (a, d, s)))
        got = dict(zip(names, planes))
        pytest.fail("; ".join(rss.diff_report(f"{name} frame {k} {what} {nm} (rand() index {off})", got[nm], ref[nm])
                              for nm in bad))


@pytest.fixture
def rast_scene(sctx, request):
    name = request.param
    rss.check_scene(name)
    sctx.rast_set_scene(*cases.rast_library_scene(name))
    yield sctx, name
    sctx.rast_set_route(-1)
    sctx.rast_set_route_limit(0)


DENSE_COLOUR_LIST = 20480      # cg_render.h: a colour mode 1-2 frame with a longer list takes the compact route


def _automatic_route(name, mode):
    n_room, n_boxes = (len(a) for a in cases.scene(name))
    cap = 32 * (n_room + 7 * n_boxes)         # the list capacity: 32 clipped triangles an input
    return COMPACT if mode and cap > DENSE_COLOUR_LIST else cgamd.rast_route(cap)


def _rast_per_frame(ctx, name, compact):
    """rast_draw frame by frame, the rand() index chained on the host as host/rasteriser.cpp chains
    it.  compact: the forced compact route in colour mode 0, the route limit of 1 in modes 1-2
    (a forced route refuses them); else the route must be the automatic one."""
    off = 0
    for k, st in enumerate(rss.states(name)):
        if compact:
            ctx.rast_set_route(COMPACT if st["mode"] == 0 else -1)
            ctx.rast_set_route_limit(1 if st["mode"] else 0)
        a, d, s, stats = ctx.rast_draw(_rast_params(st, off))
        route = ctx.rast_scratch_info()["route"]
        if compact and (st["mode"] == 0 or stats.n_tris > 0):
            assert route == COMPACT, f"{name} frame {k}"
        if not compact and name not in cases.EMPTY:
            assert route == _automatic_route(name, st["mode"]), f"{name} frame {k}"
        _rast_check(name, k, (a, d, s), "rast_draw" + (" (compact route)" if compact else ""))
        if st["mode"]:
            off += 3 * int(stats.n_shaded)


@pytest.mark.parametrize("rast_scene", rss.RAST, indirect=True)
def test_rast_draw_automatic_route(rast_scene):
    """The route the library chooses itself: dense while the scene's list capacity allows it --
    131072 in colour mode 0, 20480 in modes 1-2 (rast_mesh3000's 109440 lies between: its mode 1-2
    frames failed on the dense route with "colour count launch: invalid argument" before the
    automatic choice took the colour mode into account)."""
    ctx, name = rast_scene
    _rast_per_frame(ctx, name, compact=False)
    assert {_automatic_route("rast_mesh3000", m) for m in (0, 1, 2)} == {DENSE, COMPACT}


@pytest.mark.parametrize("rast_scene", rss.RAST, indirect=True)
def test_rast_draw_compact_route(rast_scene):
    ctx, name = rast_scene
    _rast_per_frame(ctx, name, compact=True)


@pytest.mark.parametrize("rast_scene", rss.RAST, indirect=True)
def test_rast_draw_sequence_device(rast_scene):
    """The whole session in one cg_rast_draw_sequence_device call: the rand() index chained on
    the device."""
    import torch
    ctx, name = rast_scene
    sts = rss.states(name)
    n, npx = len(sts), RA_W * RA_H
    dA = torch.zeros(n * npx, dtype=torch.int32, device="cuda")
    dD = torch.zeros(n * npx, dtype=torch.float32, device="cuda")
    dS = torch.zeros(n * npx, dtype=torch.int32, device="cuda")
    dI = torch.full((3 * (n + 1),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.rast_draw_sequence_device([_rast_params(st) for st in sts], dA.data_ptr(), dD.data_ptr(), dS.data_ptr(), 0,
                                  dI.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    info = dI.cpu().numpy().view(cgamd.RAST_SEQ_DTYPE)
    assert not info["status"].any(), f"{name}: {info['status']}"
    A, D, S = dA.cpu().numpy().view(np.uint32), dD.cpu().numpy(), dS.cpu().numpy()
    for k in range(n):
        o = slice(k * npx, (k + 1) * npx)
        _rast_check(name, k, (A[o], D[o], S[o]), "rast_draw_sequence_device")


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


def _buffers_frame(name):
    """The session's first yawed frame in colour mode 0 (low / high are written there), else frame 0."""
    sts = rss.states(name)
    return next((k for k, st in enumerate(sts) if st["mode"] == 0 and st["yaw"][0] != 0), 0)


@pytest.mark.parametrize("rast_scene", rss.RAST, indirect=True)
def test_rast_buffers_and_owners_one_frame(rast_scene):
    """cg_rast_draw_buffers on both routes: the float shade buffers against the oracle on the
    mesh, the owner planes against the ordered z-buffer restated over the oracle's primitives
    (rast_owner_ref; shadow volumes never own, so they are skipped there)."""
    ctx, name = rast_scene
    k = _buffers_frame(name)
    st = rss.states(name)[k]
    assert st["mode"] == 0
    p, po = _rast_params(st), rss.oracle_rast_params(st, 0)
    ref = oracle.rast_draw(po, scene=cases.rast_oracle_scene(name), buffers=True)
    assert mrs.sha(ref["argb"]) == rss.SESSIONS[name]["frames"][k]["argb"]          # the reference's own frame
    tris, n, _ = oracle.rast_geometry(po, scene=cases.rast_oracle_scene(name))
    depth, _, clip, pos = ro.owner_planes(po, tris, n, RA_W, RA_H, shadow_marks=False)
    src = ro.input_of_clip(p, *cases.rast_library_scene(name))
    assert src.size == n
    tri = np.where(clip >= 0, src[np.maximum(clip, 0)], NONE).astype(np.int32) if n else np.full_like(clip, NONE)
    own = {"clip": clip, "pos": pos, "tri": tri}
    assert np.array_equal(depth.view(np.uint32), ref["depth"].view(np.uint32))       # the owner rule's z-buffer
    for route in ("automatic", "compact"):
        ctx.rast_set_route(COMPACT if route == "compact" else -1)
        got = ctx.rast_draw_buffers(p)
        if route == "compact":
            assert ctx.rast_scratch_info()["route"] == COMPACT
        what = f"{name} frame {k} {route} route"
        _same(got, ref, ("screen", "low", "high", "argb", "depth", "shadow"), what)
        _same(got, own, ("clip", "pos", "tri"), what)
    if name not in cases.EMPTY:
        assert (got["clip"] >= 0).any()
