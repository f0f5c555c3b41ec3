"""GPU: the kernels at the states the reference programs themselves reach.

tests/golden/ref_sessions.json holds, per frame of 18 scripted sessions of the reference's own
raytracer, rasteriser and starfield, the globals the program had and the SHA-256 of every plane it
drew (tests/golden/make_ref_sessions.py).  Each frame's library arguments are those recorded
globals, and every comparison is bit-exact against the recorded hash: raytracer ARGB; rasteriser
ARGB, depthBuffer and shadowBuffer; starfield ARGB.  On a mismatch the oracle renders the frame and
the message gives the count and the first differing pixels.

Nothing here reads the reference tree or oracle/_ref/.  Frame sizes are the reference's #defines
(320 x 256, 900 x 720); long sessions go through the sequence calls in pieces of at most 32 frames
so that no call holds more than a few hundred MB."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cgamd
import make_golden as mg
import make_ref_sessions as mrs
import ref_session_states as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "computer-graphics_amd", "_build")
PIECE = 32                       # frames per sequence call
RT_W, RT_H = mrs.SIZES["raytracer"]
RA_W, RA_H = mrs.SIZES["rasteriser"]
ST_W, ST_H = mrs.SIZES["starfield"]


def _R(st):
    return (C.c_float * 16)(*[float(x) for x in st["R"]])


# ---- raytracer ---------------------------------------------------------------------------------

def _rt_cam(st):
    return cgamd.rt_camera(RT_W, RT_H, float(st["focal"][0]), rs.t4(st["cam"]), _R(st), 0.5)


def _rt_lights(st):
    arr = (cgamd.Light * 1)()
    arr[0].position = cgamd.Vec4(*rs.t4(st["light"]))
    arr[0].colour = cgamd.Vec3(*rs.LIGHT_COLOUR)
    return arr


def _rt_check(name, k, got, what):
    want = rs.SESSIONS[name]["frames"][k]["argb"]
    if mrs.sha(got) != want:
        import oracle
        ref = oracle.rt_draw(rs.oracle_rt_params(rs.states(name)[k]), threads=8)
        note = "" if mrs.sha(ref) == want else " (the oracle differs from the reference here too)"
        pytest.fail(rs.diff_report(f"{name} frame {k} {what}", got, ref) + note)


@pytest.fixture
def rt_ctx(ctx):
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    return ctx


@pytest.mark.parametrize("name", rs.RT)
def test_rt_render_at_recorded_states(rt_ctx, name):
    for k, st in enumerate(rs.states(name)):
        argb, _ = rt_ctx.rt_render(_rt_cam(st), _rt_lights(st))
        _rt_check(name, k, argb, "rt_render")


@pytest.mark.parametrize("name", rs.RT)
def test_rt_sequence_device_whole_session(rt_ctx, name):
    """One cg_rt_render_sequence_device call: per-frame lights, cameras, yaws and focal lengths."""
    import torch
    sts = rs.states(name)
    npx = RT_W * RT_H
    buf = torch.zeros(len(sts) * npx, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rt_ctx.rt_render_sequence_device([_rt_cam(st) for st in sts], [_rt_lights(st) for st in sts], buf.data_ptr(),
                                     None, stream.cuda_stream)
    stream.synchronize()
    got = buf.cpu().numpy().view(np.uint32).reshape(len(sts), npx)
    for k in range(len(sts)):
        _rt_check(name, k, got[k], "rt_render_sequence_device")


def test_rt_tiny_yaw_frames_take_the_yaw_lattice_route(rt_ctx):
    """After 'm' then 'n' R has cos = 1 and sin = -5.37e-9: not the identity, so the frame takes
    lattice_yaw, never the unrotated lattice route -- and is exact there (the tests above)."""
    n_tris, seen = cgamd.rt_scene()[1], 0
    for name in rs.RT:
        for st in rs.states(name):
            route = cgamd.rt_route(_rt_cam(st), n_tris, 1, 1)
            if st["yaw"][0] == rs.TINY_YAW:
                seen += 1
                assert route == "lattice_yaw", name
            elif st["yaw"][0] == 0:
                assert route == "lattice", name
    assert seen == 11


def _app(app, args, out):
    r = subprocess.run([os.path.join(BUILD, app), *args, "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return mg.screenshot_argb(out)


@pytest.mark.parametrize("name,batch", [("rt_turn_back_twice", False), ("rt_mixed", True)])
def test_raytracer_app_final_frame(tmp_path, name, batch):
    sp = rs.SESSIONS[name]
    got = _app("raytracer", ["--keys", sp["keys"]] + (["--batch"] if batch else []), str(tmp_path / "rt.bmp"))
    _rt_check(name, len(sp["keys"]) - 1, got, "raytracer --keys" + (" --batch" if batch else ""))


# ---- rasteriser --------------------------------------------------------------------------------

def _rast_params(st, rand_offset=0):
    return cgamd.rast_params(RA_W, RA_H, float(st["focal"][0]), rs.t4(st["cam"]), [float(x) for x in st["R"]],
                             rs.t4(st["light"]), float(st["indirect"][0]), st["mode"], rand_offset,
                             float(st["yaw"][0]))


def _rast_check(name, k, planes, what):
    """planes: (argb, depth, shadow) of frame k"""
    fr = rs.SESSIONS[name]["frames"][k]
    names = ("argb", "depth", "shadow")
    bad = [nm for nm, a in zip(names, planes) if mrs.sha(a) != fr[nm]]
    if bad:
        *_, (_, a, d, s, _, off) = rs.oracle_rast_session(name, upto=k + 1)
        ref = dict(zip(names, (a, d, s)))
        got = dict(zip(names, planes))
        pytest.fail("; ".join(rs.diff_report(f"{name} frame {k} {what} {nm} (rand() index {off})", got[nm], ref[nm])
                              for nm in bad))


@contextlib.contextmanager
def _rast_scene(ctx, name):
    """The session's scene (TestModelH.h's setting / settingBoxes) and, when textured, the
    reference's JPEG maps decoded on the GPU."""
    sp = rs.SESSIONS[name]
    tex = mrs.textured(sp)
    try:
        if tex:
            ctx.rast_set_textures(ctx.load_textures_jpeg(mg.TEXTURE_DIR))
        ctx.rast_set_scene(*cgamd.rast_scene(sp.get("setting", 0), sp.get("setting_boxes", 0)))
        yield
    finally:
        if tex:
            ctx.rast_set_textures(None)
        ctx.rast_set_scene()


def _rast_per_frame(ctx, name, compact=False):
    """rast_draw frame by frame, the rand() index and the indirect term chained on the host as
    host/rasteriser.cpp chains them; the chained indirect must be the reference's own."""
    keys, off, ind = rs.SESSIONS[name]["keys"], 0, np.float32(0.15)
    for k, st in enumerate(rs.states(name)):
        if keys[k] in "12":
            ind = np.float32(ind + (np.float32(0.005) if keys[k] == "2" else -np.float32(0.005)))
        assert ind.view(np.uint32) == st["indirect"].view(np.uint32)[0], f"{name} frame {k}: indirect chain"
        a, d, s, stats = ctx.rast_draw(_rast_params(st, off))
        if compact and stats.n_tris > 0:
            assert ctx.rast_scratch_info()["route"] == cgamd.RAST_ROUTE_COMPACT, f"{name} frame {k}"
        _rast_check(name, k, (a, d, s), "rast_draw" + (" (compact route)" if compact else ""))
        if st["mode"]:
            off += 3 * int(stats.n_shaded)
        elif stats.n_tris > 0:
            ind = np.float32(0.2)


@pytest.mark.parametrize("name", rs.RAST)
def test_rast_draw_frame_by_frame(ctx, name):
    with _rast_scene(ctx, name):
        _rast_per_frame(ctx, name)


@pytest.mark.parametrize("name", rs.RAST_PLAIN)
def test_rast_draw_compact_route(ctx, name):
    """The route limit lowered to 1: every frame with triangles takes the compact span and
    row-record lists, colour modes 1-2 included -- against frames the reference made."""
    with _rast_scene(ctx, name):
        try:
            ctx.rast_set_route_limit(1)
            _rast_per_frame(ctx, name, compact=True)
        finally:
            ctx.rast_set_route_limit(0)


def _pieces(n):
    return [(a, min(a + PIECE, n)) for a in range(0, n, PIECE)]


@pytest.mark.parametrize("name", rs.RAST)
def test_rast_draw_sequence_chunk_7(ctx, name):
    """cg_rast_draw_sequence into host memory with all three planes, chunk 7: the 40-frame
    sessions cross chunk borders inside a call; a later call starts at the closing rand() index
    the earlier one reported."""
    sts = rs.states(name)
    npx = RA_W * RA_H
    with _rast_scene(ctx, name):
        off = 0
        for a, b in _pieces(len(sts)):
            ps = [_rast_params(st) for st in sts[a:b]]
            ps[0].rand_offset = off
            A, D, S, info, _ = ctx.rast_draw_sequence(ps, want_depth=True, want_shadow=True, chunk=7)
            assert not info["status"].any(), f"{name} frames {a}-{b}: {info['status']}"
            off = int(info["rand_offset"][-1])
            for k in range(a, b):
                o = slice((k - a) * npx, (k - a + 1) * npx)
                _rast_check(name, k, (A[o], D[o], S[o]), "rast_draw_sequence")


@pytest.mark.parametrize("name", rs.RAST)
def test_rast_draw_sequence_device(ctx, name):
    import torch
    sts = rs.states(name)
    npx = RA_W * RA_H
    info_dtype = cgamd.RAST_SEQ_DTYPE
    with _rast_scene(ctx, name):
        off = 0
        for a, b in _pieces(len(sts)):
            n = b - a
            ps = [_rast_params(st) for st in sts[a:b]]
            ps[0].rand_offset = off
            dA = torch.zeros(n * npx, dtype=torch.int32, device="cuda")
            dD = torch.zeros(n * npx, dtype=torch.float32, device="cuda")
            dS = torch.zeros(n * npx, dtype=torch.int32, device="cuda")
            dI = torch.full((3 * (n + 1),), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.rast_draw_sequence_device(ps, dA.data_ptr(), dD.data_ptr(), dS.data_ptr(), 0, dI.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            info = dI.cpu().numpy().view(info_dtype)
            assert not info["status"].any(), f"{name} frames {a}-{b}: {info['status']}"
            off = int(info["rand_offset"][-1])
            A, D, S = dA.cpu().numpy().view(np.uint32), dD.cpu().numpy(), dS.cpu().numpy()
            for k in range(a, b):
                o = slice((k - a) * npx, (k - a + 1) * npx)
                _rast_check(name, k, (A[o], D[o], S[o]), "rast_draw_sequence_device")


@pytest.mark.parametrize("name,batch", [("rast_modes", False), ("rast_modes", True),
                                        ("rast_tex_2_3", False), ("rast_tex_2_3", True)])
def test_rasteriser_app_final_frame(tmp_path, name, batch):
    sp = rs.SESSIONS[name]
    args = ["--keys", sp["keys"]]
    if mrs.textured(sp):
        args += ["--setting", str(sp["setting"]), "--setting-boxes", str(sp["setting_boxes"]),
                 "--textures", mg.TEXTURE_DIR]
    got = _app("rasteriser", args + (["--batch"] if batch else []), str(tmp_path / "rast.bmp"))
    k = len(sp["keys"]) - 1
    if mrs.sha(got) != sp["frames"][k]["argb"]:
        *_, (_, ref, _, _, _, off) = rs.oracle_rast_session(name, upto=k + 1)
        pytest.fail(rs.diff_report(f"{name} rasteriser --keys{' --batch' if batch else ''} (rand() index {off})",
                                   got, ref))


# ---- starfield ---------------------------------------------------------------------------------

def _star_check(name, frames, what):
    """frames: (n, W * H) uint32"""
    sp = rs.SESSIONS[name]
    bad = [k for k in range(len(frames)) if mrs.sha(frames[k]) != sp["frames"][k]["argb"]]
    if bad:
        import oracle
        stars = oracle.starfield_init(mrs.N_STARS)
        for k in range(bad[0]):
            oracle.starfield_update(stars, float(sp["dts"][k]))
        ref = oracle.starfield_draw(stars, ST_W, ST_H)
        pytest.fail(f"{name} {what}: frames {bad} differ; " + rs.diff_report(f"frame {bad[0]}", frames[bad[0]], ref))


@pytest.mark.parametrize("name", rs.STAR)
def test_starfield_draw_and_update_frame_by_frame(ctx, name):
    sp = rs.SESSIONS[name]
    stars = cgamd.starfield_init(mrs.N_STARS)
    frames = []
    for k in range(len(sp["frames"])):
        assert mrs.sha(stars) == sp["frames"][k]["state"], f"{name} frame {k}: the stars differ from the reference's"
        frames.append(ctx.starfield_draw(stars, ST_W, ST_H))
        cgamd.starfield_update(stars, float(sp["dts"][k]))
    _star_check(name, np.stack(frames), "starfield_draw + starfield_update")


@pytest.mark.parametrize("name", rs.STAR)
def test_starfield_run_device(ctx, name):
    import torch
    sp = rs.SESSIONS[name]
    n, npx = len(sp["frames"]), ST_W * ST_H
    ctx.starfield_set(cgamd.starfield_init(mrs.N_STARS))
    buf = torch.zeros(n * npx, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.starfield_run_device(sp["dts"], n, ST_W, ST_H, buf.data_ptr())
    torch.cuda.synchronize()
    _star_check(name, buf.cpu().numpy().view(np.uint32).reshape(n, npx), "starfield_run_device")


@pytest.mark.parametrize("name", rs.STAR)
def test_starfield_run(ctx, name):
    sp = rs.SESSIONS[name]
    n, npx = len(sp["frames"]), ST_W * ST_H
    ctx.starfield_set(cgamd.starfield_init(mrs.N_STARS))
    out, _ = ctx.starfield_run(sp["dts"], n, ST_W, ST_H)
    _star_check(name, out.reshape(n, npx), "starfield_run")


@pytest.mark.parametrize("name", rs.STAR)
@pytest.mark.parametrize("batch", [False, True])
def test_starfield_app_final_frame(tmp_path, name, batch):
    """The app takes the session's own frame times (--dts): its screenshot is the last frame."""
    sp = rs.SESSIONS[name]
    args = ["--dts", ",".join(str(d) for d in sp["dts"])] + (["--batch"] if batch else [])
    got = _app("starfield", args, str(tmp_path / "star.bmp"))
    assert mrs.sha(got) == sp["frames"][-1]["argb"], f"{name} starfield --dts{' --batch' if batch else ''}"
