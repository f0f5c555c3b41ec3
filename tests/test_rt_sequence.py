"""CPU: the raytracer's frame-sequence C-ABI (cg_rt_render_sequence_device, cg_rt_render_sequence,
cg_rt_sequence_runs): declared, bound and exported with the documented argument types; argument
checks; how a sequence splits into runs (host logic only, no GPU); and the teeth of the GPU tests'
inputs -- consecutive states of their key scripts that differ by a light key render differently in
the oracle, so a sequence frame rendered with a stale light cannot pass."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cgamd
import rt_seq_states as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cg_rt_render_sequence_device", "cg_rt_render_sequence", "cg_rt_sequence_runs")
P = C.c_void_p


def _decl(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cg_render.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m, f"{name} not declared"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_the_documented_arguments():
    assert _decl("cg_rt_render_sequence_device") == [
        "cg_ctx *ctx", "const cg_light *lights", "int n_lights", "const cg_rt_camera *cams", "int n_frames",
        "const cg_rt_shard *shard", "void *d_out", "size_t frame_stride", "int pix_format", "void *stream"]
    assert _decl("cg_rt_render_sequence") == [
        "cg_ctx *ctx", "const cg_light *lights", "int n_lights", "const cg_rt_camera *cams", "int n_frames",
        "uint32_t *argb", "size_t frame_stride", "int chunk", "cg_stats *stats"]
    assert _decl("cg_rt_sequence_runs") == [
        "const cg_rt_camera *cams", "int n_frames", "int n_tris", "int n_spheres", "int n_lights",
        "const cg_rt_shard *shard", "int *run_start", "int *run_route", "int cap"]


def test_binding_matches_the_header():
    LP, CP, SP, IP = C.POINTER(cgamd.Light), C.POINTER(cgamd.RtCamera), C.POINTER(cgamd.RtShard), C.POINTER(C.c_int)
    sigs = cgamd._SIGS
    assert sigs["cg_rt_render_sequence_device"] == (C.c_int, [P, LP, C.c_int, CP, C.c_int, SP, P, C.c_size_t, C.c_int, P])
    assert sigs["cg_rt_render_sequence"] == (C.c_int, [P, LP, C.c_int, CP, C.c_int, P, C.c_size_t, C.c_int,
                                                       C.POINTER(cgamd.Stats)])
    assert sigs["cg_rt_sequence_runs"] == (C.c_int, [CP, C.c_int, C.c_int, C.c_int, C.c_int, SP, IP, IP, C.c_int])
    # the sequence entries take what the common-lights entries take
    assert sigs["cg_rt_render_sequence_device"] == sigs["cg_rt_render_frames_device"]
    assert sigs["cg_rt_render_sequence"] == sigs["cg_rt_render_frames"]
    for meth in ("rt_render_sequence_device", "rt_render_sequence"):
        assert callable(getattr(cgamd.Context, meth))
    assert callable(cgamd.rt_sequence_runs)


def test_library_exports_the_symbols():
    lib = cgamd.load()
    for name in NAMES:
        assert hasattr(lib, name), name


def _cams(n, W=1920, H=1080, f=1080.0):
    return [cgamd.rt_camera(W, H, f) for _ in range(n)]


def test_bad_arguments_are_invalid():
    """No device is touched.  Without a GPU there is no context, and a NULL context is itself
    CG_E_INVALID: of the render entries' four cases only `n_lights > 4096` and NULL lights are
    decided before the context is looked at, so here the `n_frames < 0` and two-sizes calls show
    no more than that nothing is dereferenced or launched; with a context all four are checked for
    their own reason on the GPU (tests/test_rt_sequence_gpu.py: test_bad_arguments_with_a_context).
    cg_rt_sequence_runs needs no context: its checks are real here."""
    lib = cgamd.load()
    lights = S.light_array([(S.LIGHT0, S.COLOUR0)] * 2)
    two = (cgamd.RtCamera * 2)(*_cams(2))
    sizes = (cgamd.RtCamera * 2)(cgamd.rt_camera(64, 60, 60.0), cgamd.rt_camera(64, 48, 60.0))
    out = (C.c_uint32 * 16)()
    dev = lib.cg_rt_render_sequence_device
    host = lib.cg_rt_render_sequence
    for fn, tail in ((dev, (None, C.cast(out, P), 0, 0, None)), (host, (C.cast(out, P), 0, 0, None))):
        assert fn(None, lights, 1, two, -1, *tail) == cgamd.CG_E_INVALID          # n_frames < 0
        assert fn(None, None, 1, two, 2, *tail) == cgamd.CG_E_INVALID             # no lights, n_lights > 0
        assert fn(None, lights, 1, sizes, 2, *tail) == cgamd.CG_E_INVALID         # frames of two sizes
        assert fn(None, lights, 4097, two, 2, *tail) == cgamd.CG_E_INVALID        # n_lights > 4096
    start, route = (C.c_int * 9)(), (C.c_int * 8)()
    runs = lib.cg_rt_sequence_runs
    assert runs(two, -1, 28, 1, 1, None, start, route, 8) == cgamd.CG_E_INVALID
    assert runs(sizes, 2, 28, 1, 1, None, start, route, 8) == cgamd.CG_E_INVALID
    assert runs(two, 2, 28, 1, 4097, None, start, route, 8) == cgamd.CG_E_INVALID
    assert runs(two, 2, -1, 1, 1, None, start, route, 8) == cgamd.CG_E_INVALID
    assert runs(None, 2, 28, 1, 1, None, start, route, 8) == cgamd.CG_E_INVALID
    assert runs(two, 2, 28, 1, 1, None, None, None, 8) == cgamd.CG_E_INVALID
    assert runs(two, 2, 28, 1, 1, None, start, route, 8) == 1
    assert runs(two, 0, 28, 1, 1, None, start, route, 8) == 0
    with pytest.raises(ValueError):
        cgamd.sequence_lights([[1, 2], [1]])


def _moving(n):
    """n Cornell frames (1920 x 1080) that differ in cameraPos and focal (+-10 steps)"""
    st = S.key_states(["UiLo"[f % 4] for f in range(n)], 1080.0)
    assert len({(s.cam, s.focal) for s in st}) > 2
    return [S.camera(s, 1920, 1080) for s in st]


@pytest.mark.parametrize("n", [20, 40])
def test_cam_focal_and_light_changes_share_one_run(n):
    """The light is not an argument of the runs at all; 40 frames are one run too: the 32-frame
    split is a launch detail."""
    assert cgamd.rt_sequence_runs(_moving(n), 28, 1, 1) == [(0, n, "lattice")]


def _pattern(Rs):
    return [cgamd.rt_camera(1920, 1080, 1080.0, R=R) for R in Rs]


def test_a_change_of_route_ends_the_run():
    y1, y2 = cgamd.yaw_matrix(0.1745), cgamd.yaw_matrix(-0.349)
    cams = _pattern([None] * 3 + [y1] * 2 + [y2] * 2 + [None])
    assert cgamd.rt_sequence_runs(cams, 28, 1, 1) == [(0, 3, "lattice"), (3, 7, "lattice_yaw"), (7, 8, "lattice")]
    assert cgamd.rt_sequence_runs(cams, 28, 1, 5) == [(0, 3, "lights"), (3, 7, "lights_yaw"), (7, 8, "lights")]
    cams = _pattern([None, S.pitch(0.2), None])
    assert cgamd.rt_sequence_runs(cams, 28, 1, 1) == [(0, 1, "lattice"), (1, 2, "pixel"), (2, 3, "lattice")]
    # a frame past the lattice bounds (|focal| <= 1e6 under a yaw) ends the run and goes per pixel
    cams = _pattern([y1] * 3)
    cams[1].focal = 2e6
    assert cgamd.rt_sequence_runs(cams, 28, 1, 1) == [(0, 1, "lattice_yaw"), (1, 2, "pixel"), (2, 3, "lattice_yaw")]


def test_runs_of_the_other_routes():
    cams = _moving(4)
    assert cgamd.rt_sequence_runs(cams, 28, 1, 65) == [(0, 4, "pixel")]
    assert cgamd.rt_sequence_runs(cams, 1_000_000, 0, 1) == [(0, 4, "big_lattice")]
    assert cgamd.rt_sequence_runs(cams, 28, 1, 1, cgamd.RtShard(1, 3, 8)) == [(0, 4, "pixel")]
    assert cgamd.rt_sequence_runs(cams, 28, 1, 1, cgamd.RtShard(0, 2, 15)) == [(0, 4, "lattice")]
    assert cgamd.rt_sequence_runs([], 28, 1, 1) == []
    # each run's route is the frame's own cg_rt_route
    mixed = _pattern([None, cgamd.yaw_matrix(0.1745), S.pitch(0.2), None])
    for a, b, r in cgamd.rt_sequence_runs(mixed, 28, 1, 1):
        assert all(cgamd.rt_route(mixed[f], 28, 1, 1) == r for f in range(a, b))


def test_cap_smaller_than_the_run_count():
    lib = cgamd.load()
    cams = _pattern([None] * 3 + [cgamd.yaw_matrix(0.1745)] * 2 + [cgamd.yaw_matrix(-0.349)] * 2 + [None])
    arr = (cgamd.RtCamera * len(cams))(*cams)
    start, route = (C.c_int * 4)(*[-7] * 4), (C.c_int * 4)(*[-7] * 4)
    assert lib.cg_rt_sequence_runs(arr, len(cams), 28, 1, 1, None, start, route, 2) == 3
    assert list(start) == [0, 3, 7, -7] and list(route) == [1, 2, -7, -7]      # two runs, closed by the third's start
    assert lib.cg_rt_sequence_runs(arr, len(cams), 28, 1, 1, None, None, None, 0) == 3


def test_mixed_script_runs():
    """Case 3 of the GPU tests: unrotated -> yawed (two angles) -> unrotated (the yaw back at exactly
    0) -> yawed (negative angle), focal 60 -> 70 -> 60."""
    st = S.key_states(S.SCRIPT_MIXED, 60.0)
    assert [s.focal for s in st] == [60.0] * 2 + [70.0] * 8 + [60.0] * 4
    assert float(st[8].yaw) == 0.0 and float(st[9].yaw) < 0.0 < float(st[3].yaw) < float(st[4].yaw)
    cams = [S.camera(s, 64, 60) for s in st]
    assert cgamd.rt_sequence_runs(cams, 28, 1, 1) == [(0, 3, "lattice"), (3, 8, "lattice_yaw"), (8, 9, "lattice"),
                                                      (9, 14, "lattice_yaw")]


@pytest.mark.parametrize("script,focal", [(S.SCRIPT_LIGHT, 75.0), (S.SCRIPT_MIXED, 60.0)])
def test_gpu_inputs_have_teeth(script, focal):
    """Frames of consecutive states that differ by a light key are pairwise different in the
    oracle (64 x 60), and so are the frames of the case-2 states."""
    st = S.key_states([""] + list(script), focal)   # from the start state on
    pairs = [(a, b) for a, b in zip(st, st[1:]) if a.light != b.light]
    assert len(pairs) >= 4
    for a, b in pairs:
        # the later state's camera with either light: only the light differs
        stale = S.State(b.cam, b.focal, b.yaw, a.light, b.keys)
        assert not np.array_equal(S.oracle_frame(b, 64, 60), S.oracle_frame(stale, 64, 60)), b.keys


def test_cross_states_have_teeth():
    st = S.cross_states()
    assert len(st) == 35 and len({s.light for s in st}) == 35 and len({s.cam for s in st}) == 35
    for a, b in ((st[0], st[1]), (st[30], st[31]), (st[31], st[32]), (st[33], st[34])):
        stale = S.State(b.cam, b.focal, b.yaw, a.light, b.keys)
        assert not np.array_equal(S.oracle_frame(b, 64, 60), S.oracle_frame(stale, 64, 60))
