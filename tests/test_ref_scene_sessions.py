"""CPU: caller-supplied scenes held to the reference programs' own code.

tests/golden/ref_scene_sessions.json holds, per frame of 18 scripted sessions, the state the
reference's globals had and the SHA-256 of every plane it drew -- on scenes that are not its
Cornell box: meshes, shadow volumes on caller boxes, sub-pixel and degenerate triangles, clouds
that take the raytracer's large-scene path, several spheres, empty scenes
(tests/ref_scene_cases.py; recorded by tests/golden/make_ref_scene_sessions.py from the unmodified
reference sources built with a scene-loading model header, oracle/ref_build.py).  Here

  * the oracle, fed each recorded state and the regenerated scene, must give the recorded planes
    bit for bit (raytracer ARGB; rasteriser ARGB, depthBuffer, shadowBuffer with the rand() index
    chained);
  * when the scene-loading binaries are there (oracle/_ref/), every session is run again and must
    give the fixture, and with CG_REF_SCENE unset they must draw what the unmodified builds draw;
  * the library's host clip (cgamd.rast_prepare) must give the oracle's clipped list and light
    byte for byte at every rasteriser state;
  * the frames are not trivial, and the big-triangle mesh takes every clip case on every plane.

The GPU at these states: tests/test_ref_scene_sessions_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import cgamd
import make_ref_scene_sessions as mrss
import make_ref_sessions as mrs
import oracle
import ref_build
import ref_scene_cases as cases
import ref_scene_states as rss
import ref_session_states as rs

THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
ZERO_PLANE = {n: mrs.sha(np.zeros(w * h, np.uint32)) for n, (w, h) in mrs.SIZES.items()}


def test_fixture_is_current_and_small():
    """The JSON holds exactly the cases of ref_scene_cases, one frame per key, hashes only."""
    assert os.path.getsize(mrss.JSON_PATH) <= mrss.MAX_JSON_BYTES
    assert list(rss.SESSIONS) == [n for n in cases.CASES if n not in mrss.LEFT_OUT]
    for name, got in rss.SESSIONS.items():
        spec = cases.spec(name)
        assert {k: got[k] for k in spec} == spec, name
        assert len(got["frames"]) == len(spec["keys"]), name
        assert tuple(got["size"]) == mrs.SIZES[spec["program"]]
        if spec["program"] == "raytracer":
            assert len(spec["keys"]) <= 8, name
        else:                                   # a yaw out and back, both colour modes, a camera move
            keys = spec["keys"]
            assert keys.count("m") == keys.count("n") > 0 and keys.count(" ") >= 2 and set(keys) & set("UDLRzx"), name


def test_start_values_reach_the_reference_globals():
    """CG_REF_CAM / CG_REF_FOCAL / CG_REF_LIGHT: the first frame without a camera, focal or light
    key shows them in the state the reference dumped."""
    for name, sp in rss.SESSIONS.items():
        keys, st = sp["keys"], rss.states(name)[0]
        if "cam" in sp and keys[0] not in "UDLRzx":
            assert [float(x) for x in st["cam"][:3]] == sp["cam"] and st["cam"][3] == 1.0, name
        if "focal" in sp and keys[0] not in "iofg":
            assert float(st["focal"][0]) == sp["focal"], name
        if "light" in sp and keys[0] not in "wsadqe":
            assert [float(x) for x in st["light"][:3]] == sp["light"] and st["light"][3] == 1.0, name
    assert sum("cam" in sp for sp in rss.SESSIONS.values()) >= 4
    assert sum("light" in sp and "focal" in sp for sp in rss.SESSIONS.values()) >= 2


def test_scene_sizes_and_nan_normals():
    sizes = {n: tuple(len(a) for a in cases.scene(n)) for n in cases.CASES}
    assert sizes["rt_cloud300"] == sizes["rt_cloud300_eye_in"] == sizes["rt_cloud300_eye_v0"] == (300, 0)
    assert sizes["rt_cloud300_sphere"] == (300, 1) and sizes["rt_room_three_spheres"] == (28, 3)
    assert sizes["rt_degenerate40"] == sizes["rt_degenerate40_around_eye"] == (40, 0)
    assert sizes["rt_degenerate300"] == sizes["rt_degenerate300_around_eye"] == (300, 0)
    assert sizes["rt_empty"] == (0, 0) and sizes["rt_one_triangle"] == (1, 0)
    assert sizes["rast_mesh3000"] == (3000, 60) and sizes["rast_subpixel20000"] == (20000, 0)
    assert sizes["rast_clip400"] == (400, 20) and sizes["rast_boxes700"] == (0, 700)
    assert sizes["rast_empty_room_boxes"][0] == 0 < sizes["rast_empty_room_boxes"][1] and sizes["rast_empty"] == (0, 0)
    # the degenerate raytracer scenes hold NaN normals (zero-area triangles), the reference's own bits
    assert np.isnan(cases.scene("rt_degenerate40")[0]["normal"]).any()
    assert np.isnan(cases.scene("rast_degenerate")[0]["normal"]).any()


def test_degenerate_mesh_is_exact_in_camera_space():
    """The first frame's camera is the origin and R the identity: the vertex at z = 0.01f and the
    one on the left plane are exactly there in the oracle's clip space, and the plane tests go the
    reference's way (z > 0.01f fails; x > -w W / 2 fails)."""
    st = rss.states("rast_degenerate")[0]
    assert not st["cam"][:3].any() and st["yaw"][0] == 0 and float(st["focal"][0]) == cases.DEGENERATE_FOCAL
    room = cases.scene("rast_degenerate")[0]
    assert room["v"][5, 0, 2] == np.float32(0.01)
    x, z = room["v"][6, 0, 0], room["v"][6, 0, 2]
    w = np.float32(z / np.float32(cases.DEGENERATE_FOCAL))
    assert x == np.float32(np.float32(w * np.float32(-900.0)) / np.float32(2))
    assert (room["v"][7, :, 2] < 0).all()
    # the tiny yaw after 'm' 'n' leaves the z = 0.01f vertex (x = 0) where it is
    st2 = rss.states("rast_degenerate")[2]
    assert st2["yaw"][0] == rss.TINY_YAW and not st2["cam"][:3].any()


@pytest.mark.parametrize("name", rss.RT)
def test_oracle_raytracer_matches_reference_frames(name):
    rss.check_scene(name)
    scene = cases.rt_oracle_scene(name)
    bad = []
    for k, (st, fr) in enumerate(zip(rss.states(name), rss.SESSIONS[name]["frames"])):
        argb = oracle.rt_draw(rss.oracle_rt_params(st), threads=THREADS, scene=scene)
        if mrs.sha(argb) != fr["argb"]:
            bad.append(k)
    assert not bad, f"{name}: oracle frames {bad} differ from the reference's"


@pytest.mark.parametrize("name", rss.RAST)
def test_oracle_rasteriser_matches_reference_frames(name):
    rss.check_scene(name)
    frames = rss.SESSIONS[name]["frames"]
    bad = []
    for k, a, d, s, _, _ in rss.oracle_rast_session(name):
        bad += [(k, plane) for plane, got in (("argb", a), ("depth", d), ("shadow", s)) if mrs.sha(got) != frames[k][plane]]
    assert not bad, f"{name}: oracle planes {bad} differ from the reference's"


@pytest.mark.parametrize("name", rss.RAST)
def test_host_clip_matches_oracle_geometry(name):
    """cgamd.rast_prepare (the library's host clip) against oracle.rast_geometry on the mesh:
    the clipped list and the light, byte for byte, at every recorded state."""
    lib_scene, ora_scene = cases.rast_library_scene(name), cases.rast_oracle_scene(name)
    for k, st in enumerate(rss.states(name)):
        p = cgamd.rast_params(900, 720, float(st["focal"][0]), rs.t4(st["cam"]), [float(x) for x in st["R"]],
                              rs.t4(st["light"]), float(st["indirect"][0]), st["mode"], 0, float(st["yaw"][0]))
        tris, n, light = cgamd.rast_prepare(p, *lib_scene)
        otris, on, olight = oracle.rast_geometry(rss.oracle_rast_params(st, 0), scene=ora_scene)
        assert n == on, f"{name} frame {k}: {n} clipped triangles, the oracle {on}"
        assert bytes(light) == bytes(olight), f"{name} frame {k}: light"
        got = np.frombuffer(C.string_at(tris, n * 84), np.uint32).reshape(n, 21)
        want = np.frombuffer(C.string_at(otris, n * 84), np.uint32).reshape(n, 21)
        diff = np.flatnonzero((got != want).any(axis=1))
        assert diff.size == 0, f"{name} frame {k}: clipped triangles {diff[:8]} of {n} differ"


@pytest.mark.parametrize("name", list(rss.SESSIONS))
def test_frames_are_not_trivial(name):
    sp = rss.SESSIONS[name]
    hashes = {fr["argb"] for fr in sp["frames"]}
    if name in cases.EMPTY:
        # an empty raytracer frame is all 0x80000000 (black, PutPixelSDL's alpha); the rasteriser's is zeros
        assert len(hashes) == 1
        return
    assert len(hashes) >= 2, name
    if sp["program"] == "rasteriser":
        assert any(fr["depth"] != ZERO_PLANE["rasteriser"] for fr in sp["frames"]), name


def test_big_triangles_take_every_clip_case():
    """rast_clip400: each of the seven in/out cases (all in; only v0 / v1 / v2 in; only v2 / v1 / v0
    out) occurs on each of planes 1-4 and 6 over the session's frames, here on random triangles
    about as large as the frustum with the camera among them.  (The recorded sessions of the
    reference's own scene take all 35 as well -- rast_fly_in flies into the boxes -- but only on
    its axis-aligned walls and two blocks.)"""
    planes = [1, 2, 3, 4, 6]
    scene = cases.rast_oracle_scene("rast_clip400")
    got = np.zeros((7, 8), np.uint64)
    for st in rss.states("rast_clip400"):
        got += oracle.rast_clip_cases(rss.oracle_rast_params(st, 0), scene)
    print(got)
    assert (got[planes][:, :7] > 0).all(), got
    assert got[5, 7] > 0 and got[5, 0] > 0            # triangles behind the near plane, and in front


# ---- the live binaries -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_bins():
    bins = ref_build.scene_binaries()
    if bins is None:
        pytest.skip("scene-loading reference binaries absent (oracle/_ref/; built by build() where the "
                    "reference tree exists)")
    return bins


def test_fixture_matches_live_scene_binaries(scene_bins):
    live = mrss.run_all(scene_bins)
    assert list(live) == list(rss.SESSIONS)
    bad = [(name, k) for name, (frames,) in live.items()
           for k, (got, want) in enumerate(zip(frames, rss.SESSIONS[name]["frames"])) if got != want]
    assert not bad, f"frames whose live dump differs from ref_scene_sessions.json: {bad[:20]}"
    assert all(len(live[n][0]) == len(rss.SESSIONS[n]["frames"]) for n in rss.SESSIONS)


@pytest.mark.parametrize("name", ["rt_mixed", "rast_modes"])
def test_scene_builds_draw_the_reference_scene_unchanged(scene_bins, tmp_path, name):
    """With CG_REF_SCENE unset the substituted model header calls the reference's own
    LoadTestModel: the _scene build gives the frames the unmodified build recorded."""
    frames, _ = mrs.run_session(name, mrs.SESSIONS[name], scene_bins, str(tmp_path))
    assert frames == rs.SESSIONS[name]["frames"]


def test_accessors_keep_the_two_sets_apart():
    bins, scene = ref_build.binaries(), ref_build.scene_binaries()
    if bins is not None:
        assert set(bins) == set(ref_build.PROGRAMS) and not any(p.endswith("_scene") for p in bins.values())
    if scene is not None:
        assert set(scene) == set(ref_build.SCENE_PROGRAMS) and all(p.endswith("_scene") for p in scene.values())
