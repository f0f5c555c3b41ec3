"""CPU: the reference programs' own runs are the root of trust.

tests/golden/ref_sessions.json holds, per frame of 18 scripted sessions, the state the reference's
globals had and the SHA-256 of every plane it drew (tests/golden/make_ref_sessions.py; the
unmodified reference sources built headless by oracle/ref_build.py).  Here

  * the oracle, fed each recorded state, must give the recorded planes bit for bit (raytracer ARGB;
    rasteriser ARGB, depthBuffer, shadowBuffer with the rand() index and the indirect term chained
    as host/rasteriser.cpp chains them; starfield ARGB and the stars themselves);
  * when the reference binaries are there (oracle/_ref/), every session is run again and must give
    the fixture -- which keeps the fixture honest -- and `raytracer` with key U must still write
    raytracer/screenshot.bmp;
  * the Python re-statements of Update() (make_golden.rast_replay_keys / rt_replay_keys) must give
    the recorded states bit for bit.

The GPU at these states: tests/test_ref_sessions_gpu.py."""
import os

import numpy as np
import pytest

import make_golden as mg
import make_ref_sessions as mrs
import oracle
import ref_build
import ref_session_states as rs

f32 = np.float32
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))


def test_fixture_is_current_and_small():
    """The JSON holds exactly the sessions of make_ref_sessions.SESSIONS, one frame per key."""
    assert os.path.getsize(mrs.JSON_PATH) <= 419_230
    assert list(rs.SESSIONS) == list(mrs.SESSIONS)
    for name, spec in mrs.SESSIONS.items():
        got = rs.SESSIONS[name]
        assert {k: got[k] for k in spec} == spec, name
        assert len(got["frames"]) == len(spec["keys"]), name
        assert tuple(got["size"]) == mrs.SIZES[spec["program"]]
    assert not any(s.get("setting") == 1 or s.get("setting_boxes") == 1 for s in mrs.SESSIONS.values())


@pytest.mark.parametrize("name", rs.RT)
def test_oracle_raytracer_matches_reference_frames(name):
    bad = []
    for k, (st, fr) in enumerate(zip(rs.states(name), rs.SESSIONS[name]["frames"])):
        argb = oracle.rt_draw(rs.oracle_rt_params(st), threads=THREADS)
        if mrs.sha(argb) != fr["argb"]:
            bad.append(k)
    assert not bad, f"{name}: oracle frames {bad} differ from the reference's"


@pytest.mark.parametrize("name", rs.RAST)
def test_oracle_rasteriser_matches_reference_frames(name):
    """All three planes; and the host apps' chain of the indirect term (0.15, '1' / '2' steps,
    0.2 after a mode 0 frame with triangles) gives the reference's own value at every frame."""
    keys, frames, sts = rs.SESSIONS[name]["keys"], rs.SESSIONS[name]["frames"], rs.states(name)
    bad, ind = [], f32(0.15)
    for k, a, d, s, cnt, _ in rs.oracle_rast_session(name):
        if keys[k] in "12":
            ind = f32(ind + (f32(0.005) if keys[k] == "2" else -f32(0.005)))
        assert ind.view(np.uint32) == sts[k]["indirect"].view(np.uint32)[0], f"{name} frame {k}: indirect chain"
        for plane, got in (("argb", a), ("depth", d), ("shadow", s)):
            if mrs.sha(got) != frames[k][plane]:
                bad.append((k, plane))
        if sts[k]["mode"] == 0 and cnt.n_tris > 0:
            ind = f32(0.2)
    assert not bad, f"{name}: oracle planes {bad} differ from the reference's"


@pytest.mark.parametrize("name", rs.STAR)
def test_oracle_starfield_matches_reference_frames(name):
    sp = rs.SESSIONS[name]
    stars = oracle.starfield_init(mrs.N_STARS)
    bad = []
    for k, fr in enumerate(sp["frames"]):
        if mrs.sha(stars) != fr["state"]:
            bad.append((k, "stars"))
        if mrs.sha(oracle.starfield_draw(stars, *mrs.SIZES["starfield"])) != fr["argb"]:
            bad.append((k, "argb"))
        oracle.starfield_update(stars, float(sp["dts"][k]))
    assert not bad, f"{name}: oracle {bad} differ from the reference's"
    assert len({fr["argb"] for fr in sp["frames"]}) > 50            # the frames move


@pytest.fixture(scope="module")
def live():
    """Every session run again through the reference binaries, side by side."""
    bins = ref_build.binaries()
    if bins is None:
        pytest.skip("reference binaries absent (oracle/_ref/; built by build() where the reference tree exists)")
    return mrs.run_all(bins)


def test_fixture_matches_live_reference_binaries(live):
    bad = [(name, k) for name, (frames, _) in live.items()
           for k, (got, want) in enumerate(zip(frames, rs.SESSIONS[name]["frames"])) if got != want]
    assert not bad, f"frames whose live dump differs from ref_sessions.json: {bad[:20]}"
    assert all(len(live[n][0]) == len(rs.SESSIONS[n]["frames"]) for n in rs.SESSIONS)


def test_live_raytracer_key_U_reproduces_reference_screenshot(live):
    """The reference's own raytracer/screenshot.bmp, through the stand-in headers: all 81,920 pixels."""
    frames, shot = live["rt_screenshot"]
    want = mg.screenshot_argb()
    assert shot is not None and np.array_equal(shot, want)
    assert frames[-1]["argb"] == mrs.sha(want)


def test_recipe_does_nothing_without_a_reference_tree(tmp_path):
    assert ref_build.build(ref=str(tmp_path / "absent")) is False


def test_recorded_screenshot_frame_is_the_reference_file():
    assert rs.SESSIONS["rt_screenshot"]["frames"][0]["argb"] == mrs.sha(mg.screenshot_argb())


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


IDENTITY = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


@pytest.mark.parametrize("name", rs.RT + rs.RAST)
def test_replay_keys_gives_the_recorded_states(name):
    """Update() as Python re-states it against the reference's own globals, after every key."""
    sp = rs.SESSIONS[name]
    replay = mg.rt_replay_keys if sp["program"] == "raytracer" else mg.rast_replay_keys
    for k, st in enumerate(rs.states(name)):
        got = replay(sp["keys"][:k + 1])
        for field in ("cam", "light"):
            assert _same_bits(got[field], st[field]), f"{name} frame {k}: {field}"
        assert _same_bits([got["yaw"]], st["yaw"]), f"{name} frame {k}: yaw {got['yaw']!r} vs {st['yaw'][0]!r}"
        assert _same_bits([got["focal"]], st["focal"]), f"{name} frame {k}: focal"
        assert _same_bits(got["R"] or IDENTITY, st["R"]), f"{name} frame {k}: R"


def test_turning_back_leaves_the_tiny_yaw():
    """'m' then 'n': yaw = -5.372047e-09, cos = 1 and sin = yaw -- neither the identity nor an
    ordinary yaw.  The reference reaches it in four sessions, textured ones included."""
    hits = 0
    for name in rs.RT + rs.RAST:
        for st in rs.states(name):
            if st["yaw"][0] == rs.TINY_YAW:
                hits += 1
                R = st["R"]
                assert R[0] == 1.0 and R[10] == 1.0 and R[8] == rs.TINY_YAW and R[2] == -rs.TINY_YAW
    assert hits >= 8
    assert len([1 for st in rs.states("rt_turn_back_twice") if st["yaw"][0] == rs.TINY_YAW]) == 3
