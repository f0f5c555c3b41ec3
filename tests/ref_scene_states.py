"""Helpers of tests/test_ref_scene_sessions*.py: the sessions the reference programs ran on the
scenes of tests/ref_scene_cases.py (tests/golden/ref_scene_sessions.json) as oracle / library
arguments.  Every frame's arguments come from the state the reference itself dumped."""
import functools

import numpy as np

import make_ref_scene_sessions as mrss
import make_ref_sessions as mrs
import ref_scene_cases as cases
from ref_session_states import LIGHT_COLOUR, TINY_YAW, diff_report, t4  # noqa: F401

SESSIONS = mrss.load()
RT = [n for n, s in SESSIONS.items() if s["program"] == "raytracer"]
RAST = [n for n, s in SESSIONS.items() if s["program"] == "rasteriser"]


@functools.lru_cache(maxsize=None)
def states(name):
    out = []
    for fr in SESSIONS[name]["frames"]:
        st = mrs.decode_state(SESSIONS[name]["program"], fr["state"])
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(st)
    return out


def check_scene(name):
    """The regenerated scene is the one the reference binary was given."""
    got = mrss.scene_sha(cases.scene_bytes(name))
    assert got == SESSIONS[name]["scene_sha256"], f"{name}: the regenerated scene differs from the recorded one"


def oracle_rt_params(st):
    import oracle
    return oracle.rt_params(320, 256, float(st["focal"][0]), t4(st["cam"]), [float(x) for x in st["R"]], 0.5,
                            [(t4(st["light"]), LIGHT_COLOUR)])


def oracle_rast_params(st, rand_offset):
    import oracle
    return oracle.rast_params(900, 720, float(st["focal"][0]), t4(st["cam"]), [float(x) for x in st["R"]],
                              t4(st["light"]), float(st["indirect"][0]), st["mode"], rand_offset,
                              yaw=float(st["yaw"][0]))


def oracle_rast_session(name, upto=None):
    """The oracle's frames of a rasteriser session at the recorded states, the rand() call index
    chained as ref_session_states.oracle_rast_session chains it (+= 3 * n_shaded in colour modes
    1-2).  Yields (frame index, argb, depth, shadow, counters, rand_offset the frame started at)."""
    import oracle
    scene = cases.rast_oracle_scene(name)
    off = 0
    for k, st in enumerate(states(name)[:upto]):
        a, d, s, cnt = oracle.rast_draw(oracle_rast_params(st, off), counters=True, scene=scene)
        yield k, a, d, s, cnt, off
        if st["mode"]:
            off += 3 * int(cnt.n_shaded)
