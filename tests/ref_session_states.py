"""Helpers of tests/test_ref_sessions*.py: the sessions recorded from the reference programs' own
runs (tests/golden/ref_sessions.json) as oracle / library arguments.  Every frame's arguments come
from the state the reference itself dumped, not from a re-reading of Update()."""
import functools

import numpy as np

import make_golden as mg
import make_ref_sessions as mrs

SESSIONS = mrs.load()
RT = [n for n, s in SESSIONS.items() if s["program"] == "raytracer"]
RAST = [n for n, s in SESSIONS.items() if s["program"] == "rasteriser"]
RAST_PLAIN = [n for n in RAST if not mrs.textured(SESSIONS[n])]
STAR = [n for n, s in SESSIONS.items() if s["program"] == "starfield"]
LIGHT_COLOUR = (14.0, 14.0, 14.0)        # raytracer skeleton.cpp:88
TINY_YAW = np.float32(float(np.float32(0.174533)) - 0.174533)   # -5.372047e-09: 'm' then 'n'


@functools.lru_cache(maxsize=None)
def states(name):
    """The decoded states of a session's frames (read-only arrays)."""
    prog = SESSIONS[name]["program"]
    out = []
    for fr in SESSIONS[name]["frames"]:
        st = mrs.decode_state(prog, fr["state"])
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(st)
    return out


def t4(v):
    return tuple(float(x) for x in v)


def oracle_rt_params(st):
    import oracle
    return oracle.rt_params(320, 256, float(st["focal"][0]), t4(st["cam"]), [float(x) for x in st["R"]], 0.5,
                            [(t4(st["light"]), LIGHT_COLOUR)])


def oracle_rast_params(name, st, rand_offset):
    import oracle
    sp = SESSIONS[name]
    return oracle.rast_params(900, 720, float(st["focal"][0]), t4(st["cam"]), [float(x) for x in st["R"]],
                              t4(st["light"]), float(st["indirect"][0]), st["mode"], rand_offset,
                              setting=sp.get("setting", 0), setting_boxes=sp.get("setting_boxes", 0),
                              yaw=float(st["yaw"][0]))


@functools.lru_cache(maxsize=1)
def oracle_texture_maps():
    """The oracle's decode of tests/golden/textures, as oracle.rast_set_textures takes it."""
    import oracle
    return {k: oracle.jpeg_decode(v) for k, v in mg.texture_jpegs().items()}


def oracle_rast_session(name, upto=None):
    """The oracle's frames of a rasteriser session at the recorded states, the rand() call index
    chained as host/rasteriser.cpp does (+= 3 * n_shaded in colour modes 1-2).  Yields
    (frame index, argb, depth, shadow, counters, rand_offset the frame started at)."""
    import oracle
    tex = mrs.textured(SESSIONS[name])
    if tex:
        oracle.rast_set_textures(oracle_texture_maps())
    try:
        off = 0
        for k, st in enumerate(states(name)[:upto]):
            a, d, s, cnt = oracle.rast_draw(oracle_rast_params(name, st, off), counters=True)
            yield k, a, d, s, cnt, off
            if st["mode"]:
                off += 3 * int(cnt.n_shaded)
    finally:
        if tex:
            oracle.rast_set_textures(None)


def diff_report(what, got, ref):
    """Count and first differing pixels of two planes, compared as bits."""
    g = got.view(np.uint32) if got.dtype != np.uint32 else got
    r = ref.view(np.uint32) if ref.dtype != np.uint32 else ref
    bad = np.flatnonzero(g != r)
    first = ", ".join(f"[{i}] got {int(g[i]):#010x} want {int(r[i]):#010x}" for i in bad[:6])
    return f"{what}: {bad.size} of {g.size} differ; {first}"
