"""Record sessions of the reference programs themselves into tests/golden/ref_sessions.json.

The reference's raytracer, rasteriser and starfield, compiled unmodified against the stand-in
headers of oracle/ref_shim/ (oracle/ref_build.py -> oracle/_ref/), are run over the fixed key
scripts / tick lists below.  Per frame the JSON keeps

  * "state": the program's own globals when Update() returns, as hex float bits (layouts in
    STATE_LAYOUT; the starfield's stars as a SHA-256), and
  * the SHA-256 of every plane the program produced: ARGB, and for the rasteriser its
    depthBuffer and shadowBuffer.

Hashes only: on a mismatch a test diagnoses pixels with the live oracle.  The tests feed the
recorded states to the oracle and to the GPU library, so no Python re-reading of Update() stands
between the reference and the code under test.

The rasteriser's texture maps reach the reference binary through cv.hpp's imread stand-in as
"<name>.jpg.bgr" files written here from oracle.jpeg_decode of tests/golden/textures: texel
values are pinned only through the oracle's JPEG decode.  Settings that index the marble map
(setting == 1 or settingBoxes == 1) are left out: Marble2000x2000.jpg is missing from the
reference tree, the reference then reads out of bounds, and a synthetic marble would pin nothing.

Usage: python tests/golden/make_ref_sessions.py   (needs the reference tree; writes the JSON)
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
JSON_PATH = os.path.join(HERE, "ref_sessions.json")
TEXTURE_DIR = os.path.join(HERE, "textures")

SIZES = {"raytracer": (320, 256), "rasteriser": (900, 720), "starfield": (320, 256)}   # #defines
PLANES = {"raytracer": ("argb",), "rasteriser": ("argb", "depth", "shadow"), "starfield": ("argb",)}
# words of a state record, as the stand-in SDL.h writes them
STATE_LAYOUT = {
    "raytracer": (("cam", 4), ("yaw", 1), ("R", 16), ("focal", 1), ("light", 4)),
    "rasteriser": (("cam", 4), ("yaw", 1), ("R", 16), ("focal", 1), ("light", 4), ("indirect", 1), ("mode", 1)),
}
N_STARS = 1000
# TestModelH.h:254-257 never assigns top_tallBlock2.index, and findU / findV read it when the boxes
# are textured: undefined behaviour (left alone, the stack value of one build changed 113 pixels on
# that face in the first frame of settings 0 / 2).  The stand-in SDL.h gives that one field this value
# before the first frame -- the "no object" value that oracle/ and the library use (texel 0, 0) --
# so that face pins the convention, not the reference.  Everything else on those frames is pinned.
UNSET_BOX_INDEX = -1

# starfield frame times (ms): 0, 1, 16 and 33 and a few of 400-2500 so that stars wrap
STAR_DTS = [0, 1, 16, 33, 16, 16, 400, 16, 33, 1, 0, 16, 2500, 16, 16, 33, 33, 900, 16, 1,
            16, 16, 16, 1300, 0, 0, 33, 16, 16, 450, 16, 16, 33, 1, 16, 2000, 16, 16, 16, 33,
            700, 16, 16, 0, 1, 33, 16, 1700, 16, 16, 16, 16, 33, 400, 16, 16, 1, 2500, 16, 16]

# Key letters as the host apps' --keys: U D L R arrows, ' ' SPACE, others themselves.
SESSIONS = {
    # ---- raytracer (w s a d q e light, U D L R camera, n m yaw, i o focal) ----
    "rt_screenshot": dict(program="raytracer", keys="U"),                 # raytracer/screenshot.bmp
    "rt_mixed": dict(program="raytracer", keys="wUimmaRnnnoqDe"),
    "rt_turn_back": dict(program="raytracer", keys="mn"),                 # yaw -5.372047e-09
    "rt_turn_back_twice": dict(program="raytracer", keys="mnUmmnn"),
    "rt_walk_in": dict(program="raytracer", keys="U" * 22 + "m" * 9 + "e" * 6 + "d" * 7 + "o" * 20),
    "rt_random40": dict(program="raytracer", keys="iDmnoedDwnoiDsaweLdsdUsLdnnLdawwasmmqDUq"),
    # ---- rasteriser (+ 1 2 indirect, z x camera y, f g focal, SPACE colour mode) ----
    "rast_modes": dict(program="rasteriser", keys="Udnfz1 U "),           # modes 0, 1, 1, 2
    "rast_turn_back": dict(program="rasteriser", keys="mn"),
    # flies into the boxes and yaws through two colour modes (51 frames)
    "rast_fly_in": dict(program="rasteriser",
                        keys="U" * 14 + "mm" + "U" * 6 + " " + "nnnn" + "UUU" + "L" * 4 + " " + "mmm" + "xx" + "U" * 5
                             + " " + "nzzRR"),
    # focal 512 -> 212, then mode 1 where '1' x 45 drives the indirect term negative (153 frames)
    "rast_long": dict(program="rasteriser",
                      keys="g" * 60 + " " + "1" * 45 + "w" * 12 + "q" * 8 + "a" * 15 + " " + "D" * 10 + "x"),
    "rast_random40_a": dict(program="rasteriser", keys="1naL1a  sf1n1nLeD qasRd1az1wgzgfzqezz1eD"),
    "rast_random40_b": dict(program="rasteriser", keys="mRnxnn21wwf1aggqResdenfm eDwRUUnng2zmL2n"),
    # textured: grill = 2, woven wood = 3; a yaw out and back, a camera move, SPACE x 3 (modes 1, 2, 0)
    "rast_tex_2_0": dict(program="rasteriser", keys="UmdzLn   R", setting=2, setting_boxes=0),
    "rast_tex_3_0": dict(program="rasteriser", keys="DnaxRm   U", setting=3, setting_boxes=0),
    "rast_tex_0_2": dict(program="rasteriser", keys="UUmeUn   z", setting=0, setting_boxes=2),
    "rast_tex_0_3": dict(program="rasteriser", keys="LnUUqm   x", setting=0, setting_boxes=3),
    "rast_tex_2_3": dict(program="rasteriser", keys="mUfUwn   D", setting=2, setting_boxes=3),
    # ---- starfield: '.' = a frame without a key ----
    "star_60": dict(program="starfield", keys="." * 60, dts=STAR_DTS),
}
assert len(SESSIONS["rast_fly_in"]["keys"]) == 51 and len(SESSIONS["rast_long"]["keys"]) == 153
assert len(STAR_DTS) == 60


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def star_ticks(dts):
    """SDL_GetTicks values that give the frame times dts: main and the static in Update() each
    consume one tick before the first frame's t2 (starfield skeleton.cpp:36, :84-85)."""
    ticks, t = [0, 0], 0
    for d in dts:
        t += int(d)
        ticks.append(t)
    return ticks


def textured(spec):
    return bool(spec.get("setting", 0) or spec.get("setting_boxes", 0))


def write_bgr_maps(workdir):
    """Textures/<file>.bgr for cv.hpp's imread: int32 rows, cols, channels, then the texels of
    oracle.jpeg_decode (cv::imread(..., CV_LOAD_IMAGE_UNCHANGED))."""
    import oracle
    d = os.path.join(workdir, "Textures")
    os.makedirs(d, exist_ok=True)
    for fn in sorted(os.listdir(TEXTURE_DIR)):
        if not fn.endswith(".jpg"):
            continue
        with open(os.path.join(TEXTURE_DIR, fn), "rb") as f:
            img = oracle.jpeg_decode(f.read())
        ch = 1 if img.ndim == 2 else img.shape[2]
        with open(os.path.join(d, fn + ".bgr"), "wb") as f:
            f.write(np.array([img.shape[0], img.shape[1], ch], "<i4").tobytes())
            f.write(np.ascontiguousarray(img).tobytes())


def run_session(name, spec, binaries, workdir, extra_env=None):
    """Run one session of a reference binary in workdir (which holds Textures/ when the session is
    textured).  -> (frames, screenshot ARGB or None); frames = [{"state": ..., plane: sha}].
    extra_env: further variables for the binary ({name: value}; None removes one set here)."""
    prog = spec["program"]
    W, H = SIZES[prog]
    npx = W * H
    tag = os.path.join(workdir, name)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CG_REF_")}
    env.update(CG_REF_KEYS=spec["keys"], CG_REF_FRAMES=tag + ".frames", CG_REF_STATE=tag + ".state")
    if prog == "rasteriser":
        env.update(CG_REF_SETTING=str(spec.get("setting", 0)), CG_REF_SETTING_BOXES=str(spec.get("setting_boxes", 0)),
                   CG_REF_BOX_INDEX=str(UNSET_BOX_INDEX))
    if "dts" in spec:
        env["CG_REF_TICKS"] = ",".join(str(t) for t in star_ticks(spec["dts"]))
    for k, v in (extra_env or {}).items():
        if v is None:
            env.pop(k, None)
        else:
            env[k] = v
    run = os.path.join(workdir, name + ".run")       # the program writes screenshot.bmp into its cwd
    os.makedirs(run, exist_ok=True)
    if textured(spec):
        os.symlink(os.path.join(workdir, "Textures"), os.path.join(run, "Textures"))
    r = subprocess.run([binaries[prog]], cwd=run, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: {prog} exited with {r.returncode}: {r.stderr[-2000:]}")
    n = len(spec["keys"])
    planes = PLANES[prog]
    raw = np.fromfile(tag + ".frames", np.uint32)
    if raw.size != n * len(planes) * npx:
        raise RuntimeError(f"{name}: {raw.size} words of frames, expected {n} x {len(planes)} x {npx}")
    raw = raw.reshape(n, len(planes), npx)
    st = np.fromfile(tag + ".state", np.uint32)
    words = 3 * N_STARS if prog == "starfield" else sum(k for _, k in STATE_LAYOUT[prog])
    if st.size != n * words:
        raise RuntimeError(f"{name}: {st.size} words of state, expected {n} x {words}")
    st = st.reshape(n, words)
    frames = []
    for f in range(n):
        e = {"state": sha(st[f]) if prog == "starfield" else st[f].astype(">u4").tobytes().hex()}
        for k, pl in enumerate(planes):
            e[pl] = sha(raw[f, k])
        frames.append(e)
    shot = os.path.join(run, "screenshot.bmp")
    argb = None
    if os.path.exists(shot):
        import make_golden as mg
        argb = mg.screenshot_argb(shot)
    for p in (tag + ".frames", tag + ".state"):
        os.unlink(p)
    shutil.rmtree(run)
    return frames, argb


def run_all(binaries, names=None, jobs=None):
    """{name: (frames, screenshot)} for the sessions, run side by side."""
    from concurrent.futures import ThreadPoolExecutor
    names = list(SESSIONS) if names is None else list(names)
    work = tempfile.mkdtemp(prefix="cg_ref_sessions_")
    try:
        if any(textured(SESSIONS[n]) for n in names):
            write_bgr_maps(work)
        jobs = jobs or max(1, min(8, len(os.sched_getaffinity(0))))
        with ThreadPoolExecutor(jobs) as ex:
            futs = {n: ex.submit(run_session, n, SESSIONS[n], binaries, work) for n in names}
            return {n: f.result() for n, f in futs.items()}
    finally:
        shutil.rmtree(work, ignore_errors=True)


# ---- readers, shared by the tests ----

def load():
    with open(JSON_PATH) as f:
        return json.load(f)["sessions"]


def decode_state(program, hexstate):
    """A recorded state as {field: float32 array} ("mode": int)."""
    w = np.frombuffer(bytes.fromhex(hexstate), ">u4").astype(np.uint32)
    out, o = {}, 0
    for name, k in STATE_LAYOUT[program]:
        v = w[o:o + k]
        out[name] = int(v[0]) if name == "mode" else v.view(np.float32).copy()
        o += k
    assert o == w.size
    return out


def main():
    import ref_build
    if not ref_build.build():
        raise SystemExit(f"no reference tree at {ref_build.reference_dir()}")
    res = run_all(ref_build.binaries())
    import make_golden as mg
    assert np.array_equal(res["rt_screenshot"][1], mg.screenshot_argb()), "raytracer 'U' differs from screenshot.bmp"
    out = {"generator": "tests/golden/make_ref_sessions.py",
           "note": "states and plane hashes recorded from the reference programs' own runs",
           "sessions": {}}
    for name, spec in SESSIONS.items():
        frames, shot = res[name]
        if shot is not None:
            assert sha(shot) == frames[-1]["argb"], f"{name}: screenshot.bmp is not the last frame"
        out["sessions"][name] = dict(spec, size=list(SIZES[spec["program"]]), frames=frames)
        print(f"{name}: {len(frames)} frames")
    blocks = []
    for name, sess in out["sessions"].items():
        head = json.dumps({k: v for k, v in sess.items() if k != "frames"})[:-1]
        rows = ",\n".join("   " + json.dumps(fr) for fr in sess["frames"])
        blocks.append(f'  {json.dumps(name)}: {head}, "frames": [\n{rows}]}}')
    with open(JSON_PATH, "w") as f:       # one frame per line
        f.write('{"generator": %s,\n "note": %s,\n "sessions": {\n' % (json.dumps(out["generator"]), json.dumps(out["note"])))
        f.write(",\n".join(blocks) + "\n }\n}\n")
    load()
    print("wrote", JSON_PATH, os.path.getsize(JSON_PATH), "bytes")


if __name__ == "__main__":
    main()
