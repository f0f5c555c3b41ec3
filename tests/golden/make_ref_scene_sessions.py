"""Record sessions of the reference programs on caller-supplied scenes into
tests/golden/ref_scene_sessions.json.

The reference's raytracer and rasteriser, their sources unmodified, are built a second time with
a model header that reads the scene from a file (oracle/ref_shim/scene/, oracle/ref_build.py ->
oracle/_ref/raytracer_scene, rasteriser_scene).  Every scene of tests/ref_scene_cases.py is
written to a temporary file and run over its key script; per session the JSON keeps the case
name, the SHA-256 of the scene bytes the binary was given, the keys and start values, and per
frame the state record and the plane hashes in make_ref_sessions.py's format.

A session becomes a fixture only if

  * the reference binary exits 0,
  * its states and planes are identical under two values of MALLOC_PERTURB_ (glibc fills
    allocated and freed memory with that byte: a frame that reads uninitialised or freed heap
    memory changes with it), and
  * the normals the reference computed for the scene (CG_REF_SCENE_NORMALS) equal the scene's,
    as bits, NaN payloads included.

LEFT_OUT lists the meshes that fail one of these, with the reason; neither side is changed for them.

Usage: python tests/golden/make_ref_scene_sessions.py   (needs the reference tree; writes the JSON)
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for sub in ("oracle", "computer-graphics_amd", "tests", os.path.join("tests", "golden")):
    if os.path.join(ROOT, sub) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, sub))

import make_ref_sessions as mrs  # noqa: E402

JSON_PATH = os.path.join(HERE, "ref_scene_sessions.json")
MAX_JSON_BYTES = 100_000
PERTURB = ("85", "170")          # 0x55, 0xAA
# case name: why the reference's behaviour on it is undefined (none so far)
LEFT_OUT = {}


def _float_text(x):
    return repr(float(np.float32(x)))      # the shortest text of the float's double: strtof reads it back exactly


def session_env(spec, scene_file, normals_file=None, perturb=None):
    env = {"CG_REF_SCENE": scene_file, "CG_REF_BOX_INDEX": None}      # the last box's index is the record's
    if "cam" in spec:
        env["CG_REF_CAM"] = ",".join(_float_text(x) for x in spec["cam"])
    if "focal" in spec:
        env["CG_REF_FOCAL"] = _float_text(spec["focal"])
    if "light" in spec:
        env["CG_REF_LIGHT"] = ",".join(_float_text(x) for x in spec["light"])
    if normals_file:
        env["CG_REF_SCENE_NORMALS"] = normals_file
    if perturb is not None:
        env["MALLOC_PERTURB_"] = perturb
    return env


def scene_sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def run_case(name, binaries, workdir, perturb=None, check_normals=False):
    """One session of a scene-loading binary -> frames ([{"state": ..., plane: sha}])."""
    import ref_scene_cases as cases
    spec = cases.spec(name)
    tag = f"{name}.{perturb or 'plain'}"
    scene_file = os.path.join(workdir, tag + ".scene")
    normals_file = os.path.join(workdir, tag + ".normals") if check_normals else None
    with open(scene_file, "wb") as f:
        f.write(cases.scene_bytes(name))
    frames, _ = mrs.run_session(tag, spec, binaries, workdir, session_env(spec, scene_file, normals_file, perturb))
    if check_normals:
        a, b = cases.scene(name)
        want = a["normal"] if spec["program"] == "raytracer" else np.concatenate([a["normal"], b["normal"]])
        got = np.fromfile(normals_file, np.uint32).reshape(-1, 4)
        want = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad = np.flatnonzero((got != want).any(axis=1)) if got.shape == want.shape else "all"
            raise RuntimeError(f"{name}: the reference's normals differ from the scene's at triangles {bad}")
        os.unlink(normals_file)
    os.unlink(scene_file)
    return frames


def run_all(binaries, names=None, jobs=None, perturbs=(None,), check_normals=False):
    """{name: [frames per value of perturbs]}, the sessions side by side."""
    from concurrent.futures import ThreadPoolExecutor
    import ref_scene_cases as cases
    names = [n for n in cases.CASES if n not in LEFT_OUT] if names is None else list(names)
    for n in names:
        cases.scene(n)                               # build the scenes before the threads start
    work = tempfile.mkdtemp(prefix="cg_ref_scene_sessions_")
    try:
        jobs = jobs or max(1, min(8, len(os.sched_getaffinity(0))))
        with ThreadPoolExecutor(jobs) as ex:
            futs = {n: [ex.submit(run_case, n, binaries, work, p, check_normals) for p in perturbs] for n in names}
            return {n: [f.result() for f in fs] for n, fs in futs.items()}
    finally:
        shutil.rmtree(work, ignore_errors=True)


def load():
    with open(JSON_PATH) as f:
        return json.load(f)["sessions"]


def main():
    import ref_build
    import ref_scene_cases as cases
    if not ref_build.build():
        raise SystemExit(f"no reference tree at {ref_build.reference_dir()}")
    t0 = time.time()
    res = run_all(ref_build.scene_binaries(), perturbs=PERTURB, check_normals=True)
    print(f"recorded in {time.time() - t0:.1f} s")
    out = {"generator": "tests/golden/make_ref_scene_sessions.py",
           "note": "states and plane hashes recorded from the reference programs' own runs on the scenes of "
                   "tests/ref_scene_cases.py",
           "sessions": {}}
    for name, (first, second) in res.items():
        if first != second:
            bad = [k for k, (a, b) in enumerate(zip(first, second)) if a != b]
            raise SystemExit(f"{name}: frames {bad} change with MALLOC_PERTURB_: the reference reads memory it did "
                             f"not write; list the case in LEFT_OUT")
        spec = cases.spec(name)
        out["sessions"][name] = dict(spec, scene_sha256=scene_sha(cases.scene_bytes(name)),
                                     size=list(mrs.SIZES[spec["program"]]), frames=first)
        print(f"{name}: {len(first)} frames")
    blocks = []
    for name, sess in out["sessions"].items():
        head = json.dumps({k: v for k, v in sess.items() if k != "frames"})[:-1]
        rows = ",\n".join("   " + json.dumps(fr) for fr in sess["frames"])
        blocks.append(f'  {json.dumps(name)}: {head}, "frames": [\n{rows}]}}')
    with open(JSON_PATH, "w") as f:       # one frame per line
        f.write('{"generator": %s,\n "note": %s,\n "sessions": {\n' % (json.dumps(out["generator"]), json.dumps(out["note"])))
        f.write(",\n".join(blocks) + "\n }\n}\n")
    load()
    size = os.path.getsize(JSON_PATH)
    assert size <= MAX_JSON_BYTES, size
    print("wrote", JSON_PATH, size, "bytes")


if __name__ == "__main__":
    main()
