"""TEST INFRASTRUCTURE ONLY -- headless builds of the reference programs.

Compiles the reference's raytracer, rasteriser and starfield, unmodified, against the stand-in
headers in oracle/ref_shim/ and the reference's own glm/, into oracle/_ref/ (ignored by git).
The rasteriser names its OpenCV header by an absolute path of its author's machine; that one
line is rewritten to "cv.hpp" in a generated copy under oracle/_ref/, which is never committed.

Flags are the reference Makefile's -O3 -Wno-switch and nothing else: no -march=native and no
-ffast-math, since contraction to FMA would change bits.

The reference tree is found through CG_REFERENCE_DIR (default /root/reference).  Without it
nothing is built and nothing fails: the recorded sessions in tests/golden/ref_sessions.json
are all that the GPU tests need.

Usage: python oracle/ref_build.py
"""
from __future__ import annotations

import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "ref_shim")
OUT = os.path.join(HERE, "_ref")
PROGRAMS = ("raytracer", "rasteriser", "starfield")
DEFINES = {"raytracer": "-DCG_REF_RT", "rasteriser": "-DCG_REF_RAST", "starfield": "-DCG_REF_STAR"}
CXXFLAGS = ["-O3", "-Wno-switch"]


def reference_dir():
    return os.environ.get("CG_REFERENCE_DIR", "/root/reference")


def binaries():
    """{program: path} of the built reference binaries, or None when any is missing."""
    paths = {p: os.path.join(OUT, p) for p in PROGRAMS}
    return paths if all(os.access(v, os.X_OK) for v in paths.values()) else None


def _newer(target, sources):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def build(ref=None, force=False):
    """Build oracle/_ref/{raytracer,rasteriser,starfield}.  Returns False (and does nothing)
    when the reference tree is absent."""
    ref = ref or reference_dir()
    if not all(os.path.isfile(os.path.join(ref, p, "Source", "skeleton.cpp")) for p in PROGRAMS):
        return False
    os.makedirs(OUT, exist_ok=True)
    shim = [os.path.join(SHIM, "SDL.h"), os.path.join(SHIM, "cv.hpp"), os.path.abspath(__file__)]
    for prog in PROGRAMS:
        srcdir = os.path.join(ref, prog, "Source")
        src = os.path.join(srcdir, "skeleton.cpp")
        exe = os.path.join(OUT, prog)
        deps = shim + [os.path.join(srcdir, f) for f in os.listdir(srcdir) if f.endswith((".h", ".cpp"))]
        if not force and _newer(exe, deps):
            continue
        if prog == "rasteriser":
            with open(src, encoding="utf-8", errors="surrogateescape") as f:
                text = f.read()
            text, n = re.subn(r'(?m)^#include\s+"/[^"\n]*opencv/cv\.hpp"', '#include "cv.hpp"', text)
            if n != 1:
                raise RuntimeError(f"{src}: expected one absolute OpenCV include, found {n}")
            gen = os.path.join(OUT, "rasteriser_src")
            os.makedirs(gen, exist_ok=True)
            src = os.path.join(gen, "skeleton.cpp")
            with open(src, "w", encoding="utf-8", errors="surrogateescape") as f:
                f.write(text)
        cmd = ["g++", *CXXFLAGS, DEFINES[prog], "-I", SHIM, "-I", srcdir, "-I", os.path.join(ref, "glm"),
               src, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("reference build failed: " + " ".join(cmd) + "\n" + r.stderr[-4000:])
    return True


if __name__ == "__main__":
    print("built" if build(force=True) else f"no reference tree at {reference_dir()}: nothing built")
