#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of libcgamd.so, symbol by symbol.

    python scripts/codeobj_diff.py OLD/libcgamd.so NEW/libcgamd.so

Every function and object of every code object (codeobj.kernel_symbols) must exist in both and
hold the same bytes; kernel descriptors (`.kd`) are compared with their code-entry offset
(bytes 16-23) masked, as codeobj.kernel_sha256 masks it.  Exit status 1 on any difference: a
host-only change must print "0 differences".
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "computer-graphics_amd"))
import codeobj  # noqa: E402


def symbols(path):
    out = {}
    for s, b in codeobj.kernel_symbols(path).items():
        out[s] = b[:16] + bytes(8) + b[24:] if s.endswith(".kd") and len(b) >= 24 else b
    return out


def main(old, new):
    a, b = symbols(old), symbols(new)
    diff = [f"only in {old}: {s}" for s in sorted(a.keys() - b.keys())]
    diff += [f"only in {new}: {s}" for s in sorted(b.keys() - a.keys())]
    diff += [f"bytes differ: {s}" for s in sorted(a.keys() & b.keys()) if a[s] != b[s]]
    for d in diff:
        print(d)
    kd = sum(s.endswith(".kd") for s in a)
    print(f"{len(a)} symbols ({kd} kernel descriptors) against {len(b)}: {len(diff)} differences")
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
