"""CPU: the frame-sequence C-ABI (cg_rast_draw_sequence_device and its two
companions) is declared in the header, bound with the same layout, and
exported by the library where it is built."""
import ctypes as C
import os
import re

import cgamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cg_rast_draw_sequence_device", "cg_rast_set_rand_capacity", "cg_glibc_rand_device")
CTYPES = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32}


def _header():
    return open(os.path.join(ROOT, "include", "cg_render.h")).read()


def _header_struct():
    """[(field, ctype)] of cg_rast_seq_frame as the header declares it"""
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*cg_rast_seq_frame\s*;", _header())
    assert m, "cg_rast_seq_frame not declared"
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), CTYPES[ty]) for n in names.split(",")]
    return fields


def test_header_declares_sequence_api():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    m = re.search(r"cg_rast_draw_sequence_device\s*\(([^)]*)\)", src)
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[7] == "cg_rast_seq_frame *d_info" and args[8] == "void *stream"
    fields = _header_struct()
    assert [f for f, _ in fields] == ["rand_offset", "n_shaded", "status", "pad"]

    class Hdr(C.Structure):
        _fields_ = fields
    assert C.sizeof(Hdr) == 24


def test_binding_struct_matches_header():
    class Hdr(C.Structure):
        _fields_ = _header_struct()
    assert C.sizeof(cgamd.RastSeqFrame) == C.sizeof(Hdr) == 24
    for name, ty in _header_struct():
        got, want = getattr(cgamd.RastSeqFrame, name), getattr(Hdr, name)
        assert (got.offset, got.size) == (want.offset, want.size), name
    assert (cgamd.RastSeqFrame.rand_offset.offset, cgamd.RastSeqFrame.n_shaded.offset,
            cgamd.RastSeqFrame.status.offset, cgamd.RastSeqFrame.pad.offset) == (0, 8, 16, 20)
    for name in NAMES:
        assert name in cgamd.EXPORTS
    for meth in ("rast_draw_sequence_device", "rast_set_rand_capacity", "glibc_rand_device"):
        assert callable(getattr(cgamd.Context, meth))


def test_library_exports_sequence_symbols():
    if not os.path.exists(cgamd.LIB_PATH):
        return   # not built here: the header and the binding are checked above
    lib = cgamd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.cg_rast_set_rand_capacity(None, 0) == cgamd.CG_E_INVALID   # argument check only: no device touched
