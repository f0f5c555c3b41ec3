"""CPU: cg_rast_draw_sequence is declared, bound and exported with the documented argument
types; a NULL context is CG_E_INVALID (nothing is dereferenced); and the binding's own argument
checks (the C entry has no capacity argument, so short destinations are refused in Python)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cgamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p


def test_header_declares_the_documented_arguments():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cg_render.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cg_rast_draw_sequence\s*\(([^)]*)\)", src)
    assert m, "cg_rast_draw_sequence not declared"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == [
        "cg_ctx *ctx", "const cg_rast_params *ps", "int n_frames", "uint32_t *argb", "float *depth",
        "int32_t *shadow", "size_t frame_stride", "int chunk", "cg_rast_seq_frame *info", "cg_stats *stats"]


def test_binding_matches_the_header():
    assert cgamd._SIGS["cg_rast_draw_sequence"] == (
        C.c_int, [P, C.POINTER(cgamd.RastParams), C.c_int, P, P, P, C.c_size_t, C.c_int,
                  C.POINTER(cgamd.RastSeqFrame), C.POINTER(cgamd.Stats)])
    assert "cg_rast_draw_sequence" in cgamd.EXPORTS and callable(cgamd.Context.rast_draw_sequence)
    assert cgamd.RAST_SEQ_DTYPE.itemsize == C.sizeof(cgamd.RastSeqFrame) == 24
    for name, (_, ctype) in zip(cgamd.RAST_SEQ_DTYPE.names, cgamd.RastSeqFrame._fields_):
        assert cgamd.RAST_SEQ_DTYPE.fields[name][1] == getattr(cgamd.RastSeqFrame, name).offset
        assert cgamd.RAST_SEQ_DTYPE.fields[name][0].itemsize == C.sizeof(ctype)


def test_library_exports_the_symbol_and_refuses_a_null_context():
    lib = cgamd.load()
    assert hasattr(lib, "cg_rast_draw_sequence")
    ps = (cgamd.RastParams * 2)(cgamd.rast_params(64, 48, 40.0), cgamd.rast_params(64, 48, 40.0))
    out = np.zeros(2 * 64 * 48, np.uint32)
    info = (cgamd.RastSeqFrame * 3)()
    st = cgamd.Stats()
    assert lib.cg_rast_draw_sequence(None, ps, 2, out.ctypes.data_as(P), None, None, 0, 0, info, C.byref(st)) \
        == cgamd.CG_E_INVALID
    assert lib.cg_rast_draw_sequence(None, ps, 0, None, None, None, 0, 0, None, None) == cgamd.CG_E_INVALID
    assert not out.any()


def test_binding_argument_checks():
    W, H = 64, 48
    npx = W * H
    ps = [cgamd.rast_params(W, H, 40.0, colour_mode=k % 3) for k in range(3)]
    planes = cgamd.rast_sequence_planes
    stride, a, d, s = planes(ps)
    assert stride == npx and a.dtype == np.uint32 and a.size == 3 * npx and d is None and s is None
    stride, a, d, s = planes(ps, want_depth=True, want_shadow=True, frame_stride=npx + 7)
    assert stride == npx + 7 and d.dtype == np.float32 and s.dtype == np.int32
    assert a.size == d.size == s.size == 3 * (npx + 7)
    exact = np.zeros(2 * (npx + 7) + npx, np.uint32)          # the last frame needs no gap after it
    assert planes(ps, out=exact, frame_stride=npx + 7)[1] is exact
    dep = np.zeros(3 * npx, np.float32)
    assert planes(ps, want_depth=dep)[2] is dep
    for bad in (dict(chunk=65), dict(chunk=-1), dict(frame_stride=npx - 1),
                dict(out=np.zeros(3 * npx - 1, np.uint32)),                 # one pixel short
                dict(out=np.zeros(3 * npx, np.uint32), frame_stride=npx + 1),
                dict(want_depth=np.zeros(3 * npx - 1, np.float32)),
                dict(want_shadow=np.zeros(3 * npx, np.int16)),              # 2-byte elements
                dict(out=np.zeros((3 * npx, 2), np.uint32)[:, 0])):         # not contiguous
        with pytest.raises(ValueError):
            planes(ps, **bad)
    with pytest.raises(ValueError):
        planes(ps[:2] + [cgamd.rast_params(W, H + 1, 40.0)])
    assert planes([], out=np.zeros(4, np.uint32))[0] == 0 and planes([])[1].size == 0
