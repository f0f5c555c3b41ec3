"""CPU: the interface of cg_rt_set_scene_device and the scene grid's sizing rule (cg_rt_grid_dims),
checked against the formula of rt_grid_build restated here in numpy float64."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cgamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


def _header():
    with open(os.path.join(ROOT, "include", "cg_render.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


@pytest.mark.parametrize("proto", [
    "int cg_rt_set_scene_device(cg_ctx *ctx, const cg_tri *d_tris, int n_tris, const cg_sphere *spheres , "
    "int n_spheres, void *stream);",
    "int cg_rt_set_grid_caps(cg_ctx *ctx, long long entries, long long candidates);",
    "int cg_rt_grid_dims(const float vmin[3], const float vmax[3], int n_tris, float lo[3], float *h, "
    "float *inv_h, int res[3]);",
    "int cg_rt_grid_get(cg_ctx *ctx, int res[3], float lo[3], float *h, int *start, size_t start_cap, "
    "int *tris, size_t tris_cap, size_t *n_start, size_t *n_entries);",
    "int cg_rt_grid_info(cg_ctx *ctx, uint64_t out[4]);",
])
def test_header_declares(proto):
    assert proto in _header()


def test_symbols_and_bindings():
    lib = cgamd.load()
    P = C.c_void_p
    want = {
        "cg_rt_set_scene_device": [P, P, C.c_int, C.POINTER(cgamd.Sphere), C.c_int, P],
        "cg_rt_set_grid_caps": [P, C.c_longlong, C.c_longlong],
        "cg_rt_grid_info": [P, C.POINTER(C.c_uint64)],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    for name in ("cg_rt_grid_dims", "cg_rt_grid_get"):
        assert name in cgamd.EXPORTS and getattr(lib, name).restype is C.c_int
    for meth in ("rt_set_scene_device", "rt_grid", "rt_grid_info", "rt_set_grid_caps"):
        assert callable(getattr(cgamd.Context, meth))
    assert callable(cgamd.rt_grid_dims)
    assert C.sizeof(cgamd.Tri) == 76


def _ref_dims(vmin, vmax, n):
    """rt_grid_build's sizing: cubic cells for ~1/4 triangle centroid each, at most 512 an axis."""
    lo = np.minimum(FLT_MAX, np.asarray(vmin, np.float32))
    hi = np.maximum(-FLT_MAX, np.asarray(vmax, np.float32))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        return None
    lo = (lo - np.float32(1e-4)).astype(np.float32)
    hi = (hi + np.float32(1e-4)).astype(np.float32)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    vol = 1.0
    for a in range(3):
        vol *= float(ext[a])
    cbrt = math.cbrt if hasattr(math, "cbrt") else (lambda x: float(np.cbrt(np.float64(x))))
    h = 0.5 * cbrt(vol / max(1.0, n / 2.0))
    for a in range(3):
        h = max(h, float(ext[a]) / 512.0)
    res = [max(1, min(512, int(math.ceil(float(ext[a]) / h)))) for a in range(3)]
    return dict(lo=lo, h=np.float32(h), inv_h=np.float32(1.0 / h), res=np.array(res, np.int32)), h, ext


def _same(got, ref):
    assert got is not None
    assert got["lo"].tobytes() == ref["lo"].tobytes()
    assert np.float32(got["h"]).tobytes() == ref["h"].tobytes()
    assert np.float32(got["inv_h"]).tobytes() == ref["inv_h"].tobytes()
    assert got["res"].tolist() == ref["res"].tolist()


def test_grid_dims_million_triangle_scene():
    n = 1_000_000
    a = np.frombuffer(bytes(cgamd.random_scene(n, 0x5EED)), np.float32).reshape(n, 19)
    v = a[:, :12].reshape(n * 3, 4)[:, :3]
    vmin, vmax = v.min(axis=0), v.max(axis=0)
    ref, h, _ = _ref_dims(vmin, vmax, n)
    _same(cgamd.rt_grid_dims(vmin, vmax, n), ref)
    assert (ref["res"] > 100).all() and (ref["res"] <= 512).all()
    assert 3_000_000 < int(np.prod(ref["res"].astype(np.int64))) < 6_000_000     # ~4 cells a triangle


def test_grid_dims_flat_scene():
    vmin, vmax, n = (-1.0, -1.0, 0.5), (1.0, 1.0, 0.5), 300
    ref, h, ext = _ref_dims(vmin, vmax, n)
    got = cgamd.rt_grid_dims(vmin, vmax, n)
    _same(got, ref)
    assert got["res"][2] == 1
    assert h >= ext.max() / 512.0 and (got["res"][:2] > 1).all()


def test_grid_dims_elongated_scene_clamps_at_512():
    vmin, vmax, n = (0.0, 0.0, 0.0), (1000.0, 1e-3, 1e-3), 100_000
    ref, h, ext = _ref_dims(vmin, vmax, n)
    got = cgamd.rt_grid_dims(vmin, vmax, n)
    _same(got, ref)
    assert got["res"].tolist() == [512, 1, 1]
    assert h == ext[0] / 512.0


@pytest.mark.parametrize("vmin,vmax", [((-np.inf, -1, -1), (1, 1, 1)), ((-1, -1, -1), (1, np.inf, 1)),
                                       ((-np.inf,) * 3, (np.inf,) * 3)])
def test_grid_dims_infinite_bounds_give_no_grid(vmin, vmax):
    assert _ref_dims(vmin, vmax, 100) is None
    assert cgamd.rt_grid_dims(vmin, vmax, 100) is None
    assert cgamd.rt_grid_dims((-1, -1, -1), (1, 1, 1), 100) is not None
    assert cgamd.rt_grid_dims((-1, -1, -1), (1, 1, 1), 0) is None
