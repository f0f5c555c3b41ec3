"""r_magnitude (raytracer/Source/skeleton.cpp:371) as the one-light lattice kernels form it
(light_rmag_inrange, cg_rt_dev.h): the compiler's FP64 square root written out without its range
scaling, which never acts on a sum of three squared floats.  cg_rt_probe_rmag_device runs it on
float triples; the reference is numpy, float32(sqrt((r0 + r1) + r2)) with r_k the float64 square of
component k -- IEEE operations, one rounding each, as the reference program's C++ performs them.
Equality is bit for bit.  A NaN result must be a NaN: which payload survives an operation on two
NaNs is not defined by IEEE 754, numpy's host and the GPU differ there, and no frame holds one.

Inputs: 2^20 triples of random float bit patterns (every exponent, either sign, denormals,
infinities and NaNs among them), random triples inside the room's range, and the edge cases listed
in _edge_cases(): zeros of both signs, denormals, FLT_MAX, infinities, NaN, and triples whose
float64 sum lies next to the square of a float rounding midpoint.  The harness is first checked on
the CPU alone: numpy's reference against Python's math.sqrt and an exact rational test of the
rounding."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import cgamd

FLT_MAX = float(np.finfo(np.float32).max)
DENORM_MIN = float(np.float32(2.0 ** -149))
N_RANDOM = 1 << 20


def _reference(r):
    """float32(sqrt(float64 sum)) of float32 triples r[n, 3]."""
    with np.errstate(all="ignore"):
        d = r.astype(np.float64)
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def _midpoint_triples(rng, n):
    """Triples whose float64 sum of squares is within a few ulps (of float64) of m * m, m the midpoint
    of two neighbouring floats: the root is next to a rounding boundary of the final narrowing.  The
    components are taken greedily, each the float root of what is left."""
    f = rng.uniform(0.01, 8.0, n).astype(np.float32)
    m = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2.0
    left = m * m
    out = np.zeros((n, 3), np.float32)
    out[:, 0] = np.sqrt(left * rng.uniform(0.2, 0.9, n)).astype(np.float32)
    left = left - out[:, 0].astype(np.float64) ** 2
    out[:, 1] = np.nextafter(np.sqrt(left).astype(np.float32), np.float32(0.0))   # not above what is left
    left = np.maximum(left - out[:, 1].astype(np.float64) ** 2, 0.0)
    out[:, 2] = np.sqrt(left).astype(np.float32)
    return out


def _edge_cases():
    z, nz, inf, nan = 0.0, -0.0, float("inf"), float("nan")
    dn, dbig = DENORM_MIN, float(np.float32(2.0 ** -127))
    rows = [
        (z, z, z), (nz, nz, nz), (z, nz, z), (nz, z, nz),
        (dn, z, z), (z, dn, z), (z, z, dn), (dn, dn, dn), (-dn, dn, nz), (dbig, dbig, dbig),
        (float(np.float32(2.0 ** -126)), z, z), (dn, 1.0, z), (dn, z, FLT_MAX),
        (FLT_MAX, z, z), (FLT_MAX, FLT_MAX, FLT_MAX), (-FLT_MAX, FLT_MAX, -FLT_MAX), (FLT_MAX, 1.0, dn),
        (inf, z, z), (-inf, 1.0, 2.0), (inf, inf, inf), (inf, -inf, z), (FLT_MAX, inf, dn),
        (nan, z, z), (z, nan, z), (1.0, 2.0, nan), (nan, nan, nan), (inf, nan, z), (nan, -inf, FLT_MAX),
        (3.0, 4.0, z), (1.0, 2.0, 2.0), (2.0, 3.0, 6.0), (1.0, 1.0, 1.0), (0.5, -0.5, 0.7),
    ]
    return np.array(rows, np.float32)


_INPUTS = {}


def _inputs():
    """All triples, built once: random bit patterns, the room's range, midpoints, edge cases."""
    if "r" not in _INPUTS:
        rng = np.random.default_rng(0x726D6167)
        bits = rng.integers(0, 1 << 32, (N_RANDOM, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
        room = rng.uniform(-2.0, 2.0, (1 << 16, 3)).astype(np.float32)
        r = np.ascontiguousarray(np.concatenate([bits, room, _midpoint_triples(rng, 1 << 14), _edge_cases()]))
        r.setflags(write=False)
        _INPUTS["r"] = r
        _INPUTS["ref"] = _reference(r)
        _INPUTS["ref"].setflags(write=False)
    return _INPUTS["r"], _INPUTS["ref"]


def _same_bits(got, ref, r, what):
    """got == ref bit for bit; where ref is a NaN, got must be a NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    nan = np.isnan(ref)
    bad = np.flatnonzero(np.where(nan, ~np.isnan(got), got.view(np.uint32) != ref.view(np.uint32)))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(ref)} differ; first at {bad[:4]}: inputs "
                           f"{[r[i].tolist() for i in bad[:4]]}, got {got[bad[:4]].view(np.uint32)}, "
                           f"reference {ref[bad[:4]].view(np.uint32)}")


def _f32(x):
    """A Python float rounded to float32 by the C library (struct), without numpy."""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(float("inf"), x)


def test_rmag_harness_on_the_cpu():
    """numpy alone passes the harness: on the edge cases, the midpoint triples and a sample of the
    random ones its reference equals math.sqrt narrowed by struct, bit for bit, and math.sqrt's
    float64 root s is the correctly rounded one, shown with rationals: (s - ulp/2)^2 <= x <=
    (s + ulp/2)^2 (the float is that root narrowed, two roundings as in the reference program).
    The inputs hold what the module's docstring lists."""
    r, ref = _inputs()
    assert np.isnan(ref).sum() > 1000 and np.isinf(ref).sum() > 20 and (ref == 0).sum() >= 4
    with np.errstate(all="ignore"):
        d = r.astype(np.float64)
        x = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert (x[np.isfinite(x) & (x > 0)] >= 2.0 ** -298).all()    # the range argument of the comment
    assert np.signbit(x[x == 0]).sum() == 0                        # never -0
    pick = np.concatenate([np.arange(0, N_RANDOM, 97), np.arange(N_RANDOM, len(r))])
    alone = np.array([_f32(math.sqrt(v)) if v == v and v >= 0 else float("nan") for v in x[pick].tolist()], np.float32)
    _same_bits(ref[pick], alone, r[pick], "numpy against math.sqrt")
    _same_bits(alone, ref[pick], r[pick], "math.sqrt against numpy")
    near = 0
    for i in pick[-(len(_edge_cases()) + (1 << 14)):][::8]:
        if not (math.isfinite(x[i]) and x[i] > 0):
            continue
        s = math.sqrt(float(x[i]))
        S, X = Fraction(s), Fraction(float(x[i]))
        lo, hi = (S + Fraction(math.nextafter(s, 0.0))) / 2, (S + Fraction(math.nextafter(s, math.inf))) / 2
        assert lo * lo <= X <= hi * hi, (r[i].tolist(), s)
        g = _f32(s)
        if math.isfinite(g) and g < FLT_MAX:           # s against the midpoints beside its float
            for other in (float(np.nextafter(np.float32(g), np.float32(0))), float(np.nextafter(np.float32(g), np.float32(np.inf)))):
                if math.isfinite(other) and abs(S - (Fraction(g) + Fraction(other)) / 2) < S * Fraction(1, 1 << 44):
                    near += 1
    assert near > 100, f"only {near} roots next to a float rounding midpoint"


@pytest.mark.gpu
def test_rmag_probe_matches_float64_sqrt(ctx):
    """light_rmag_inrange on every triple == float32(sqrt(float64 sum)), bit for bit."""
    import torch
    r, ref = _inputs()
    n = len(r)
    dr = torch.from_numpy(np.array(r)).cuda()
    dm = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    cgamd.probe_rmag_device(dr.data_ptr(), n, dm.data_ptr())
    torch.cuda.synchronize()
    _same_bits(dm.cpu().numpy(), ref, r, "cg_rt_probe_rmag_device")


@pytest.mark.gpu
def test_rmag_probe_arguments(ctx):
    """n = 0 is a no-op; a missing array and a negative count are refused."""
    lib = cgamd.load()
    assert lib.cg_rt_probe_rmag_device(None, 0, None, None) == cgamd.CG_OK
    assert lib.cg_rt_probe_rmag_device(None, 4, None, None) != cgamd.CG_OK
    assert lib.cg_rt_probe_rmag_device(None, -1, None, None) != cgamd.CG_OK
