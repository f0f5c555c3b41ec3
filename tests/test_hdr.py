"""CPU: the exposure chain's definitions (include/cg_render.h, csrc/cg_hdr.h).

* tests/hdr_ref.py, the numpy restatement, against answers written out as literals;
* the library's host-only helpers (cg_hdr_luminance, cg_hdr_bin, cg_hdr_bin_edge, cg_hdr_exposure,
  cg_hdr_tone) against the restatement on bit patterns: the literals and 100,000 random patterns;
* the header declares every new entry point and cgamd binds each with the right arity;
* cg_hdr_exposure's CG_E_INVALID returns.
No compute call needs a GPU here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cgamd
import hdr_ref as ref
from cgamd import P

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CG_E_INVALID = -1

NEW_ENTRY_POINTS = {          # name: number of parameters in include/cg_render.h
    "cg_hdr_luminance": 3, "cg_hdr_bin": 1, "cg_hdr_bin_edge": 1, "cg_hdr_exposure": 5, "cg_hdr_tone": 3,
    "cg_hdr_histogram_device": 9, "cg_hdr_exposure_device": 7, "cg_rt_tonemap_pack_device": 11,
    "cg_rt_render_exposed_device": 14, "cg_rt_render_exposed": 14,
}


def _same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:4]}: {got.flat[bad[0]]!r} != {want.flat[bad[0]]!r}"


# ---- the restatement, by hand ------------------------------------------------------------------

def test_bins_known_answers():
    b = lambda v: int(ref.bin_of(F(v)).reshape(-1)[0])
    assert b(1.0) == 128
    assert b(0.5) == 120
    assert b(np.nextafter(F(1), F(0))) == 127
    assert b(2.0 ** -16) == 0
    assert b(1e-30) == 0
    assert b(1e-45) == 0                      # a denormal
    assert b(65536.0) == 255
    assert b(np.inf) == 255
    assert b(61440.0) == 255 and b(np.nextafter(F(61440.0), F(0))) == 254     # bin 255 starts at 2^15 * 15/8
    assert b(0.0) == b(-0.0) == b(-1.0) == b(np.nan) == b(-np.inf) == -1
    assert b(2.0) == 136 and b(1.125) == 129 and b(np.nextafter(F(1.125), F(0))) == 128   # eight bins an octave


def test_edges_known_answers():
    assert float(ref.bin_edge(127)) == 1.0
    assert float(ref.bin_edge(255)) == 65536.0
    assert float(ref.bin_edge(0)) == 2.0 ** -16 * 1.125
    assert float(ref.bin_edge(128)) == 1.125
    for k in range(ref.BINS - 1):             # the upper edge of a bin is the first value of the next
        e = ref.bin_edge(k)
        assert ref.bin_of(e).item() == k + 1 and ref.bin_of(np.nextafter(e, F(0))).item() == k


def test_luminance_known_answers():
    # in exact arithmetic on the three float32 constants, rounding after each add: exactly 1.0f
    assert ref.luminance(1, 1, 1).view(np.uint32) == 0x3F800000
    assert float(ref.luminance(0, 0, 0)) == 0.0
    # the association is (a + b) + c: with a = -b the sum is c exactly, while a + (b + c) is not
    big = F(3.0e7)
    x, y = big / F(0.2126), -big / F(0.7152)
    a, b_, c = F(0.2126) * x, F(0.7152) * y, F(0.0722) * F(1)
    assert float(ref.luminance(x, y, 1)) == float(F(F(a + b_) + c))
    assert float(F(F(a + b_) + c)) != float(F(a + F(b_ + c)))


HAND = {   # name: (bin the running sum reaches k in, or None for an empty histogram)
    "empty": None, "one_bin": 128, "permille_0": 10, "permille_1": 10, "permille_500": 100, "permille_1000": 200,
    "sum_equals_k_at_boundary": 60, "one_past_boundary": 70, "huge_counts": 255,
}
EDGE = {10: 2.0 ** -15 * 1.375, 100: 0.1015625, 200: 576.0, 60: 0.003173828125, 70: 0.00732421875, 128: 1.125,
        255: 65536.0}


def test_hand_histograms():
    cases = ref.hand_histograms()
    assert {c[0] for c in cases} == set(HAND)
    for name, hist, permille in cases:
        want = F(1.0) if HAND[name] is None else F(F(3.0) / F(EDGE[HAND[name]]))
        got = ref.target_scale(hist, permille, 3.0, 2.0 ** -30, 2.0 ** 30)
        assert got.view(np.uint32) == want.view(np.uint32), name
    # the clamp
    assert float(ref.target_scale(cases[1][1], 990, 3.0, 2.0 ** -30, 2.0)) == 2.0
    assert float(ref.target_scale(cases[1][1], 990, 3.0, 4.0, 8.0)) == 4.0
    assert float(ref.target_scale(cases[0][1], 990, 3.0, 4.0, 8.0)) == 4.0     # empty: 1.0f before the clamp


def _one_bin(b, n=7):
    h = np.zeros(ref.BINS, np.uint32)
    h[b] = n
    return h


def test_adaptation_chain_by_hand():
    # t = 1 / edge: bins 127, 135, 119 have edges 1, 2, 0.5, so t = 1, 0.5, 2
    hists = np.stack([_one_bin(127), _one_bin(135), _one_bin(119)])
    kw = dict(permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16)
    assert ref.exposure(hists, rate=1.0, **kw).tolist() == [1.0, 0.5, 2.0]
    # s1 = 1 + (0.5 - 1) * 0.25 = 0.875; s2 = 0.875 + (2 - 0.875) * 0.25 = 1.15625
    assert ref.exposure(hists, rate=0.25, **kw).tolist() == [1.0, 0.875, 1.15625]
    # a previous scale is frame 0's: s0 = 4; s1 = 4 + (0.5 - 4) * 0.25 = 3.125; s2 = 3.125 + (2 - 3.125) * 0.25
    assert ref.exposure(hists, rate=0.25, prev=4.0, **kw).tolist() == [4.0, 3.125, 2.84375]
    assert ref.exposure(hists, rate=0.0, **kw).tolist() == [1.0, 1.0, 1.0]
    # chunks: the first frame of a later chunk repeats the scale before it
    assert ref.exposure_chunked(hists, rate=0.25, chunk=2, **kw).tolist() == [1.0, 0.875, 0.875]


def test_tone_and_put_pixel_by_hand():
    v = np.array([0.0, 1.0, 3.0, np.inf, -1.0, np.nan], np.float32)
    assert ref.tone(ref.TONE_LINEAR, v).tolist()[:5] == [0.0, 1.0, 3.0, np.inf, -1.0]
    r = ref.tone(ref.TONE_REINHARD, v)
    assert r[:3].tolist() == [0.0, 0.5, 0.75] and np.isnan(r[3]) and np.isinf(r[4]) and np.isnan(r[5])
    w = ref.tone(ref.TONE_REINHARD_WHITE, v, 4.0)        # (v * (1 + v / 4)) / (1 + v)
    assert w[:3].tolist() == [0.0, 0.625, 1.3125]
    assert ref.chan8(np.array([0.0, 1.0, 0.5, 2.0, -1.0, np.nan, np.inf, -np.inf, 0.999], np.float32)).tolist() == \
        [0, 255, 127, 255, 0, 0, 255, 0, 254]
    assert int(ref.put_pixels(np.array([1.0, 0.5, 0.0], np.float32))) == 0x80FF7F00


def test_frame_record_by_hand():
    px = np.array([[1, 1, 1, 9], [0, 0, 0, 1], [5, 5, 5, 0], [2, 2, 2, -0.0], [0.5, 0.5, 0.5, np.nan],
                   [np.nan, 0, 0, 1], [-1, 0, 0, 3], [0.25, 0.25, 0.25, 1]], np.float32)
    hist, rec = ref.stats_of(px)
    assert rec == dict(n_counted=2, n_dark=3, n_uncovered=3, max_bits=0x3F800000, min_bits=0x3E800000)
    assert hist[128] == 1 and hist[112] == 1 and hist.sum() == 2
    hist3, rec3 = ref.stats_of(px[:, :3])
    assert rec3["n_uncovered"] == 0 and rec3["n_counted"] == 5 and rec3["n_dark"] == 3
    assert ref.stats_of(px[1:2])[1] == dict(n_counted=0, n_dark=1, n_uncovered=0, max_bits=0, min_bits=0xFFFFFFFF)


# ---- the library's host helpers against the restatement ----------------------------------------

def _patterns():
    rng = np.random.default_rng(0x4D8)
    return np.concatenate([ref.special_luminances(), ref.random_floats(rng, 100_000)])


def test_c_bin_and_edge_equal_the_restatement():
    L = _patterns()
    assert np.array_equal(cgamd.hdr_bin(L), ref.bin_of(L))
    assert set(np.unique(ref.bin_of(L)).tolist()) == set(range(-1, 256))      # every bin was drawn
    b = np.arange(ref.BINS)
    _same_bits(cgamd.hdr_bin_edge(b), ref.bin_edge(b), "edge")
    lib = cgamd.load()
    assert lib.cg_hdr_bin_edge(-1) == 0.0 and lib.cg_hdr_bin_edge(256) == 0.0
    with pytest.raises(ValueError):
        cgamd.hdr_bin_edge([256])


def test_c_luminance_equals_the_restatement():
    rng = np.random.default_rng(0x4D9)
    n = 100_000
    xyz = ref.random_floats(rng, 3 * n).reshape(n, 3)
    sp = ref.special_luminances()
    xyz = np.concatenate([xyz, np.stack([sp, np.roll(sp, 1), np.roll(sp, 2)], axis=1),
                          np.ones((1, 3), np.float32)])
    got, want = cgamd.hdr_luminance(xyz[:, 0], xyz[:, 1], xyz[:, 2]), ref.luminance(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)            # a NaN's payload is not part of the definition
    _same_bits(got[~nan], want[~nan], "luminance")
    assert nan.sum() < n // 50 and np.isfinite(want).sum() > n // 2


@pytest.mark.parametrize("op", [ref.TONE_LINEAR, ref.TONE_REINHARD, ref.TONE_REINHARD_WHITE])
def test_c_tone_equals_the_restatement(op):
    v = _patterns()
    for white2 in (1.0, 7.5):
        got, want = cgamd.hdr_tone(op, v, white2), ref.tone(op, v, white2)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        _same_bits(got[~nan], want[~nan], f"tone {op}")


def test_c_exposure_equals_the_restatement():
    for hists, kw, prev in ref.exposure_cases():
        got = cgamd.hdr_exposure(hists, prev=prev, **kw)
        _same_bits(got, ref.exposure(hists, prev=prev, **kw), f"{kw} prev {prev}")
    hists = np.stack([_one_bin(127), _one_bin(135), _one_bin(119)])
    assert cgamd.hdr_exposure(hists, rate=0.25).tolist() == [1.0, 0.875, 1.15625]
    assert cgamd.hdr_exposure(hists, rate=0.25, prev=4.0).tolist() == [4.0, 3.125, 2.84375]


def test_c_exposure_refuses_bad_parameters():
    lib = cgamd.load()
    hist = np.zeros((2, ref.BINS), np.uint32)
    out = np.zeros(2, np.float32)

    def rc(n=2, h=hist, o=out, params=True, **kw):
        p = cgamd.hdr_params(**kw)
        return lib.cg_hdr_exposure(h.ctypes.data_as(P) if h is not None else None, n, C.byref(p) if params else None,
                                   None, o.ctypes.data_as(P) if o is not None else None)
    assert rc() == 0
    assert rc(n=0, h=None, o=None) == 0
    assert rc(permille=-1) == CG_E_INVALID
    assert rc(permille=1001) == CG_E_INVALID
    assert rc(rate=-0.001) == CG_E_INVALID
    assert rc(rate=1.001) == CG_E_INVALID
    assert rc(rate=float("nan")) == CG_E_INVALID
    assert rc(scale_min=2.0, scale_max=1.0) == CG_E_INVALID
    assert rc(scale_min=1.0, scale_max=1.0) == 0
    assert rc(h=None) == CG_E_INVALID
    assert rc(o=None) == CG_E_INVALID
    assert rc(params=False) == CG_E_INVALID
    assert rc(n=-1) == CG_E_INVALID
    with pytest.raises(ValueError):
        cgamd.hdr_exposure(hist, permille=2000)


# ---- the interface ------------------------------------------------------------------------------

def _declarations():
    src = open(os.path.join(ROOT, "include", "cg_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src)}


def test_header_declares_and_cgamd_binds_every_new_entry_point():
    decl = _declarations()
    lib = cgamd.load()
    for name, arity in NEW_ENTRY_POINTS.items():
        assert name in decl, name
        assert len(decl[name].split(",")) == arity, (name, decl[name])
        assert hasattr(lib, name), name
        assert name in cgamd.EXPORTS and len(cgamd._SIGS[name][1]) == arity, name
    assert C.sizeof(cgamd.HdrStats) == 32 and cgamd.HDR_STATS_DTYPE.itemsize == 32
    assert C.sizeof(cgamd.HdrExposureParams) == 20
    src = open(os.path.join(ROOT, "include", "cg_render.h")).read()
    for macro, value in (("CG_HDR_BINS", 256), ("CG_TONE_LINEAR", cgamd.TONE_LINEAR), ("CG_TONE_REINHARD", cgamd.TONE_REINHARD),
                         ("CG_TONE_REINHARD_WHITE", cgamd.TONE_REINHARD_WHITE)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    for method in ("hdr_histogram_device", "hdr_exposure_device", "rt_tonemap_pack_device", "rt_render_exposed_device",
                   "rt_render_exposed"):
        assert callable(getattr(cgamd.Context, method)), method
    assert "2^32" in src[src.index("} cg_hdr_stats;") - 900:src.index("} cg_hdr_stats;")]
