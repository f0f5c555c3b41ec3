"""CPU: the bloom contract (include/cg_render.h "Bloom", csrc/cg_bloom.h).

* tests/bloom_ref.py, the numpy restatement, and cg_hdr_bloom against three answers written out as
  literals;
* cg_hdr_bloom_layout against the size rule for every size 1..70 and levels 1..6;
* cg_hdr_bloom / cg_hdr_bloom_pack against the restatement on bit patterns over the contract's size
  list, on pixels of every kind (random bit patterns, NaN, +-inf, negatives, -0, denormals, every
  coverage value), scales that include 0, negative, +inf and NaN, both rules, every tone curve;
* intensity == 0 is the pack without bloom;
* every refusal; the header declares every new entry point and cgamd binds each with its arity.
No compute call needs a GPU here."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import bloom_ref as bref
import cgamd
import hdr_ref
from cgamd import P
from test_hdr_gpu import _pixels

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CG_E_INVALID = -1

NEW_ENTRY_POINTS = {          # name: number of parameters in include/cg_render.h
    "cg_hdr_bloom_layout": 7, "cg_hdr_bloom": 6, "cg_hdr_bloom_pack": 10, "cg_hdr_bloom_device": 11,
    "cg_hdr_bloom_pack_device": 16, "cg_rt_render_exposed_bloom_device": 15, "cg_rt_render_exposed_bloom": 15,
    "cg_rast_draw_exposed_bloom_device": 13, "cg_rast_draw_exposed_bloom": 13,
}

# (threshold, cap, intensity): the defaults, the largest values the contract admits, a cap below the threshold
PARAMS = [(1.0, 64.0, 0.25), (0.0, 2.0 ** 64, 2.0 ** 32), (0.5, 0.5, 1.5)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frame_of_bright(b):
    """A frame float32[H, W, 4] whose bright pass at scale 1, threshold 0 is the plane b (H x W, >= 0)."""
    b = np.asarray(b, np.float32)
    return np.stack([b, b, b, np.ones_like(b)], axis=2)


def _levels_of(pyr, W, H, levels):
    """The stored pyramid float32[total, 4] as planes [h, w, 4]."""
    ws, hs, off, total = bref.layout(W, H, levels)
    assert pyr.shape == (total, 4)
    return [pyr[o:o + w * h].reshape(h, w, 4) for w, h, o in zip(ws, hs, off)]


# ---- the three hand pins ------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(16, 16), (1, 1), (7, 5), (33, 17), (64, 3)])
@pytest.mark.parametrize("levels", [1, 3, 6])
def test_constant_bright_plane_counts_the_levels(W, H, levels):
    """A bright plane of 1.0 everywhere: U_k == levels - k + 1 exactly, odd sizes included."""
    U = bref.pyramid_of_bright(np.ones((H, W, 3), np.float32), levels)
    frame = _frame_of_bright(np.ones((H, W), np.float32))
    lib = _levels_of(cgamd.hdr_bloom(frame, 1.0, levels=levels, threshold=0.0, cap=64.0, intensity=0.0), W, H, levels)
    for k in range(1, levels + 1):
        want = F(levels - k + 1)
        assert (U[k - 1] == want).all(), k
        assert (lib[k - 1][..., :3] == want).all(), k
        assert (_bits(lib[k - 1][..., 3]) == 0).all()


def test_block_of_four_bright_pixels_is_the_binomial_kernel():
    b = np.zeros((16, 16), np.float32)
    b[8:10, 8:10] = 4.0
    k = np.array([1, 4, 6, 4, 1], np.float32) / F(16)
    want = np.zeros((8, 8), np.float32)
    want[2:7, 2:7] = F(4) * np.outer(k, k)
    assert want[4, 4] == F(0.5625) and want.sum() == F(4.0)
    U1 = bref.pyramid_of_bright(np.repeat(b[..., None], 3, axis=2), 1)[0]
    lib = _levels_of(cgamd.hdr_bloom(_frame_of_bright(b), 1.0, levels=1, threshold=0.0, cap=64.0, intensity=0.0), 16, 16, 1)[0]
    for c in range(3):
        assert np.array_equal(_bits(U1[..., c]), _bits(want)), c
        assert np.array_equal(_bits(lib[..., c]), _bits(want)), c


def test_single_bright_pixel_known_answers():
    b = np.zeros((16, 16), np.float32)
    b[8, 8] = 4.0
    for levels, want in ((1, F(0.140625)), (2, F(0.17016602))):
        U1 = bref.pyramid_of_bright(np.repeat(b[..., None], 3, axis=2), levels)[0]
        lib = _levels_of(cgamd.hdr_bloom(_frame_of_bright(b), 1.0, levels=levels, threshold=0.0, cap=64.0, intensity=0.0),
                         16, 16, levels)[0]
        assert U1[4, 4, 0] == want and U1[4, 4, 2] == want, (levels, U1[4, 4])
        assert lib[4, 4, 0] == want and lib[4, 4, 1] == want, (levels, lib[4, 4])


def test_bright_pass_by_hand():
    """NaN and negatives give 0, +inf gives cap, an uncovered pixel is dark, the scale multiplies before the threshold."""
    px = np.array([[[2.0, np.nan, -3.0, 1.0], [np.inf, 0.5, -0.0, 1.0], [9.0, 9.0, 9.0, 0.0], [9.0, 9.0, 9.0, np.nan],
                    [3.0, 1.5, 1000.0, 2.0]]], np.float32)
    got = bref.bright(px, 2.0, 1.0, 64.0)[0]
    want = np.array([[3.0, 0.0, 0.0], [64.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [5.0, 2.0, 64.0]], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(bref.bright(px, np.nan, 1.0, 64.0)), _bits(np.zeros((1, 5, 3), np.float32)))
    assert np.array_equal(_bits(bref.bright(px, np.inf, 1.0, 64.0)[0, 0]), _bits(np.array([64.0, 0.0, 0.0], np.float32)))
    # the library: a 4 x 4 frame of one pixel has B_1 == b everywhere, and the blur of a constant plane of
    # these values is exact ((2b / 16 + 2b / 4) + 3b / 8 == b), so a one-level pyramid shows b itself
    for i in range(5):
        frame = np.tile(px[0, i], (4, 4, 1))
        for s, row in ((2.0, want[i]), (np.nan, np.zeros(3, np.float32)),
                       (np.inf, np.array([64.0, 0.0, 0.0], np.float32) if i == 0 else None)):
            if row is None:
                continue
            pyr = cgamd.hdr_bloom(frame, s, levels=1, threshold=1.0, cap=64.0, intensity=0.0)
            assert pyr.shape == (4, 4) and np.array_equal(_bits(pyr[:, :3]), _bits(np.tile(row, (4, 1)))), (i, s, pyr)


# ---- layout -------------------------------------------------------------------------------------

def test_layout_follows_the_size_rule():
    for levels in range(1, 7):
        for W, H in itertools.product(range(1, 71), range(1, 71)):
            ws, hs, off, total = [], [], [], 0
            w, h = W, H
            for _ in range(levels):
                w, h = (w + 1) // 2, (h + 1) // 2
                ws.append(w), hs.append(h), off.append(total)
                total += w * h
            assert cgamd.hdr_bloom_layout(W, H, levels) == (ws, hs, off, total), (W, H, levels)
    assert cgamd.hdr_bloom_layout(1, 1, 6) == ([1] * 6, [1] * 6, list(range(6)), 6)
    assert bref.layout(1920, 1080, 4) == cgamd.hdr_bloom_layout(1920, 1080, 4)
    lib = cgamd.load()
    assert lib.cg_hdr_bloom_layout(33, 17, 3, None, None, None, None) == 3          # any pointer may be NULL
    for W, H, levels in ((0, 4, 1), (4, 0, 1), (-1, 4, 1), (4, 4, 0), (4, 4, 7), (4, 4, -1)):
        assert lib.cg_hdr_bloom_layout(W, H, levels, None, None, None, None) == CG_E_INVALID, (W, H, levels)
        with pytest.raises(ValueError):
            cgamd.hdr_bloom_layout(W, H, levels)


# ---- the host functions against the restatement -------------------------------------------------

def _frame(rng, W, H):
    px = _pixels(rng, W * H, 4).reshape(H, W, 4)
    if W * H >= 4:
        px.reshape(-1, 4)[rng.integers(0, W * H)] = (3.0, 7.0, 1.5, 1.0)      # one ordinary bright pixel at least
    return px


@pytest.mark.parametrize("W,H", bref.SIZES, ids=[f"{w}x{h}" for w, h in bref.SIZES])
def test_host_functions_match_the_restatement(W, H):
    rng = np.random.default_rng(1000 * W + H)
    frame = _frame(rng, W, H)
    combos = itertools.cycle(itertools.product((bref.RULE_RT, bref.RULE_RAST),
                                               (hdr_ref.TONE_LINEAR, hdr_ref.TONE_REINHARD, hdr_ref.TONE_REINHARD_WHITE)))
    n = 0
    for levels in (1, 2, 6):
        for i, s in enumerate(bref.SCALES):
            thr, cap, inten = PARAMS[(i + levels) % len(PARAMS)]
            rule, op = next(combos)
            bloom = cgamd.hdr_bloom_params(levels, thr, cap, inten)
            want_pyr, want_px = bref.frame(frame, s, levels, thr, cap, inten, rule, op, 7.5)
            got_pyr = cgamd.hdr_bloom(frame, s, bloom)
            bad = np.flatnonzero(_bits(got_pyr) != _bits(want_pyr))
            assert bad.size == 0, (levels, s, bad[:4], got_pyr.flat[bad[0]], want_pyr.flat[bad[0]])
            assert np.isfinite(got_pyr).all()
            got_px = cgamd.hdr_bloom_pack(frame, got_pyr, s, bloom, rule, op, 7.5)
            bad = np.flatnonzero(got_px.ravel() != want_px.ravel())
            assert bad.size == 0, (levels, s, rule, op, bad[:4], hex(got_px.flat[bad[0]]), hex(want_px.flat[bad[0]]))
            n += int((want_pyr > 0).any())
    assert n >= 9 or W * H < 4                                                 # not a comparison of zeros


def test_every_rule_and_curve_on_one_frame():
    rng = np.random.default_rng(77)
    W, H = 33, 17
    frame = _frame(rng, W, H)
    frame[2:6, 3:9, :3] = rng.random((4, 6, 3), np.float32) * F(6.0)
    frame[2:6, 3:9, 3] = 1.0
    for (thr, cap, inten), s in zip(PARAMS, (1.0, 0.37, 5.5)):
        bloom = cgamd.hdr_bloom_params(3, thr, cap, inten)
        pyr = cgamd.hdr_bloom(frame, s, bloom)
        U = bref.pyramid(frame, s, 3, thr, cap)
        assert np.array_equal(_bits(pyr), _bits(bref.stored(U))) and (U[0] > 0).any()
        seen = set()
        for rule in (bref.RULE_RT, bref.RULE_RAST):
            for op in (hdr_ref.TONE_LINEAR, hdr_ref.TONE_REINHARD, hdr_ref.TONE_REINHARD_WHITE):
                got = cgamd.hdr_bloom_pack(frame, pyr, s, bloom, rule, op, 4.0)
                assert np.array_equal(got, bref.composite(frame, U[0], s, inten, rule, op, 4.0)), (rule, op)
                seen.add(got.tobytes())
        assert len(seen) == 6 or inten != 0.25            # the default parameters tell every rule and curve apart
        # rule RAST leaves the uncovered pixels 0; rule RT packs them
        unc = ~(frame[..., 3] > 0)
        assert unc.any() and (cgamd.hdr_bloom_pack(frame, pyr, s, bloom, bref.RULE_RAST)[unc] == 0).all()
        assert (cgamd.hdr_bloom_pack(frame, pyr, s, bloom, bref.RULE_RT)[unc] != 0).all()


def test_only_level_one_of_the_pyramid_is_read_by_the_pack():
    rng = np.random.default_rng(5)
    frame = _frame(rng, 33, 17)
    bloom = cgamd.hdr_bloom_params(4)
    pyr = cgamd.hdr_bloom(frame, 1.0, bloom)
    n1 = 17 * 9
    other = pyr.copy()
    other[n1:] = np.nan
    assert np.array_equal(cgamd.hdr_bloom_pack(frame, other, 1.0, bloom), cgamd.hdr_bloom_pack(frame, pyr, 1.0, bloom))


@pytest.mark.parametrize("op", [hdr_ref.TONE_LINEAR, hdr_ref.TONE_REINHARD, hdr_ref.TONE_REINHARD_WHITE])
def test_zero_intensity_is_the_pack_without_bloom(op):
    rng = np.random.default_rng(40 + op)
    W, H = 65, 63
    frame = _frame(rng, W, H)
    for s in (1.0, 0.37, 0.0, -2.0, np.inf, np.nan):
        bloom = cgamd.hdr_bloom_params(3, 0.0, 64.0, 0.0)
        pyr = cgamd.hdr_bloom(frame, s, bloom)
        rt = cgamd.hdr_bloom_pack(frame, pyr, s, bloom, bref.RULE_RT, op, 7.5)
        assert np.array_equal(rt, hdr_ref.pack(frame, s, op, 7.5)), s
        rast = cgamd.hdr_bloom_pack(frame, pyr, s, bloom, bref.RULE_RAST, op, 7.5)
        assert np.array_equal(rast, cgamd.rast_pack_pixel(frame, s, op, 7.5)), s


# ---- refusals and the interface -----------------------------------------------------------------

BAD_PARAMS = [dict(levels=0), dict(levels=7), dict(levels=-1), dict(threshold=-1.0), dict(threshold=float("nan")),
              dict(cap=0.0), dict(cap=-1.0), dict(cap=float("nan")), dict(cap=2.0 ** 65), dict(cap=float("inf")),
              dict(intensity=-0.5), dict(intensity=float("nan")), dict(intensity=2.0 ** 33), dict(intensity=float("inf"))]


def test_refusals():
    lib = cgamd.load()
    W, H = 5, 4
    frame = np.ones((H, W, 4), np.float32)
    pyr = np.zeros((64, 4), np.float32)
    out = np.zeros((H, W), np.uint32)

    def bloom(rgba=frame, w=W, h=H, pyr_=pyr, params=True, **kw):
        p = cgamd.hdr_bloom_params(**kw)
        return lib.cg_hdr_bloom(rgba.ctypes.data_as(P) if rgba is not None else None, w, h, 1.0,
                                C.byref(p) if params else None, pyr_.ctypes.data_as(P) if pyr_ is not None else None)

    def pack(rgba=frame, pyr_=pyr, w=W, h=H, rule=0, op=0, white2=1.0, argb=out, params=True, **kw):
        p = cgamd.hdr_bloom_params(**kw)
        return lib.cg_hdr_bloom_pack(rgba.ctypes.data_as(P) if rgba is not None else None,
                                     pyr_.ctypes.data_as(P) if pyr_ is not None else None, w, h, 1.0,
                                     C.byref(p) if params else None, rule, op, white2,
                                     argb.ctypes.data_as(P) if argb is not None else None)
    for call in (bloom, pack):
        assert call() == 0
        assert call(cap=2.0 ** 64, intensity=2.0 ** 32, threshold=0.0, levels=6) == 0      # the limits themselves
        assert call(threshold=float("inf")) == 0
        for kw in BAD_PARAMS:
            assert call(**kw) == CG_E_INVALID, kw
        assert call(rgba=None) == CG_E_INVALID and call(pyr_=None) == CG_E_INVALID and call(params=False) == CG_E_INVALID
        assert call(w=0) == CG_E_INVALID and call(h=0) == CG_E_INVALID and call(w=-3) == CG_E_INVALID
    assert pack(argb=None) == CG_E_INVALID
    assert pack(rule=2) == CG_E_INVALID and pack(rule=-1) == CG_E_INVALID
    assert pack(op=3) == CG_E_INVALID and pack(op=-1) == CG_E_INVALID
    assert pack(op=2, white2=0.0) == CG_E_INVALID and pack(op=2, white2=float("nan")) == CG_E_INVALID
    assert pack(op=1, white2=0.0) == 0
    with pytest.raises(ValueError):
        cgamd.hdr_bloom(frame, 1.0, levels=7)
    with pytest.raises(ValueError):
        cgamd.hdr_bloom_pack(frame, pyr, 1.0, rule=5)


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
    assert C.sizeof(cgamd.HdrBloomParams) == 16
    src = open(os.path.join(ROOT, "include", "cg_render.h")).read()
    for macro, value in (("CG_BLOOM_MAX_LEVELS", cgamd.BLOOM_MAX_LEVELS), ("CG_BLOOM_RULE_RT", cgamd.BLOOM_RULE_RT),
                         ("CG_BLOOM_RULE_RAST", cgamd.BLOOM_RULE_RAST)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    p = cgamd.hdr_bloom_params()
    assert (p.levels, p.threshold, p.cap, p.intensity) == (4, 1.0, 64.0, 0.25)
    for method in ("hdr_bloom_device", "hdr_bloom_pack_device", "rt_render_exposed_bloom_device",
                   "rt_render_exposed_bloom", "rast_draw_exposed_bloom_device", "rast_draw_exposed_bloom"):
        assert callable(getattr(cgamd.Context, method)), method
    for fn in ("hdr_bloom_layout", "hdr_bloom", "hdr_bloom_pack"):
        assert callable(getattr(cgamd, fn)), fn


def test_default_bloom_changes_the_cornell_box():
    """The reference scene saturates under its light of colour 14: with the default parameters
    (threshold 1.0) the oracle's own float frame has bright pixels, and the composite differs from
    the frame without bloom -- glow on the pixels around them, the background included."""
    import rt_radiance_ref as rref
    rad = rref.reference("id_1")
    p = cgamd.hdr_bloom_params()
    U = bref.pyramid(rad, 1.0, p.levels, p.threshold, p.cap)
    assert (U[0] > 0).any()
    plain = hdr_ref.pack(rad, 1.0)
    for rule in (bref.RULE_RT, bref.RULE_RAST):
        got = bref.composite(rad, U[0], 1.0, p.intensity, rule, hdr_ref.TONE_LINEAR)
        assert (got != plain).any()
        assert np.array_equal(got, cgamd.hdr_bloom_pack(rad, cgamd.hdr_bloom(rad, 1.0, p), 1.0, p, rule))
    spill = (plain == 0x80000000) & (bref.composite(rad, U[0], 1.0, p.intensity, bref.RULE_RT, hdr_ref.TONE_LINEAR) != 0x80000000)
    print(f"pixels changed: {(got != plain).sum()} of {plain.size}; background pixels lit by the glow: {spill.sum()}")
