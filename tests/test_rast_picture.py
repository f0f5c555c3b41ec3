"""CPU: the rasteriser's float picture and pack (include/cg_render.h, csrc/cg_hdr.h).

* tests/rast_picture_ref.py's self-checks, which tie the restated picture to the oracle: the lit
  frame has no marks and the full frame's low, high and depth planes; the lit screen minus the
  restated darkening is the full screen on every marked pixel; PutPixelSDL of the picture is the
  oracle's frame inside, and that frame is 0 on the border.  Cases: the reference scene at 96x64
  in colour modes 0, 1 and 2, and at 67x45 with indirect_first 0.15 and a moved camera;
* the header declares every new entry point and cgamd binds each with the right arity;
* cg_rast_pack_pixel against the restated pack on random bit patterns and hand values, all three
  curves;
* the argument errors that need no device.
No compute call needs a GPU here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cgamd
import hdr_ref
import oracle
import rast_picture_ref as pref
from cgamd import P

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CG_E_INVALID = -1

NEW_ENTRY_POINTS = {          # name: number of parameters in include/cg_render.h
    "cg_rast_draw_picture_device": 6, "cg_rast_draw_picture": 4, "cg_rast_draw_sequence_picture_device": 9,
    "cg_rast_tonemap_pack_device": 11, "cg_rast_pack_pixel": 4, "cg_rast_draw_exposed_device": 12,
    "cg_rast_draw_exposed": 12,
}

CASES = {
    "96x64-mode0": dict(width=96, height=64, colour_mode=0),
    "96x64-mode1": dict(width=96, height=64, colour_mode=1, rand_offset=12_000_000),
    "96x64-mode2": dict(width=96, height=64, colour_mode=2, rand_offset=12_000_000),
    "67x45-indirect-camera": dict(width=67, height=45, indirect_first=0.15, cam=(0.2, -0.1, -2.6, 1.0)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_restated_picture_agrees_with_the_oracle(name):
    kw = dict(CASES[name])
    p = oracle.rast_params(kw.pop("width"), kw.pop("height"), **kw)
    rgba, full, checks = pref.picture(p)
    print(name, checks)
    assert checks["marked"] > 100, checks              # the darkening is exercised
    assert pref.clean(checks), checks
    H, W = p.height, p.width
    assert rgba.shape == (H, W, 4)
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    assert (rgba[inner][:, 3] == 1.0).all()
    assert not hdr_ref.bits(rgba[~inner]).any()         # +0 four times
    if p.colour_mode == 0:   # what a clamped 8-bit frame loses: channels above 1 and below 0 are both present
        assert (rgba[..., :3] > 1.0).any() and (rgba[..., :3] < 0.0).any()
    _, rec = hdr_ref.stats_of(rgba.reshape(-1, 4))
    assert rec["n_uncovered"] == 2 * W + 2 * H - 4


def test_darkening_counts_the_lower_left_mark_twice():
    s = np.zeros((5, 5), np.int32)
    s[2, 2] = 1
    assert pref.darkening(s)[2, 2] == F(0.05)           # 1 / 9
    s[3, 3] = 1                                         # [y+1][x+1] is never read
    assert pref.darkening(s)[2, 2] == F(0.05)
    s[3, 1] = 1                                         # [y+1][x-1] twice: 3 / 9
    assert pref.darkening(s)[2, 2] == F(0.05)
    s[1, 1] = s[1, 2] = s[1, 3] = 1                     # 6 / 9 = 0.667 -> 0.08
    assert pref.darkening(s)[2, 2] == F(0.08)
    s[2, 1] = 1                                         # 7 / 9 = 0.778 -> 0.1
    assert pref.darkening(s)[2, 2] == F(0.1)
    s[2, 3] = 1                                         # 8 / 9 = 0.889 -> 0.12
    assert pref.darkening(s)[2, 2] == F(0.12)
    s[3, 2] = 1                                         # 9 / 9 -> 0.3
    assert pref.darkening(s)[2, 2] == F(0.3)
    assert pref.darkening(s)[0].tolist() == [0.0] * 5   # the border is never darkened


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
    assert cgamd._SIGS["cg_rast_pack_pixel"][0] is C.c_uint32
    for method in ("rast_draw_picture", "rast_draw_picture_device", "rast_draw_sequence_picture_device",
                   "rast_tonemap_pack_device", "rast_draw_exposed_device", "rast_draw_exposed"):
        assert callable(getattr(cgamd.Context, method)), method
    assert callable(cgamd.rast_pack_pixel)


# ---- cg_rast_pack_pixel --------------------------------------------------------------------------

HAND = [-0.0, 0.0, np.nan, -1.0, -2.0, np.inf, -np.inf, 0.5, 1.0, 2.55, 1e-45]
HAND_W = [0.0, -0.0, np.nan, 1.0, -1.0, np.inf, 9.0, 1e-45]


def _pack_inputs():
    rng = np.random.default_rng(0x9A57)
    n = 20_000
    px = hdr_ref.random_floats(rng, 4 * n).reshape(n, 4)
    px[: n // 2, 3] = rng.choice(np.array(HAND_W, np.float32), n // 2)       # half with a w that decides
    hand = np.array([[a, b, c, w] for a in HAND for b in (0.25, a) for c in (-1.0, 3.0) for w in HAND_W], np.float32)
    return np.concatenate([px, hand])


@pytest.mark.parametrize("op,white2", [(hdr_ref.TONE_LINEAR, 1.0), (hdr_ref.TONE_REINHARD, 1.0),
                                       (hdr_ref.TONE_REINHARD_WHITE, 7.5)])
def test_c_pack_pixel_equals_the_restatement(op, white2):
    px = _pack_inputs()
    for scale in (1.0, 0.37, 1000.0, 2.0 ** -16):
        got = cgamd.rast_pack_pixel(px, scale, op, white2)
        c = px[:, :3]
        with np.errstate(all="ignore"):
            want = hdr_ref.pack(np.where(c > 0, c, F(0.0)).astype(np.float32), scale, op, white2)
            want = np.where(px[:, 3] > 0, want, np.uint32(0)).astype(np.uint32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"op {op} scale {scale}: {bad.size} differ, first {px[bad[0]]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"
        assert np.array_equal(want, pref.pack(px, scale, op, white2))


def test_pack_pixel_rules_by_hand():
    pk = lambda *px, **kw: int(cgamd.rast_pack_pixel(np.array(px, np.float32), **kw))
    assert pk(1.0, 1.0, 1.0, 0.0) == 0                          # border rule: not 0x80000000
    assert pk(1.0, 1.0, 1.0, np.nan) == 0 and pk(1.0, 1.0, 1.0, -1.0) == 0
    assert pk(0.0, 0.0, 0.0, 1.0) == 0x80000000
    assert pk(2.55, 0.5, -0.3, 1.0) == 0x80FF7F00               # LINEAR at 1: PutPixelSDL's clamp
    assert pk(np.nan, -np.inf, np.inf, 1.0) == 0x800000FF
    # clamp rule: Reinhard's pole at -1 is never reached, a darkened pixel stays black under a large scale
    assert pk(-0.001, -0.001, -0.001, 1.0, scale=999.0, op=hdr_ref.TONE_REINHARD) == 0x80000000
    assert pk(-2.0, -1.0, -0.5, 1.0, scale=1.0, op=hdr_ref.TONE_REINHARD) == 0x80000000
    assert pk(1.0, 3.0, 0.0, 1.0, op=hdr_ref.TONE_REINHARD) == 0x807FBF00          # 1/2, 3/4
    assert cgamd.load().cg_rast_pack_pixel(None, 1.0, 0, 1.0) == 0


# ---- argument errors that need no device ---------------------------------------------------------

def test_entry_points_refuse_a_null_context():
    lib = cgamd.load()
    p = cgamd.rast_params(32, 24)
    ex = cgamd.hdr_params()
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(P)
    assert lib.cg_rast_draw_picture_device(None, C.byref(p), ptr, None, None, None) == CG_E_INVALID
    assert lib.cg_rast_draw_picture(None, C.byref(p), ptr, None) == CG_E_INVALID
    assert lib.cg_rast_draw_sequence_picture_device(None, C.byref(p), 1, ptr, None, None, 0, ptr, None) == CG_E_INVALID
    assert lib.cg_rast_tonemap_pack_device(None, ptr, 4, 1, 0, ptr, 0, 1.0, ptr, 0, None) == CG_E_INVALID
    assert lib.cg_rast_draw_exposed_device(None, C.byref(p), 1, C.byref(ex), None, 0, 1.0, ptr, 0, ptr, ptr,
                                           None) == CG_E_INVALID
    assert lib.cg_rast_draw_exposed(None, C.byref(p), 1, C.byref(ex), None, 0, 1.0, ptr, 0, ptr, None,
                                    None) == CG_E_INVALID
    with pytest.raises(ValueError):
        cgamd.rast_pack_pixel(np.zeros((2, 3), np.float32))
