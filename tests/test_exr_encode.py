"""CPU: the EXR encoder's contract.  The host encoder (cg_image_encode_exr_host) and the numpy
restatement (tests/exr_enc_ref.py, part a) against the hashes of tests/golden/exr_enc_cases.json,
which pin files that the independent reader (part b: struct, zlib, numpy) accepts; the reader
again, live, on the host encoder's files; the half rule on its own against numpy's
astype(float16); the header; the bound; strides, capacities and refusals."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import cgamd
import exr_enc_ref as ref
import make_exr_enc_cases as mk

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "exr_enc_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
GROUPS = mk.groups()
P = C.c_void_p
RULE_1_TABLE = {0x7F800001: 0x7C01, 0x7FC00000: 0x7E00, 0x477FEFFF: 0x7BFF, 0x477FF000: 0x7C00, 0x33000000: 0x0000,
                0x33000001: 0x0001, 0x387FC000: 0x03FF, 0x3F801000: 0x3C00, 0x3F803000: 0x3C02}


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _gid(g):
    return mk.case_name(g[0], g[1], "x", *g[2:]).replace("-x-", "-")


def _numpy_half(bits):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(bits, np.uint32).view(np.float32).astype(np.float16).view(np.uint16)


def test_goldens_cover_the_generator():
    assert sorted(GOLDEN) == sorted(mk.case_name(*c) for c in mk.all_cases())


@pytest.mark.parametrize("group", list(GROUPS), ids=_gid)
def test_host_and_reference_match_goldens(group):
    h, w, ch, typ, comp = group
    for content in GROUPS[group]:
        want = GOLDEN[mk.case_name(h, w, content, ch, typ, comp)]
        px, alpha = mk.inputs(h, w, content, typ), mk.alpha_of(content)
        for who, data in (("host", cgamd.image_encode_exr_host(px, ch, typ, comp, alpha)),
                          ("numpy", ref.encode(px, ch, typ, comp, alpha))):
            assert (len(data), _sha(data)) == (want["length"], want["sha256"]), f"{who} {content}"


@pytest.mark.parametrize("group", list(GROUPS), ids=_gid)
def test_independent_reader_returns_the_samples(group):
    """The host encoder's file through the reader: FLOAT bit for bit, HALF numpy's astype(float16)."""
    h, w, ch, typ, comp = group
    for content in GROUPS[group]:
        px, alpha = mk.inputs(h, w, content, typ), mk.alpha_of(content)
        data = cgamd.image_encode_exr_host(px, ch, typ, comp, alpha)
        got = mk.accepted(data, px, ch, typ, comp, alpha)
        assert got["raw_chunks"] == GOLDEN[mk.case_name(h, w, content, ch, typ, comp)]["raw_chunks"], content
        n = cgamd.image_exr_bound(w, h, ch, typ)
        assert len(data) == n if comp == ref.NONE else len(data) <= n, content


def test_special_cases_take_the_paths_they_are_for():
    threads, window = cgamd.image_exr_enc_limits()
    assert (threads, window) == (mk.PIECE, mk.WINDOW)
    assert 16 * 7 * 8 < threads < 16 * 9 * 8                      # 18x7 and 18x9, RGBA half
    _, notes = ref.info(mk.inputs(20, 900, "patch"), alpha_scale=mk.PATCH_ALPHA)
    assert not notes[0]["raw"] and window < notes[0]["bytes"] < 16 * 900 * 8
    assert 16 * 1400 * 16 > 65535
    for typ in (ref.HALF, ref.FLOAT):
        for size in ((1, 1), (33, 7), (40, 65), (20, 900)):
            _, notes = ref.info(mk.inputs(*size, "noise", typ), ref.RGBA, typ)
            assert all(c["raw"] for c in notes), (typ, size)
    _, notes = ref.info(mk.inputs(40, 65, "mixed"))
    assert [c["raw"] for c in notes] == [False, True, False]
    _, notes = ref.info(mk.inputs(1, 1, "constant"))
    assert notes[0]["raw"]


# ---- rule 1 ----
def test_half_rule_table():
    bits = np.array(list(RULE_1_TABLE), np.uint32)
    want = np.array(list(RULE_1_TABLE.values()), np.uint16)
    assert np.array_equal(cgamd.image_exr_half(bits.view(np.float32)), want)
    assert np.array_equal(ref.half_bits(bits), want)
    assert np.array_equal(_numpy_half(bits), want)


def test_half_rule_around_every_finite_half():
    """float(h), the midpoint to its successor and the floats just below and above that midpoint, both signs."""
    h = np.arange(0, 0x7C00, dtype=np.uint16)
    f = h.view(np.float16).astype(np.float32).view(np.uint32).astype(np.int64)
    nxt = np.arange(1, 0x7C01, dtype=np.uint16).view(np.float16).astype(np.float64)
    nxt[-1] = 65536.0                                             # the successor of 65504 as the rounding sees it
    mid = ((h.view(np.float16).astype(np.float64) + nxt) / 2).astype(np.float32)   # exact: one more bit than a half
    mid = mid.view(np.uint32).astype(np.int64)
    pos = np.concatenate([f, mid, mid - 1, mid + 1]).astype(np.uint32)
    bits = np.concatenate([pos, pos | np.uint32(0x80000000)])
    want = _numpy_half(bits)
    assert np.array_equal(cgamd.image_exr_half(bits.view(np.float32)), want)
    assert np.array_equal(ref.half_bits(bits), want)
    # what the sweep is for: a tie goes to the even half, its neighbours to the nearer one
    k = np.arange(h.size)
    got_mid = cgamd.image_exr_half(mid.astype(np.uint32).view(np.float32))
    assert np.array_equal(got_mid, np.where(k % 2 == 0, k, k + 1).astype(np.uint16))


def test_half_rule_on_random_bit_patterns():
    bits = mk.pcg32(1 << 20, 2024).astype(np.uint32)
    want = _numpy_half(bits)
    assert np.array_equal(cgamd.image_exr_half(bits.view(np.float32)), want)
    assert np.array_equal(ref.half_bits(bits), want)
    assert cgamd.image_exr_half(np.zeros(0, np.float32)).size == 0


def test_alpha_scale_one_keeps_the_bits_of_w():
    px = mk.inputs(17, 5, "specials")
    assert np.isnan(px[..., 3]).any()
    data = cgamd.image_encode_exr_host(px, ref.RGBA, ref.FLOAT, ref.NONE, 1.0)
    assert np.array_equal(ref.read(data)["planes"]["A"], np.ascontiguousarray(px[..., 3]).view(np.uint32))
    # another scale is one float32 product
    px = mk.inputs(17, 5, "patch")
    data = cgamd.image_encode_exr_host(px, ref.RGBA, ref.FLOAT, ref.ZIP, 0.3)
    want = np.ascontiguousarray(px[..., 3] * np.float32(0.3)).view(np.uint32)
    assert np.array_equal(ref.read(data)["planes"]["A"], want)


# ---- the header, the bound ----
def test_header_lengths_and_the_contract_s_example():
    for (w, h) in ((1, 1), (1920, 1080), (65535, 65535)):
        for ch, n in ((ref.RGBA, 331), (ref.RGB, 313)):
            for typ in (ref.HALF, ref.FLOAT):
                for comp in (ref.NONE, ref.ZIP):
                    got = cgamd.image_exr_header(w, h, ch, typ, comp)
                    assert len(got) == n and got == ref.header(w, h, ch, typ, comp)
    src = open(os.path.join(os.path.dirname(HERE), "include", "cg_render.h")).read()
    m = re.search(r"A 2 x 1 RGB half ZIP file's header:\n(.*?)\n \* 3 Chunks", src, re.S)
    printed = bytes.fromhex(re.sub(r"[\s*]", "", m.group(1)))
    assert printed == cgamd.image_exr_header(2, 1, ref.RGB, ref.HALF, ref.ZIP)


def test_bound_is_a_none_file_s_length():
    for (h, w) in ((1, 1), (17, 5), (33, 7), (1080, 1920), (65535, 65535)):
        for ch, nch, hdr in ((ref.RGB, 3, 313), (ref.RGBA, 4, 331)):
            for typ, bps in ((ref.HALF, 2), (ref.FLOAT, 4)):
                assert cgamd.image_exr_bound(w, h, ch, typ) == hdr + 16 * h + h * w * nch * bps
    lib = cgamd.load()
    for args in ((0, 1, 4, 1), (1, 65536, 4, 1), (1, 1, 5, 1), (1, 1, 4, 0), (1, 1, 4, 3)):
        assert lib.cg_image_exr_bound(*args) == cgamd.CG_E_INVALID


# ---- strides, capacities, refusals ----
def _host(px, w, h, stride, prm, cap, out=None):
    lib = cgamd.load()
    n = C.c_size_t(12345)
    buf = out if out is not None else np.full(cap + 16, 0xA5, np.uint8)
    rc = lib.cg_image_encode_exr_host(px.ctypes.data_as(P), w, h, stride, C.byref(prm) if prm is not None else None,
                                      buf.ctypes.data_as(P) if cap or out is not None else None, cap, C.byref(n))
    return rc, n.value, buf


def test_row_stride_null_params_and_capacity():
    h, w = 17, 5
    px = mk.inputs(h, w, "patch")
    wide = np.full((h, w + 3, 4), np.float32(7.5))
    wide[:, :w] = px
    wide = np.ascontiguousarray(wide)
    for prm, args in ((None, (ref.RGBA, ref.HALF, ref.ZIP, 1.0)),
                      (cgamd.ExrParams(ref.RGB, ref.FLOAT, ref.ZIP, 1.0), (ref.RGB, ref.FLOAT, ref.ZIP, 1.0)),
                      (cgamd.ExrParams(ref.RGBA, ref.HALF, ref.NONE, 0.5), (ref.RGBA, ref.HALF, ref.NONE, 0.5))):
        want = ref.encode(px, *args)
        rc, n, buf = _host(wide, w, h, w + 3, prm, len(want))
        assert rc == cgamd.CG_OK and n == len(want) and bytes(buf[:n]) == want and (buf[n:] == 0xA5).all()
        rc, n, _ = _host(px, w, h, 0, prm, 0)                              # the length query, out NULL
        assert rc == cgamd.CG_E_CAPACITY and n == len(want)
        for cap in (1, 8, 331, len(want) // 2, len(want) - 1):
            rc, n, buf = _host(px, w, h, 0, prm, cap)
            assert rc == cgamd.CG_E_CAPACITY and n == len(want)
            assert bytes(buf[:cap]) == want[:cap] and (buf[cap:] == 0xA5).all(), cap


def test_refusals():
    px = np.zeros((2, 2, 4), np.float32)
    ok = cgamd.ExrParams(ref.RGBA, ref.HALF, ref.ZIP, 1.0)
    out = np.zeros(4096, np.uint8)
    lib = cgamd.load()
    n = C.c_size_t()
    bad = [cgamd.ExrParams(5, 1, 3, 1.0), cgamd.ExrParams(2, 1, 3, 1.0), cgamd.ExrParams(4, 0, 3, 1.0), cgamd.ExrParams(4, 3, 3, 1.0),
           cgamd.ExrParams(4, 1, 1, 1.0), cgamd.ExrParams(4, 1, 2, 1.0), cgamd.ExrParams(4, 1, 3, float("inf")),
           cgamd.ExrParams(4, 1, 3, float("nan"))]
    for prm in bad:
        assert _host(px, 2, 2, 0, prm, 4096, out)[0] == cgamd.CG_E_INVALID
        assert lib.cg_image_exr_header(2, 2, C.byref(prm), out.ctypes.data_as(P), 4096, C.byref(n)) == cgamd.CG_E_INVALID
    for (w, h, stride) in ((0, 2, 0), (2, 0, 0), (65536, 1, 0), (1, 65536, 0), (2, 2, 1)):
        assert _host(px, w, h, stride, ok, 4096, out)[0] == cgamd.CG_E_INVALID
    o = out.ctypes.data_as(P)
    assert lib.cg_image_encode_exr_host(None, 2, 2, 0, C.byref(ok), o, 4096, C.byref(n)) == cgamd.CG_E_INVALID
    assert lib.cg_image_encode_exr_host(px.ctypes.data_as(P), 2, 2, 0, C.byref(ok), None, 4096, C.byref(n)) == cgamd.CG_E_INVALID
    assert lib.cg_image_encode_exr_host(px.ctypes.data_as(P), 2, 2, 0, C.byref(ok), o, 4096, None) == cgamd.CG_E_INVALID
    assert lib.cg_image_exr_half(None, 4, o) == cgamd.CG_E_INVALID
    assert lib.cg_image_exr_half(px.ctypes.data_as(P), 4, None) == cgamd.CG_E_INVALID
    assert lib.cg_image_exr_half(px.ctypes.data_as(P), -1, o) == cgamd.CG_E_INVALID
    assert lib.cg_image_exr_header(2, 2, None, o, 4, C.byref(n)) == cgamd.CG_E_CAPACITY and n.value == 331
    with pytest.raises(ValueError):
        cgamd.image_encode_exr_host(np.zeros((2, 2, 3), np.float32))


def test_binding_names_the_calls():
    for name, arity in (("cg_image_encode_exr_host", 8), ("cg_image_exr_bound", 4), ("cg_image_exr_header", 6),
                        ("cg_image_exr_half", 3), ("cg_image_exr_enc_limits", 2), ("cg_image_encode_exr_device", 11),
                        ("cg_image_encode_exr", 9)):
        assert name in cgamd.EXPORTS and len(cgamd._SIGS[name][1]) == arity, name
    for name in ("image_encode_exr", "image_encode_exr_device"):
        assert callable(getattr(cgamd.Context, name))
