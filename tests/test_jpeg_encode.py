"""CPU: the baseline JPEG encoder's host-only entry points (cg_image_encode_jpeg_host,
cg_image_jpeg_header, cg_image_jpeg_bound) against the bytes Pillow writes.

Pillow's bytes are the expected output throughout: tests/golden/jpeg_enc_cases.json holds the
SHA-256 and length of Pillow's file per case (tests/golden/make_jpeg_enc_cases.py regenerates it),
and where Pillow imports its live bytes are compared too.  tests/jpeg_enc_ref.py, a numpy
restatement of the contract that shares no code with the library, must give the same files."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import cgamd
import jpeg_enc_ref as ref
import make_jpeg_enc_cases as mk
from cgamd import P

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "jpeg_enc_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
CG_E_INVALID, CG_E_CAPACITY = -1, -5


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _encode_raw(argb, w, h, stride, quality, sub, cap, guard=64):
    """cg_image_encode_jpeg_host into a buffer of cap bytes followed by `guard` bytes of 0xA5:
    (rc, n, the cap bytes, whether the guard is intact)."""
    lib = cgamd.load()
    buf = np.full(cap + guard, 0xA5, np.uint8)
    prm = cgamd.JpegParams(quality, sub)
    n = C.c_size_t(0)
    rc = lib.cg_image_encode_jpeg_host(argb.ctypes.data_as(P), w, h, stride, C.byref(prm), buf.ctypes.data_as(P), cap,
                                       C.byref(n))
    return rc, n.value, buf[:cap].tobytes(), bool((buf[cap:] == 0xA5).all())


def test_case_list_is_the_generator_s():
    names = [mk.case_name(*c) for c in mk.all_cases()]
    assert sorted(names) == sorted(GOLDEN) and len(names) == len(mk.SIZES) * 4 * 6 * 2
    intervals_444 = {(h, w): -(-w // 8) * 3 for (h, w) in mk.SIZES}
    assert intervals_444[(16, 1100)] == 414
    assert -(-88 // 8) == 11 and -(-150 // 16) == 10          # the RST number wraps past 7


@pytest.mark.parametrize("size", list(mk.SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_restatement_and_golden_agree(size):
    h, w = size
    for content in mk.CONTENTS:
        argb = mk.inputs(h, w, content)
        for q in mk.QUALITIES:
            for sub in mk.SUBSAMPLINGS:
                name = mk.case_name(h, w, content, q, sub)
                want = GOLDEN[name]
                got = cgamd.image_encode_jpeg_host(argb, q, sub)
                assert (len(got), _sha(got)) == (want["length"], want["sha256"]), f"host {name}"
                r = ref.encode(argb, q, sub)
                assert (len(r), _sha(r)) == (want["length"], want["sha256"]), f"restatement {name}"
                assert cgamd.image_jpeg_header(w, h, q, sub) == got[:629] == ref.header(w, h, q, sub), name
                assert got[627:629] == b"\x3f\x00" and got[-2:] == b"\xff\xd9"


def test_pillow_live_bytes():
    pytest.importorskip("PIL")
    for h, w, content, q, sub in mk.all_cases():
        argb = mk.inputs(h, w, content)
        data = mk.pillow_bytes(argb, q, sub)
        name = mk.case_name(h, w, content, q, sub)
        assert (len(data), _sha(data)) == (GOLDEN[name]["length"], GOLDEN[name]["sha256"]), f"golden {name}"
        assert cgamd.image_encode_jpeg_host(argb, q, sub) == data, name


def test_alpha_is_ignored():
    argb = mk.inputs(17, 33, "random")
    files = {cgamd.image_encode_jpeg_host((argb & np.uint32(0x00FFFFFF)) | np.uint32(a << 24), 75, 2) for a in (0, 128, 255)}
    assert len(files) == 1 and _sha(files.pop()) == GOLDEN[mk.case_name(17, 33, "random", 75, 2)]["sha256"]


def test_row_stride_is_honoured():
    h, w = 31, 15
    argb = mk.inputs(h, w, "random")
    wide = np.full((h, w + 5), 0x00FF00FF, np.uint32)
    wide[:, :w] = argb
    for sub in (0, 2):
        want = GOLDEN[mk.case_name(h, w, "random", 90, sub)]
        rc, n, data, ok = _encode_raw(wide, w, h, w + 5, 90, sub, 8192)
        assert rc == 0 and ok and (n, _sha(data[:n])) == (want["length"], want["sha256"])
    assert _encode_raw(wide, w, h, w - 1, 90, 0, 8192)[0] == CG_E_INVALID


def test_argument_errors():
    lib = cgamd.load()
    argb = mk.inputs(8, 8, "random")
    for w, h, q, sub in [(0, 8, 75, 0), (8, 0, 75, 0), (-1, 8, 75, 0), (65536, 1, 75, 0), (1, 65536, 75, 0), (8, 8, 0, 0),
                         (8, 8, 101, 0), (8, 8, -5, 2), (8, 8, 75, 1), (8, 8, 75, 3), (8, 8, 75, -1)]:
        assert _encode_raw(argb, w, h, 0, q, sub, 4096)[0] == CG_E_INVALID, (w, h, q, sub)
        prm = cgamd.JpegParams(q, sub)
        buf = np.zeros(1024, np.uint8)
        assert lib.cg_image_jpeg_header(w, h, C.byref(prm), buf.ctypes.data_as(P), 1024) == CG_E_INVALID
        assert not buf.any()
    for w, h, sub in [(0, 8, 0), (8, 0, 2), (65536, 8, 0), (8, 8, 1)]:
        assert lib.cg_image_jpeg_bound(w, h, sub) == CG_E_INVALID
    prm = cgamd.JpegParams(75, 0)
    n = C.c_size_t()
    buf = np.zeros(4096, np.uint8)
    a, b = argb.ctypes.data_as(P), buf.ctypes.data_as(P)
    assert lib.cg_image_encode_jpeg_host(None, 8, 8, 0, C.byref(prm), b, 4096, C.byref(n)) == CG_E_INVALID
    assert lib.cg_image_encode_jpeg_host(a, 8, 8, 0, None, b, 4096, C.byref(n)) == CG_E_INVALID
    assert lib.cg_image_encode_jpeg_host(a, 8, 8, 0, C.byref(prm), None, 4096, C.byref(n)) == CG_E_INVALID
    assert lib.cg_image_encode_jpeg_host(a, 8, 8, 0, C.byref(prm), b, 4096, None) == CG_E_INVALID
    assert lib.cg_image_jpeg_header(8, 8, None, b, 4096) == CG_E_INVALID
    assert lib.cg_image_jpeg_header(8, 8, C.byref(prm), None, 4096) == CG_E_INVALID
    assert lib.cg_image_jpeg_header(8, 8, C.byref(prm), b, 628) == CG_E_CAPACITY and not buf.any()
    assert lib.cg_image_jpeg_header(8, 8, C.byref(prm), b, 629) == 629


def test_capacity_one_byte_short():
    for (h, w, content, q, sub) in [(17, 33, "random", 75, 2), (20, 35, "noise", 100, 2), (1, 1, "constant", 50, 0)]:
        argb = mk.inputs(h, w, content)
        want = GOLDEN[mk.case_name(h, w, content, q, sub)]
        full = cgamd.image_encode_jpeg_host(argb, q, sub)
        rc, n, data, ok = _encode_raw(argb, w, h, 0, q, sub, want["length"])
        assert rc == 0 and ok and n == want["length"] and data == full
        rc, n, data, ok = _encode_raw(argb, w, h, 0, q, sub, want["length"] - 1)
        assert rc == CG_E_CAPACITY and n == want["length"] and ok and data == full[:-1]
        rc, n, data, ok = _encode_raw(argb, w, h, 0, q, sub, 0)      # a length query
        assert rc == CG_E_CAPACITY and n == want["length"] and ok


def test_bound_covers_the_noise_cases():
    for (h, w) in mk.SIZES:
        for sub in (0, 2):
            bound = cgamd.image_jpeg_bound(w, h, sub)
            longest = max(GOLDEN[mk.case_name(h, w, c, 100, sub)]["length"] for c in mk.CONTENTS)
            assert bound >= longest and bound >= GOLDEN[mk.case_name(h, w, "noise", 100, sub)]["length"]
            mcu = 16 if sub else 8
            mx, my = -(-w // mcu), -(-h // mcu)
            per_interval = 2 * -(-(mx * (6 if sub else 3) * 1660) // 8)
            assert bound == 629 + my * per_interval + 2 * (my - 1) + 2


def test_decoder_accepts_every_product():
    lib = cgamd.load()
    for h, w, content, q, sub in mk.all_cases():
        data = cgamd.image_encode_jpeg_host(mk.inputs(h, w, content), q, sub)
        buf = np.frombuffer(data, np.uint8)
        assert lib.cg_image_jpeg_check(buf.ctypes.data_as(P), buf.size) == 0, (h, w, content, q, sub)
        assert cgamd.jpeg_info(data) == (w, h, 3)
