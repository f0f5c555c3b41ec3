"""CPU: the PNG encoder's contract.  The host encoder (cg_image_encode_png_host) and the numpy
restatement (tests/png_enc_ref.py) against the hashes of tests/golden/png_enc_cases.json, which
pin files that zlib and Pillow accept; the decoders again, live; the code-length rule and its
limiter on their own; the bound; strides, capacities and refusals; and the files' size against
zlib's run-length strategy on the two golden screenshots.

    python tests/test_png_encode.py        # measure the size check and rewrite profiles/png_enc_size.json
"""
import ctypes as C
import hashlib
import io
import json
import lzma
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    for _p in ("computer-graphics_amd", os.path.join("tests", "golden"), "tests"):
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), _p))

import cgamd  # noqa: E402
import make_png_enc_cases as mk  # noqa: E402
import png_enc_ref as ref  # noqa: E402

with open(os.path.join(HERE, "golden", "png_enc_cases.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
GROUPS = mk.groups()
P = C.c_void_p


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _gid(g):
    return f"{g[0]}x{g[1]}-c{g[2]}-f{'a' if g[3] < 0 else g[3]}"


def _want(argb, colour):
    return argb if colour == ref.RGBA else argb | np.uint32(0xFF000000)


def test_goldens_cover_the_generator():
    assert sorted(GOLDEN) == sorted(mk.case_name(*c) for c in mk.all_cases())


@pytest.mark.parametrize("group", list(GROUPS), ids=_gid)
def test_host_and_reference_match_goldens(group):
    h, w, colour, filt = group
    for content in GROUPS[group]:
        want = GOLDEN[mk.case_name(h, w, content, colour, filt)]
        argb = mk.inputs(h, w, content, colour)
        for who, data in (("host", cgamd.image_encode_png_host(argb, colour, filt)), ("numpy", ref.encode(argb, colour, filt))):
            assert (len(data), _sha(data)) == (want["length"], want["sha256"]), f"{who} {content}"


@pytest.mark.parametrize("group", [g for g in GROUPS if g[0] * g[1] <= 40 * 65 or g[3] == 0], ids=_gid)
def test_independent_decoders_return_the_pixels(group):
    """The host encoder's file through the test's chunk walk, zlib.decompress and numpy un-filtering."""
    h, w, colour, filt = group
    for content in GROUPS[group]:
        argb = mk.inputs(h, w, content, colour)
        assert np.array_equal(ref.decode(cgamd.image_encode_png_host(argb, colour, filt)), _want(argb, colour)), content


def test_pillow_returns_the_pixels():
    Image = pytest.importorskip("PIL.Image")
    for group in [g for g in GROUPS if g[:2] in ((1, 1), (17, 5), (40, 65), (17, 1400))]:
        h, w, colour, filt = group
        for content in GROUPS[group]:
            argb = mk.inputs(h, w, content, colour)
            im = Image.open(io.BytesIO(cgamd.image_encode_png_host(argb, colour, filt)))
            assert im.mode == ("RGBA" if colour == ref.RGBA else "RGB")
            px = np.asarray(im.convert("RGBA")).astype(np.uint32)
            got = (px[..., 3] << 24) | (px[..., 0] << 16) | (px[..., 1] << 8) | px[..., 2]
            assert np.array_equal(got, _want(argb, colour)), (group, content)


def test_special_cases_take_the_paths_they_are_for():
    for colour in mk.COLOURS:
        h, w = mk.FIB_SIZE
        _, bands = ref.info(mk.inputs(h, w, "fib", colour), colour, 0)
        assert bands[0]["depth"] > 15 and not bands[0]["stored"]
        _, bands = ref.info(mk.inputs(h, w, "noise", colour), colour, ref.ADAPTIVE)
        assert all(b["stored"] for b in bands) and bands[0]["bytes"] > 65535
        sym, _, _ = ref.tokens(ref.filtered(mk.inputs(h, w, "runs", colour), colour, 0)[0])
        lens = sorted(set(int(s) for s in sym[sym > 256]))
        # run n -> a literal and: 4: 3; 5: 4; 258: 257; 259: 258; 260: 258 + 1 literal; 261: 258 + 2 literals;
        # 262: 258, 3; 517: 258, 258
        assert lens == [257, 258, 284, 285], lens
        _, window = cgamd.image_png_enc_limits()
        _, bands = ref.info(mk.inputs(20, 900, "nibble", colour), colour, ref.ADAPTIVE)
        assert not bands[0]["stored"] and bands[0]["dyn_bits"] > 8 * window


# ---- the code-length rule ----
def _kraft(lengths):
    return sum(2.0 ** -int(ln) for ln in lengths if ln)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


@pytest.mark.parametrize("name,freq,limit", [
    ("fibonacci 30 at 15", _fib(30), 15),
    ("fibonacci 19 at 7", _fib(19), 7),
    ("fibonacci 40 among zeros at 15", [0, 0] + _fib(40) + [0] * 5, 15),
    ("fibonacci 19 reversed at 7", _fib(19)[::-1], 7),
    ("two symbols", [0, 5, 0, 0, 9], 15),
    ("two symbols at 7", [7, 7], 7),
    ("all equal 286", [3] * 286, 15),
    ("all equal 19", [1] * 19, 7),
    ("all equal 128 at 7", [2] * 128, 7),
    ("steps", [1] * 100 + [50] * 100 + [5000] * 86, 15),
])
def test_code_lengths(name, freq, limit):
    got = cgamd.image_png_code_lengths(freq, limit)
    want = ref.code_lengths(freq, limit)
    assert list(got) == want, name
    assert max(got) <= limit
    assert _kraft(got) == 1.0, name               # powers of two down to 2^-15: exact in a double
    assert all((ln > 0) == (f > 0) for ln, f in zip(got, freq))
    if "fibonacci" in name:
        deep = []
        ref.code_lengths(freq, limit, deep)
        assert deep[0] > limit, "the case must run the limiter"


def test_code_lengths_one_symbol_and_refusals():
    assert list(cgamd.image_png_code_lengths([0, 0, 4], 15)) == [0, 0, 1]
    assert list(cgamd.image_png_code_lengths([0, 0, 0], 15)) == [0, 0, 0]
    lib = cgamd.load()
    f = np.ones(300, np.uint32)
    out = np.zeros(300, np.uint8)
    for n, limit in ((0, 15), (287, 15), (10, 0), (10, 16), (9, 3)):      # 9 symbols do not fit 3 bits
        assert lib.cg_image_png_code_lengths(f.ctypes.data_as(P), n, limit, out.ctypes.data_as(P)) == cgamd.CG_E_INVALID
    assert lib.cg_image_png_code_lengths(None, 4, 15, out.ctypes.data_as(P)) == cgamd.CG_E_INVALID
    assert lib.cg_image_png_code_lengths(f.ctypes.data_as(P), 4, 15, None) == cgamd.CG_E_INVALID
    big = np.full(4, 0x80000000, np.uint32)                               # the sum passes 2^32
    assert lib.cg_image_png_code_lengths(big.ctypes.data_as(P), 4, 15, out.ctypes.data_as(P)) == cgamd.CG_E_INVALID


# ---- the bound ----
def test_bound_holds_and_noise_reaches_it():
    """Every case is within the bound; a frame of noise, all of whose bands are stored, is exactly
    as long (slack 0: the bound is the stored form)."""
    for name, c in GOLDEN.items():
        bound = cgamd.image_png_bound(c["w"], c["h"], c["colour"])
        assert c["length"] <= bound, name
        if c["content"] == "noise":
            assert c["length"] == bound, name
    for (w, h, colour) in ((1, 1, 2), (65535, 65535, 6), (1920, 1080, 2)):
        bpp = 4 if colour == 6 else 3
        bands = [min(16, h - k) * (1 + w * bpp) for k in range(0, h, 16)]
        want = 8 + 25 + 12 + 2 + 4 + sum(12 + n + 5 * -(-n // 65535) for n in bands) + 5 * (len(bands) - 1)
        assert cgamd.image_png_bound(w, h, colour) == want
    lib = cgamd.load()
    for args in ((0, 1, 2), (1, 65536, 2), (4, 4, 3), (4, 4, 0)):
        assert lib.cg_image_png_bound(*args) == cgamd.CG_E_INVALID


# ---- strides, capacities, refusals ----
def _call(argb, w, h, stride, colour, filt, cap, out=None):
    lib = cgamd.load()
    prm = cgamd.PngParams(colour, filt)
    n = C.c_size_t(12345)
    buf = np.full(cap + 64, 0xA5, np.uint8) if out is None else out
    rc = lib.cg_image_encode_png_host(argb.ctypes.data_as(P), w, h, stride, C.byref(prm), buf.ctypes.data_as(P), cap, C.byref(n))
    return rc, n.value, buf


def test_row_stride():
    h, w = 17, 5
    for colour in mk.COLOURS:
        argb = mk.inputs(h, w, "patch", colour)
        wide = np.full((h, w + 9), 0x12345678, np.uint32)
        wide[:, :w] = argb
        want = GOLDEN[mk.case_name(h, w, "patch", colour, ref.ADAPTIVE)]
        rc, n, buf = _call(wide, w, h, w + 9, colour, ref.ADAPTIVE, 4096)
        assert rc == cgamd.CG_OK and n == want["length"] and _sha(buf[:n]) == want["sha256"]
        assert (buf[n:] == 0xA5).all()


def test_capacity():
    h, w = 33, 7
    argb = mk.inputs(h, w, "patch", ref.RGB)
    full = cgamd.image_encode_png_host(argb, ref.RGB, ref.ADAPTIVE)
    for cap in (len(full) - 1, len(full) // 2, 8, 0):
        rc, n, buf = _call(argb, w, h, 0, ref.RGB, ref.ADAPTIVE, cap)
        assert rc == cgamd.CG_E_CAPACITY and n == len(full)
        assert bytes(buf[:cap]) == full[:cap] and (buf[cap:] == 0xA5).all(), cap
    lib = cgamd.load()
    prm = cgamd.PngParams(ref.RGB, ref.ADAPTIVE)
    n = C.c_size_t()
    assert lib.cg_image_encode_png_host(argb.ctypes.data_as(P), w, h, 0, C.byref(prm), None, 0, C.byref(n)) == cgamd.CG_E_CAPACITY
    assert n.value == len(full)
    rc, n2, buf = _call(argb, w, h, 0, ref.RGB, ref.ADAPTIVE, len(full))
    assert rc == cgamd.CG_OK and bytes(buf[:n2]) == full


def test_refusals():
    lib = cgamd.load()
    a = np.zeros((8, 8), np.uint32)
    out = np.zeros(4096, np.uint8)
    n = C.c_size_t()
    ok = dict(argb=a.ctypes.data_as(P), w=8, h=8, stride=0, colour=2, filt=-1, out=out.ctypes.data_as(P), cap=4096, n=C.byref(n))
    for kw in (dict(w=0), dict(w=65536), dict(h=0), dict(h=65536), dict(colour=0), dict(colour=3), dict(colour=4),
               dict(filt=5), dict(filt=-2), dict(argb=None), dict(n=None), dict(out=None), dict(stride=7)):
        k = dict(ok, **kw)
        prm = cgamd.PngParams(k["colour"], k["filt"])
        rc = lib.cg_image_encode_png_host(k["argb"], k["w"], k["h"], k["stride"], C.byref(prm), k["out"], k["cap"], k["n"])
        assert rc == cgamd.CG_E_INVALID, kw
    assert lib.cg_image_encode_png_host(ok["argb"], 8, 8, 0, None, ok["out"], 4096, ok["n"]) == cgamd.CG_E_INVALID


# ---- size against zlib's run-length strategy ----
SCREENSHOTS = ("rt_screenshot_320x256.bmp", "rast_screenshot_900x720.bmp.xz")
# The excess of our IDAT chunks over the stand-in, measured on the CPU (profiles/png_enc_size.json):
# 0.000 % on rt_screenshot_320x256 (38,005 bytes each) and -0.103 % on rast_screenshot_900x720
# (368,677 against 369,057).  The token model is the stand-in's, so only trees and headers differ.
MEASURED_EXCESS_PERCENT = {"rt_screenshot_320x256.bmp": 0.000, "rast_screenshot_900x720.bmp.xz": -0.103}
MARGIN_PERCENT = 1.0


def _screenshot(name):
    path = os.path.join(HERE, "golden", name)
    with (lzma.open(path) if name.endswith(".xz") else open(path, "rb")) as f:
        b = f.read()
    off, w, h = int.from_bytes(b[10:14], "little"), int.from_bytes(b[18:22], "little"), int.from_bytes(b[22:26], "little", signed=True)
    bits = b[28] | b[29] << 8
    assert bits in (24, 32)
    pitch = (w * bits // 8 + 3) & ~3
    rows = np.frombuffer(b, np.uint8, pitch * abs(h), off).reshape(abs(h), pitch)[:, :w * bits // 8].reshape(abs(h), w, bits // 8)
    if h > 0:
        rows = rows[::-1]
    px = rows.astype(np.uint32)
    return np.uint32(0xFF000000) | (px[..., 2] << 16) | (px[..., 1] << 8) | px[..., 0]


def size_excess(name):
    """-> (our IDAT bytes, the stand-in's, the excess in percent): the stand-in deflates the same
    filtered bytes with zlib at level 9, strategy Z_RLE, raw, a full flush per 16-row band, and
    12 bytes of chunk a band."""
    argb = _screenshot(name)
    data = ref.encode(argb, ref.RGB, ref.ADAPTIVE)
    assert data == cgamd.image_encode_png_host(argb, ref.RGB, ref.ADAPTIVE)
    ours = sum(len(body) + 12 for kind, body in ref.walk(data) if kind == b"IDAT")
    filt = ref.filtered(argb, ref.RGB, ref.ADAPTIVE)
    stand_in = 0
    for k in range(0, argb.shape[0], ref.BAND):
        z = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        stand_in += len(z.compress(filt[k:k + ref.BAND].tobytes()) + z.flush(zlib.Z_FULL_FLUSH)) + 12
    return ours, stand_in, 100.0 * (ours - stand_in) / stand_in


@pytest.mark.parametrize("name", SCREENSHOTS)
def test_size_against_the_run_length_stand_in(name):
    ours, stand_in, excess = size_excess(name)
    print(f"{name}: {ours} bytes against {stand_in}, excess {excess:.3f} %")
    assert excess <= MEASURED_EXCESS_PERCENT[name] + MARGIN_PERCENT


if __name__ == "__main__":
    doc = {"what": "IDAT bytes of the encoder's file (RGB, adaptive) against zlib level 9 Z_RLE raw deflate of the same filtered "
                   "bytes with a full flush per 16-row band plus 12 bytes a band; measured on the CPU",
           "zlib": zlib.ZLIB_VERSION, "frames": {}}
    for shot in SCREENSHOTS:
        o, s, e = size_excess(shot)
        doc["frames"][shot] = {"ours_idat_bytes": o, "stand_in_bytes": s, "excess_percent": round(e, 3)}
    with open(os.path.join(os.path.dirname(HERE), "profiles", "png_enc_size.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1))
