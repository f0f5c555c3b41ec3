"""Shared by the JPEG decoder tests (numpy only, no Pillow, no GPU):

  encode()        a baseline (SOF0) JPEG writer that starts from chosen quantised
                  coefficients and quantisation tables: flat Huffman tables (4-bit DC
                  codes over categories 0-11, 8-bit AC codes over the 162 baseline
                  symbols, neither with an all-ones code), optional restart intervals,
                  one interleaved scan or one scan per component, optional JFIF / Adobe
                  markers, free component ids and sampling factors
  ideal_plane()   the float64 N-point inverse DCT of the dequantised blocks, N = 8 or 16
  jdcolor9()      libjpeg 9's integer YCbCr -> RGB (jdcolor.c ycc_rgb_convert), as BGR
  synthetic_cases(), pillow_case_params()   the deterministic case lists
  load_fixture()  tests/golden/jpeg_cases.npz (written by tests/golden/make_jpeg_cases.py)
  ideal_errors(), bound_from()   the |sample - ideal| check shared by the CPU and GPU tests
"""
import hashlib
import math
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "jpeg_cases.npz")
SAN_DIR = os.path.join(GOLDEN, "jpeg_san")

# T.81 Figure A.6: zig-zag position -> natural (row-major) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                   45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Table K.1 (luminance), natural order
Q_ANNEX_K = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113,
                      92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]).reshape(8, 8)
Q_FLAT3 = np.full((8, 8), 3)
Q_FLAT2 = np.full((8, 8), 2)
QUANT = {"annexk": Q_ANNEX_K, "flat3": Q_FLAT3, "flat2": Q_FLAT2}

# the 162 symbols of a baseline AC table: EOB, ZRL, and run/size with size 1..10
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
_AC_CODE = {sym: k for k, sym in enumerate(AC_SYMBOLS)}


# ------------------------------------------------------------------ the encoder

class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)      # pad with ones (T.81 F.1.2.3)

    def marker(self, m):
        self.flush()
        self.out += bytes([0xFF, m])


def _magnitude(v):
    """(category, the category's low bits) of a DC difference or AC coefficient (T.81 F.1.2.1)."""
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _put_block(bw, block, pred):
    """One 8x8 block of quantised coefficients (natural order); returns its DC value."""
    zz = block.reshape(64)[ZIGZAG]
    dc = int(zz[0])
    s, low = _magnitude(dc - pred)
    assert s <= 11, "DC difference outside the table's categories"
    bw.put(s, 4)
    bw.put(low, s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(_AC_CODE[0xF0], 8)
            run -= 16
        s, low = _magnitude(v)
        assert s <= 10, "AC coefficient outside the table's categories"
        bw.put(_AC_CODE[(run << 4) | s], 8)
        bw.put(low, s)
        run = 0
    if run:
        bw.put(_AC_CODE[0x00], 8)
    return dc


def _seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def grid(width, height, sampling):
    """Per component (blocks_y, blocks_x) of the coefficient arrays encode() takes: whole
    MCUs for a multi-component file, ceil(size / 8) for a one-component file (whose declared
    sampling factors mean nothing, T.81 A.2.2 / libjpeg jdinput.c)."""
    if len(sampling) == 1:
        return [((height + 7) // 8, (width + 7) // 8)]
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return [(my * v, mx * h) for h, v in sampling]


def encode(coef, quant, width, height, sampling, restart=0, interleaved=True, jfif=False, adobe=None,
           ids=None):
    """Baseline JPEG bytes of the quantised coefficients `coef`: per component an int array
    (blocks_y, blocks_x, 8, 8) of the shape grid() gives, natural [v][u] order.  quant: per
    component an (8, 8) table.  sampling: per component (h, v).  restart: the restart
    interval in MCUs (0: none).  interleaved=False writes one scan per component, which
    then covers ceil(component size / 8) blocks only.  adobe: None, or the APP14 transform."""
    nc = len(sampling)
    ids = tuple(range(1, nc + 1)) if ids is None else tuple(ids)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    j = bytearray(b"\xff\xd8")
    if jfif:
        j += _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    if adobe is not None:
        j += _seg(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([adobe]))
    tables, tq = [], []
    for q in quant:                                   # one DQT entry per distinct table
        for k, t in enumerate(tables):
            if np.array_equal(t, q):
                tq.append(k)
                break
        else:
            tq.append(len(tables))
            tables.append(np.asarray(q))
    for k, t in enumerate(tables):
        j += _seg(0xDB, bytes([k]) + bytes(int(x) for x in t.reshape(64)[ZIGZAG]))
    sof = struct.pack(">BHHB", 8, height, width, nc)
    for i, (h, v) in enumerate(sampling):
        sof += bytes([ids[i], (h << 4) | v, tq[i]])
    j += _seg(0xC0, sof)
    j += _seg(0xC4, bytes([0x00, 0, 0, 0, 12] + [0] * 12) + bytes(range(12)))
    j += _seg(0xC4, bytes([0x10, 0, 0, 0, 0, 0, 0, 0, 162] + [0] * 8) + bytes(AC_SYMBOLS))
    if restart:
        j += _seg(0xDD, struct.pack(">H", restart))

    def run_scan(comps, mcus):
        """comps: component indices; mcus: the scan's MCUs, each a list of (comp, by, bx)."""
        nonlocal j
        j += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([ids[c], 0x00]) for c in comps) + bytes([0, 63, 0]))
        bw, pred, rst = _Bits(), {c: 0 for c in comps}, 0
        for n, mcu in enumerate(mcus):
            if restart and n and n % restart == 0:
                bw.marker(0xD0 + (rst & 7))
                rst += 1
                pred = {c: 0 for c in comps}
            for c, by, bx in mcu:
                pred[c] = _put_block(bw, coef[c][by, bx], pred[c])
        bw.flush()
        j += bw.out

    if nc == 1 or not interleaved:
        for c, (h, v) in enumerate(sampling):
            if nc == 1:
                nby, nbx = coef[c].shape[:2]
            else:
                nbx = (-(-width * h // hmax) + 7) // 8
                nby = (-(-height * v // vmax) + 7) // 8
            run_scan([c], [[(c, by, bx)] for by in range(nby) for bx in range(nbx)])
    else:
        mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
        run_scan(list(range(nc)),
                 [[(c, y * v + dy, x * h + dx) for c, (h, v) in enumerate(sampling) for dy in range(v)
                   for dx in range(h)] for y in range(my) for x in range(mx)])
    return bytes(j + b"\xff\xd9")


# ------------------------------------------------------------- the references

def ideal_plane(coef, q, N):
    """float64 N-point inverse DCT (N = 8 or 16) of the dequantised blocks, unclamped:
    f(x,y) = 1/4 sum_{u,v<8} C(u) C(v) F(v,u) cos((2x+1) u pi / 2N) cos((2y+1) v pi / 2N) + 128,
    C(0) = 1/sqrt(2).  coef: (blocks_y, blocks_x, 8, 8) -> (blocks_y * N, blocks_x * N)."""
    x, u = np.arange(N, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    A = np.cos((2 * x + 1) * u * math.pi / (2 * N))
    A[:, 0] *= 1 / math.sqrt(2)
    F = np.asarray(coef, np.float64) * np.asarray(q, np.float64)
    f = 0.25 * np.einsum("yv,abvu,xu->aybx", A, F, A) + 128.0
    by, bx = F.shape[:2]
    return f.reshape(by * N, bx * N)


def _fix16(x):
    return int(x * 65536 + 0.5)


def jdcolor9(ycc):
    """libjpeg 9 jdcolor.c ycc_rgb_convert on uint8 (H, W, 3) YCbCr planes -> uint8 BGR.
    (libjpeg 6b / turbo use FIX(0.34414) where libjpeg 9 has FIX(0.344136286).)"""
    y, cb, cr = (ycc[..., k].astype(np.int64) for k in range(3))
    cb, cr, half = cb - 128, cr - 128, 1 << 15
    r = y + ((_fix16(1.402) * cr + half) >> 16)
    g = y + ((-_fix16(0.344136286) * cb + half - _fix16(0.714136286) * cr) >> 16)
    b = y + ((_fix16(1.772) * cb + half) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


# ------------------------------------------------------------------ the cases

SIZES = [(1, 1), (8, 8), (7, 9), (17, 15), (16, 16), (33, 31), (65, 40)]       # (width, height)
SAMPLINGS = {"gray": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)]}
PATTERNS = ["dense", "dconly", "single", "sparse", "c63"]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _coefficients(rng, shape, q, pattern):
    """Quantised coefficients (blocks_y, blocks_x, 8, 8) whose ideal samples stay well inside
    [-128, 383]; `clamp` drives a good share of them below 0 and above 255."""
    by, bx = shape
    c = np.zeros((by, bx, 8, 8), np.int64)
    qf = np.asarray(q, np.float64)
    dc = np.rint(rng.uniform(-500, 500, (by, bx)) / qf[0, 0]).astype(np.int64)
    u, v = np.meshgrid(np.arange(8), np.arange(8))
    if pattern == "dense":
        c = np.rint(rng.uniform(-1, 1, c.shape) * 260.0 / (1 + u + v) / qf).astype(np.int64)
        c[..., 0, 0] = dc
    elif pattern == "dconly":
        c[..., 0, 0] = dc
    elif pattern in ("single", "c63"):
        pos = rng.integers(1, 64, (by, bx)) if pattern == "single" else np.full((by, bx), 63)
        val = np.rint(rng.uniform(-300, 300, (by, bx)) / qf.reshape(64)[pos]).astype(np.int64)
        val[val == 0] = 1
        np.put_along_axis(c.reshape(by, bx, 64), pos[..., None], val[..., None], -1)
        c[..., 0, 0] = dc // 2
    elif pattern == "sparse":
        mask = rng.random(c.shape) < 0.08
        c = np.where(mask, np.rint(rng.uniform(-150, 150, c.shape) / qf), 0).astype(np.int64)
        c[..., 0, 0] = dc
    elif pattern == "clamp":
        # half the blocks DC only, up to +-960 (dequantised +-1920: ideal -112 .. 368); the others
        # one coefficient of +-360 on a small DC (ideal within 128 +- 25 +- 180)
        dconly = rng.random((by, bx)) < 0.5
        big = rng.integers(-960, 961, (by, bx))
        pos = rng.integers(1, 64, (by, bx))
        val = np.where(rng.random((by, bx)) < 0.5, 360, -360)
        np.put_along_axis(c.reshape(by, bx, 64), pos[..., None], np.where(dconly, 0, val)[..., None], -1)
        c[..., 0, 0] = np.where(dconly, big, rng.integers(-100, 101, (by, bx)))
    else:
        raise ValueError(pattern)
    return c


class Synthetic:
    """One synthetic file: .name, .jpeg, its inputs, and .planes -- True when the decoded
    channels are the components' own sample planes (gray, or Adobe transform 0)."""

    def __init__(self, name, width, height, sampling, pattern, qnames, restart=0, interleaved=True,
                 jfif=False, adobe=0, ids=None):
        self.name, self.width, self.height, self.sampling = name, width, height, sampling
        self.clamping = pattern == "clamp"
        rng = _rng(name)
        self.quant = [QUANT[qnames[min(i, len(qnames) - 1)]] for i in range(len(sampling))]
        self.coef = [_coefficients(rng, g, q, pattern) for g, q in zip(grid(width, height, sampling), self.quant)]
        nc = len(sampling)
        self.channels = nc
        rgb_ids = ids is not None and tuple(ids) == (0x52, 0x47, 0x42)
        # libjpeg default_decompress_parms: JFIF -> YCbCr, else Adobe by its transform, else by ids
        self.planes = nc == 1 or (not jfif and (adobe == 0 if adobe is not None else rgb_ids))
        self.jpeg = encode(self.coef, self.quant, width, height, sampling, restart, interleaved, jfif,
                           adobe if nc == 3 else None, ids)
        hmax = max(h for h, _ in sampling)
        self.scale = [1 if nc == 1 else hmax // h for h, _ in sampling]
        self.any_scaled = max(self.scale) > 1

    def ideal(self):
        """Unclamped float64 ideal of the decoded array, (H, W) or (H, W, 3) in BGR order
        (planes files only)."""
        assert self.planes
        p = [ideal_plane(c, q, 8 * s)[:self.height, :self.width]
             for c, q, s in zip(self.coef, self.quant, self.scale)]
        return p[0] if self.channels == 1 else np.stack(p[::-1], -1)


_SYNTHETIC = None


def synthetic_cases():
    """The deterministic synthetic list (built once)."""
    global _SYNTHETIC
    if _SYNTHETIC is not None:
        return _SYNTHETIC
    S, out = SAMPLINGS, []
    # every pattern at every sampling, sizes that end inside a block / an MCU, both tables
    sizes = [(1, 1), (7, 9), (17, 15), (16, 16), (33, 31), (65, 40)]
    for si, (w, h) in enumerate(sizes):
        for pi, pat in enumerate(PATTERNS):
            for sname in ("gray", "444", "420"):
                k = si + pi
                qn = ("annexk", "flat3") if k % 2 == 0 else ("flat3", "annexk")
                out.append(Synthetic(f"syn_{pat}_{sname}_{w}x{h}", w, h, S[sname], pat, qn, restart=(0, 1, 2, 3)[k % 4],
                                     interleaved=k % 3 != 1))
    # the clamping set: quantisation value 2
    for w, h in ((33, 31), (65, 40)):
        for sname in ("gray", "444", "420"):
            out.append(Synthetic(f"clamp_{sname}_{w}x{h}", w, h, S[sname], "clamp", ("flat2",), restart=(w > 40) * 3))
    # a one-component file that declares 2x2 sampling
    out.append(Synthetic("gray_declared_2x2_33x31", 33, 31, [(2, 2)], "dense", ("annexk",)))
    out.append(Synthetic("gray_declared_2x2_r2_17x15", 17, 15, [(2, 2)], "sparse", ("flat3",), restart=2))
    # three components, one scan per component, at each sampling, with and without restarts
    for sname in ("444", "420"):
        for r in (0, 3):
            out.append(Synthetic(f"perscan_{sname}_r{r}_65x40", 65, 40, S[sname], "dense", ("annexk", "flat3"),
                                 restart=r, interleaved=False))
    # restart interval 1 on more than 8 MCUs: the RSTn counter wraps past 7
    for sname in ("gray", "444", "420"):
        for inter in (True, False):
            out.append(Synthetic(f"rst1_{sname}_{'il' if inter else 'ni'}_65x40", 65, 40, S[sname], "sparse",
                                 ("flat3",), restart=1, interleaved=inter))
    # colour-space conventions (libjpeg default_decompress_parms)
    for sname in ("444", "420"):
        out.append(Synthetic(f"cs_a_nomarkers_ids123_{sname}", 17, 15, S[sname], "dense", ("flat3",), adobe=None))
        out.append(Synthetic(f"cs_b_nomarkers_idsRGB_{sname}", 17, 15, S[sname], "dense", ("flat3",), adobe=None,
                             ids=(0x52, 0x47, 0x42)))
        out.append(Synthetic(f"cs_c_jfif_and_adobe0_{sname}", 17, 15, S[sname], "dense", ("flat3",), jfif=True,
                             adobe=0))
        out.append(Synthetic(f"cs_d_adobe1_{sname}", 17, 15, S[sname], "dense", ("flat3",), adobe=1))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    _SYNTHETIC = out
    return out


def pillow_case_params():
    """(name, (w, h), mode, progressive, restart blocks, quality kind) of the Pillow-encoded files."""
    out = []
    for w, h in SIZES:
        for mode in ("gray", "444", "420"):
            for prog in (False, True):
                for r in (0, 1, 3):
                    for qk in ("q35opt", "q100"):
                        out.append((f"pil_{mode}_{'prog' if prog else 'base'}_r{r}_{qk}_{w}x{h}", (w, h), mode, prog,
                                    r, qk))
    return out


_FIXTURE = None


def load_fixture():
    """{'pillow': {name: (jpeg bytes, hash or None)}, 'synthetic': {name: (sha256 of the
    file, hash or None)}} from tests/golden/jpeg_cases.npz."""
    global _FIXTURE
    if _FIXTURE is None:
        z = np.load(FIXTURE)
        blob, off = z["blob"].tobytes(), z["offsets"]
        pil = {str(n): (blob[off[i]:off[i + 1]], str(hh) or None)
               for i, (n, hh) in enumerate(zip(z["names"], z["hashes"]))}
        syn = {str(n): (str(s), str(hh) or None) for n, s, hh in zip(z["syn_names"], z["syn_sha"], z["syn_hashes"])}
        _FIXTURE = {"pillow": pil, "synthetic": syn}
    return _FIXTURE


def all_files():
    """[(name, jpeg bytes, recorded hash or None)] of every fixture and synthetic file."""
    fx = load_fixture()
    out = [(n, j, hh) for n, (j, hh) in fx["pillow"].items()]
    out += [(c.name, c.jpeg, fx["synthetic"][c.name][1]) for c in synthetic_cases()]
    return out


# ------------------------------------------------------------- the ideal check

def ideal_errors(case, img):
    """Of one planes file decoded to `img`: (worst |sample - clip(ideal, 0, 255)| over the
    samples whose ideal lies in [-128, 383], samples excluded, samples below 0, above 255, all)."""
    ideal = case.ideal()
    keep = (ideal >= -128.0) & (ideal <= 383.0)
    err = np.abs(np.asarray(img, np.float64) - np.clip(ideal, 0.0, 255.0))
    return (float(err[keep].max()), int((~keep).sum()), int((ideal < 0).sum()), int((ideal > 255).sum()),
            int(ideal.size))


def bound_from(decode):
    """B = 0.5 + twice the worst excess over 0.5 of `decode` (the oracle) on the planes
    files; also the worst error itself."""
    worst = max(ideal_errors(c, decode(c.jpeg))[0] for c in synthetic_cases() if c.planes)
    return 0.5 + 2.0 * max(worst - 0.5, 0.0), worst
