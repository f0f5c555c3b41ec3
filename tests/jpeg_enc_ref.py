"""A numpy restatement of the JPEG encoder's contract (include/cg_render.h, "JPEG encoding"), header
included.  It shares no code with the library and is built the other way round: whole padded
planes, every block transformed at once, one Python integer as an interval's bit string.  All
arithmetic is int64 numpy or Python integers, `>>` arithmetic."""
import numpy as np

S444, S420 = 0, 2

BASE_Q = (
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32,
)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728"
                  "292a3435363738393a434445464748494a535455565758595a636465666768696a737475767778797a83848586878889"
                  "8a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2"
                  "e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a26"
                  "2728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a828384858687"
                  "88898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9da"
                  "e2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
)
assert all(len(v) == 162 == sum(b) for v, b in zip(AC_VALS, AC_BITS))


def _zigzag():
    """Row-major index of the k-th zig-zag coefficient: anti-diagonals, alternating direction."""
    order = []
    for d in range(15):
        cells = [(y, d - y) for y in range(8) if 0 <= d - y < 8]
        order += cells if d % 2 else cells[::-1]
    return np.array([y * 8 + x for y, x in order])


ZIGZAG = _zigzag()


def _codes(bits, vals):
    """Annex C: {symbol: (code, length)}."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[t], list(range(12))) for t in range(2)]
AC_CODES = [_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def quant_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((np.array(b, np.int64) * scale + 50) // 100, 1, 255) for b in BASE_Q]


def header(w, h, quality, sub):
    q = quant_tables(quality)
    mx = -(-w // (16 if sub == S420 else 8))
    out = bytes.fromhex("ffd8ffe000104a46494600010100000100010000")
    for t in range(2):
        out += bytes([0xFF, 0xDB, 0x00, 0x43, t]) + bytes(int(v) for v in q[t][ZIGZAG])
    out += bytes([0xFF, 0xC0, 0x00, 0x11, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22 if sub == S420 else 0x11, 0,
                  2, 0x11, 1, 3, 0x11, 1])
    for t in range(2):
        out += bytes([0xFF, 0xC4, 0x00, 0x1F, t]) + bytes(DC_BITS[t]) + bytes(range(12))
        out += bytes([0xFF, 0xC4, 0x00, 0xB5, 0x10 | t]) + bytes(AC_BITS[t]) + AC_VALS[t]
    out += bytes([0xFF, 0xDD, 0x00, 0x04, mx >> 8, mx & 255])
    return out + bytes.fromhex("ffda000c03010002110311003f00")


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, rows):
    """jfdctint over the last axis of d (..., 8)."""
    n = 11 if rows else 15
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if rows else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if rows else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069, z4 * -3196
    z3, z4 = z3 + z5, z4 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _blocks(plane, q):
    """A padded plane (8 BY, 8 BX) to quantised coefficients (BY, BX, 64) in zig-zag order."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    b = _fdct_pass(b, True)                                           # rows: along x
    b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # columns: along y
    c = b.reshape(by, bx, 64)
    q8 = 8 * q
    v = (np.abs(c) + (q8 >> 1)) // q8
    return (np.sign(c) * v)[..., ZIGZAG]


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def coefficients(argb, quality, sub):
    """Per MCU row, per MCU, the list of (table, zig-zag coefficients) in scan order; plus MX."""
    a = np.asarray(argb, np.uint32)
    h, w = a.shape
    r, g, b = (((a >> s) & 255).astype(np.int64) for s in (16, 8, 0))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    q = quant_tables(quality)
    mcu = 16 if sub == S420 else 8
    mx, my = -(-w // mcu), -(-h // mcu)
    if sub == S444:
        planes = [_blocks(_pad(p, 8 * my, 8 * mx), q[1 if i else 0]) for i, p in enumerate((y, cb, cr))]
        return [[[(1 if i else 0, planes[i][row, col]) for i in range(3)] for col in range(mx)] for row in range(my)], mx
    yc = _blocks(_pad(y, 16 * my, 16 * mx), q[0])
    chroma = []
    for p in (cb, cr):
        p = _pad(p, h + (h & 1), 16 * mx)
        bias = np.where(np.arange(8 * mx) & 1, 2, 1)
        c = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        chroma.append(_blocks(_pad(c, 8 * my, 8 * mx), q[1]))
    bw, bh = -(-w // 8), -(-h // 8)
    rows = []
    for row in range(my):
        mcus = []
        for col in range(mx):
            blocks = []
            for k in range(4):
                bx, by = 2 * col + (k & 1), 2 * row + (k >> 1)
                c = yc[by, bx]
                if bx >= bw or by >= bh:          # a dummy block: the previous block's quantised DC alone
                    c = np.zeros(64, np.int64)
                    c[0] = blocks[-1][1][0]
                blocks.append((0, c))
            blocks += [(1, chroma[0][row, col]), (1, chroma[1][row, col])]
            mcus.append(blocks)
        rows.append(mcus)
    return rows, mx


def _value_bits(v, size):
    return (v - 1 if v < 0 else v) & ((1 << size) - 1)


def _interval(mcus, n_comp_blocks):
    """One MCU row's entropy-coded bytes, padded and stuffed."""
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    for blocks in mcus:
        for k, (t, c) in enumerate(blocks):
            comp = 0 if k < n_comp_blocks else k - n_comp_blocks + 1
            diff = int(c[0]) - pred[comp]
            pred[comp] = int(c[0])
            cat = abs(diff).bit_length()
            code, length = DC_CODES[t][cat]
            acc = (((acc << length) | code) << cat) | _value_bits(diff, cat)
            nbits += length + cat
            last = 0
            for i in np.flatnonzero(c[1:]) + 1:
                run = int(i) - last - 1
                while run >= 16:
                    code, length = AC_CODES[t][0xF0]
                    acc = (acc << length) | code
                    nbits += length
                    run -= 16
                v = int(c[i])
                size = abs(v).bit_length()
                code, length = AC_CODES[t][(run << 4) | size]
                acc = (((acc << length) | code) << size) | _value_bits(v, size)
                nbits += length + size
                last = int(i)
            if last != 63:
                code, length = AC_CODES[t][0]
                acc = (acc << length) | code
                nbits += length
    padn = -nbits % 8
    acc = (acc << padn) | ((1 << padn) - 1)
    return acc.to_bytes((nbits + padn) // 8, "big").replace(b"\xff", b"\xff\x00")


def intervals(argb, quality, sub):
    rows, _ = coefficients(argb, quality, sub)
    return [_interval(m, 4 if sub == S420 else 1) for m in rows]


def encode(argb, quality, sub):
    a = np.asarray(argb, np.uint32)
    h, w = a.shape
    out = header(w, h, quality, sub)
    for k, iv in enumerate(intervals(a, quality, sub)):
        if k:
            out += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        out += iv
    return out + b"\xff\xd9"
