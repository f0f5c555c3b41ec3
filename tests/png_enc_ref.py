"""A numpy restatement of the PNG encoder's contract (include/cg_render.h, "PNG encoding"), written
from the contract's words and sharing no code with the library: filters, bands, the run tokens,
the code-length rule with its limiter, the run-length coded header, the stored fallback, the
chunks.  encode() returns the file; info() also says per band whether it was stored and how deep
the unlimited literal/length code would have been."""
import zlib

import numpy as np

RGB, RGBA = 2, 6
ADAPTIVE = -1
BAND = 16
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
# length 3 .. 258 -> (symbol, extra bits, extra value): RFC 1951's table, the last row that fits
_LEN_SYM = np.zeros((259, 3), np.int64)
for _l in range(3, 259):
    _k = 28 if _l == 258 else max(i for i in range(28) if LEN_BASE[i] <= _l)
    _LEN_SYM[_l] = (257 + _k, LEN_EXTRA[_k], _l - LEN_BASE[_k])


def raw_bytes(argb, colour):
    """(H, W * bpp) uint8: R G B [A] per pixel."""
    a = np.asarray(argb, np.uint32)
    ch = [(a >> 16) & 255, (a >> 8) & 255, a & 255] + ([(a >> 24) & 255] if colour == RGBA else [])
    return np.stack(ch, -1).reshape(a.shape[0], -1).astype(np.uint8)


def filtered(argb, colour, filt):
    """(H, 1 + W * bpp) uint8: every row's type byte and filtered bytes."""
    bpp = 4 if colour == RGBA else 3
    v = raw_bytes(argb, colour).astype(np.int64)
    h, n = v.shape
    a = np.zeros_like(v)
    a[:, bpp:] = v[:, :-bpp]
    b = np.zeros_like(v)
    b[1:] = v[:-1]
    c = np.zeros_like(v)
    c[1:, bpp:] = v[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([v, v - a, v - b, v - ((a + b) >> 1), v - paeth]) & 255          # (5, H, n)
    if filt == ADAPTIVE:
        cost = np.where(cand < 128, cand, 256 - cand).sum(-1)                        # (5, H)
        types = cost.argmin(0)                                                       # the first minimum
    else:
        types = np.full(h, filt)
    rows = cand[types, np.arange(h)]
    return np.concatenate([types[:, None], rows], 1).astype(np.uint8)


def tokens(d):
    """The tokens of a band's bytes d in order -> (symbol, extra bits, extra value) arrays, matches
    with symbols above 256."""
    d = np.asarray(d, np.uint8)
    n = d.size
    start = np.concatenate([[True], d[1:] != d[:-1]])
    first = np.flatnonzero(start)
    runlen = np.diff(np.append(first, n))
    rid = np.cumsum(start) - 1
    j = np.arange(n) - first[rid]          # bytes of the run before this one
    rl = runlen[rid]
    q, r = np.divmod(np.maximum(j - 1, 0), 258)
    full = (rl - 1) // 258                 # matches of 258
    rem = (rl - 1) - 258 * full
    in_run = (rl >= 4) & (j >= 1)
    mlen = np.where(q < full, 258, rem)    # the match this byte falls into, were there one
    is_match = in_run & (mlen >= 3)
    literal = ~is_match
    emits = literal | (is_match & (r == 0))
    sym = np.where(literal, d.astype(np.int64), _LEN_SYM[np.where(is_match, mlen, 3), 0])
    eb = np.where(literal, 0, _LEN_SYM[np.where(is_match, mlen, 3), 1])
    ev = np.where(literal, 0, _LEN_SYM[np.where(is_match, mlen, 3), 2])
    return sym[emits], eb[emits], ev[emits]


def code_lengths(freq, limit, depth_out=None):
    """Rule 5.  depth_out: a list that receives the deepest leaf before the limit."""
    freq = [int(f) for f in freq]
    used = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    lengths = [0] * len(freq)
    m = len(used)
    if m == 0:
        return lengths
    if m == 1:
        lengths[used[0][1]] = 1
        return lengths
    # nodes: (weight, children); leaves queue and internal queue, the leaf first on a tie
    leaves = [(f, None, i) for i, (f, s) in enumerate(used)]
    inner = []
    li = ii = 0

    def take():
        nonlocal li, ii
        if li < m and (ii >= len(inner) or leaves[li][0] <= inner[ii][0]):
            li += 1
            return leaves[li - 1]
        ii += 1
        return inner[ii - 1]
    for _ in range(m - 1):
        x = take()
        y = take()
        inner.append((x[0] + y[0], (x, y), None))
    depth = [0] * m
    stack = [(inner[-1], 0)]
    while stack:
        node, dep = stack.pop()
        if node[1] is None:
            depth[node[2]] = dep
        else:
            stack.append((node[1][0], dep + 1))
            stack.append((node[1][1], dep + 1))
    if depth_out is not None:
        depth_out.append(max(depth))
    count = [0] * (limit + 1)
    for dep in depth:
        count[min(dep, limit)] += 1
    kraft = sum(count[dep] << (limit - dep) for dep in range(1, limit + 1))
    while kraft > (1 << limit):
        dep = max(k for k in range(1, limit) if count[k])
        count[dep] -= 1
        count[dep + 1] += 2
        count[limit] -= 1
        kraft -= 1
    i = 0
    for dep in range(limit, 0, -1):
        for _ in range(count[dep]):
            lengths[used[i][1]] = dep
            i += 1
    return lengths


def canonical(lengths):
    """RFC 1951 3.2.2 -> codes, as sent (top bit first)."""
    mx = max(lengths)
    count = [0] * (mx + 2)
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            codes[s] = nxt[ln]
            nxt[ln] += 1
    return codes


def _reverse(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


def _pack(values, nbits):
    """Bit strings (value, count; lowest bit first) back to back -> (bytes, total bits); the last byte zero padded."""
    values = np.asarray(values, np.int64)
    nbits = np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    idx = np.repeat(np.arange(values.size), nbits)
    k = np.arange(total) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    bits = ((values[idx] >> k) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


def cl_sequence(seq):
    """Rule 6's run-length coding of a length sequence -> [(symbol, extra bits, extra value)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                out.append((18, 7, t - 11))
                r -= t
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                out.append((16, 2, t - 3))
                r -= t
        out += [(v, 0, 0)] * r
    return out


def band_data(d, first, last, note=None):
    """A band's chunk data without the Adler-32: bytes."""
    sym, eb, ev = tokens(d)
    freq = np.bincount(sym, minlength=286)
    freq[256] += 1
    deep = []
    ll = code_lengths(freq, 15, deep)
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    cls = cl_sequence(ll[:hlit] + [1, 1])
    clf = [0] * 19
    for s, _, _ in cls:
        clf[s] += 1
    cl = code_lengths(clf, 7)
    hclen = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1)
    header_bits = 3 + 14 + 3 * hclen + sum(cl[s] + b for s, b, _ in cls)
    extra = [0] * 257 + [LEN_EXTRA[s - 257] + 1 for s in range(257, 286)]
    dyn_bits = header_bits + sum(int(freq[s]) * (ll[s] + extra[s]) for s in range(286))
    n = d.size
    nblk = -(-n // 65535)
    stored = dyn_bits >= 8 * n + 40 * nblk
    if note is not None:
        note.append({"stored": bool(stored), "depth": deep[0], "bytes": int(n), "dyn_bits": int(dyn_bits)})
    out = bytearray(b"\x78\x01" if first else b"")
    if stored:
        raw = d.tobytes()
        for k in range(nblk):
            part = raw[k * 65535:(k + 1) * 65535]
            out += bytes([1 if last and k == nblk - 1 else 0]) + len(part).to_bytes(2, "little")
            out += (len(part) ^ 0xFFFF).to_bytes(2, "little") + part
    else:
        llc, clc = canonical(ll), canonical(cl)
        llr = np.array([_reverse(c, n_) for c, n_ in zip(llc, ll)], np.int64)
        lla = np.array(ll, np.int64)
        vals = [1 if last else 0, 2, hlit - 257, 1, hclen - 4] + [cl[CL_ORDER[k]] for k in range(hclen)]
        nb = [1, 2, 5, 5, 4] + [3] * hclen
        for s, b, v in cls:
            vals.append(_reverse(clc[s], cl[s]) | (v << cl[s]))
            nb.append(cl[s] + b)
        is_m = sym > 256
        # a token: the code, the extra bits above it, a match's 0 distance bit above those
        tv = llr[sym] | (ev << lla[sym])
        tn = lla[sym] + eb + is_m
        vals = np.concatenate([np.array(vals, np.int64), tv, [llr[256]]])
        nb = np.concatenate([np.array(nb, np.int64), tn, [lla[256]]])
        if not last:
            vals, nb = np.append(vals, 0), np.append(nb, 3)
        data, _ = _pack(vals, nb)
        out += data
    if not last:
        out += (b"\x00" if stored else b"") + b"\x00\x00\xff\xff"
    return bytes(out)


def chunk(kind, data):
    return len(data).to_bytes(4, "big") + kind + data + zlib.crc32(kind + data).to_bytes(4, "big")


def adler32(data):
    a, b = 1, 0
    arr = np.frombuffer(data, np.uint8).astype(np.int64)
    for k in range(0, arr.size, 4096):      # pieces short enough for int64
        part = arr[k:k + 4096]
        n = part.size
        b = (b + n * a + int((part * np.arange(n, 0, -1)).sum())) % 65521
        a = (a + int(part.sum())) % 65521
    return (b << 16) | a


def info(argb, colour=RGB, filt=ADAPTIVE):
    """-> (the file, one record per band)."""
    argb = np.asarray(argb, np.uint32)
    h, w = argb.shape
    f = filtered(argb, colour, filt)
    nb = -(-h // BAND)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, colour, 0, 0, 0]))
    note = []
    for k in range(nb):
        d = f[k * BAND:(k + 1) * BAND].reshape(-1)
        data = band_data(d, k == 0, k == nb - 1, note)
        if k == nb - 1:
            data += adler32(f.tobytes()).to_bytes(4, "big")
        out += chunk(b"IDAT", data)
    return out + chunk(b"IEND", b""), note


def encode(argb, colour=RGB, filt=ADAPTIVE):
    return info(argb, colour, filt)[0]


# ---- decoding with nothing of ours: a chunk walk, zlib, un-filtering -------------------------
def walk(data):
    """-> [(type, data)] after checking the signature, every length and every CRC."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    out, p = [], 8
    while p < len(data):
        n = int.from_bytes(data[p:p + 4], "big")
        kind, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        assert len(body) == n, "a chunk runs past the file"
        assert int.from_bytes(data[p + 8 + n:p + 12 + n], "big") == zlib.crc32(kind + body), f"CRC of {kind}"
        out.append((kind, body))
        p += 12 + n
    assert p == len(data) and out[0][0] == b"IHDR" and out[-1] == (b"IEND", b"")
    assert all(k == b"IDAT" for k, _ in out[1:-1]), "a chunk that is neither IHDR, IDAT nor IEND"
    return out


def decode(data):
    """The file -> uint32 (H, W) pixels (alpha 255 for colour type 2), by zlib and numpy alone."""
    chunks = walk(data)
    ihdr = chunks[0][1]
    w, h = int.from_bytes(ihdr[:4], "big"), int.from_bytes(ihdr[4:8], "big")
    assert ihdr[8] == 8 and ihdr[9] in (RGB, RGBA) and ihdr[10:] == b"\0\0\0"
    bpp = 4 if ihdr[9] == RGBA else 3
    raw = zlib.decompress(b"".join(body for _, body in chunks[1:-1]))
    assert len(raw) == h * (1 + w * bpp)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * bpp)
    out = np.zeros((h, w * bpp), np.int64)
    prev = np.zeros(w * bpp, np.int64)
    for y in range(h):
        t, f = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if t == 0:
            cur = f
        elif t == 2:
            cur = (f + prev) & 255
        else:
            cur = np.zeros(w * bpp, np.int64)
            for x in range(w * bpp):
                a = cur[x - bpp] if x >= bpp else 0
                b = prev[x]
                c = prev[x - bpp] if x >= bpp else 0
                if t == 1:
                    pr = a
                elif t == 3:
                    pr = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pr = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[x] = (f[x] + pr) & 255
        out[y] = prev = cur
    px = out.reshape(h, w, bpp).astype(np.uint32)
    alpha = px[..., 3] if bpp == 4 else np.uint32(255)
    return (alpha << 24) | (px[..., 0] << 16) | (px[..., 1] << 8) | px[..., 2]
