"""(a) A numpy restatement of the EXR encoder's contract (include/cg_render.h, "EXR encoding"), written
from the contract's words: the half rule in integers, the header, the chunk table, the planar rows,
ZIP's reorder and predictor and the raw fallback.  The deflate rules are the PNG contract's and come
from png_enc_ref.  encode() returns the file; info() also says per chunk whether it stayed raw and how long its data is.

(b) read(): a reader that shares nothing with (a) -- struct, zlib.decompress and numpy only, written
from the OpenEXR file layout.  It checks the container as it goes and returns the channels' samples.
No OpenEXR library is at hand here, so zlib judges every stream and this reader the container."""
import struct
import zlib

import numpy as np

import png_enc_ref

RGB, RGBA = 3, 4
HALF, FLOAT = 1, 2
NONE, ZIP = 0, 3
ZIP_LINES = 16


# ---- (a) the contract ---------------------------------------------------------------------------
def half_bits(f32_bits):
    """Rule 1 on uint32 float bits -> uint16 half bits, in integers."""
    f = np.asarray(f32_bits, np.uint32).astype(np.int64)
    sign = (f >> 16) & 0x8000
    a = f & 0x7FFFFFFF
    mant = (a >> 13) & 0x3FF
    nan = 0x7C00 | mant | (mant == 0)
    r = a - 0x38000000
    h = r >> 13
    rem = r & 0x1FFF
    normal = h + ((rem > 0x1000) | ((rem == 0x1000) & ((h & 1) == 1)))
    shift = np.clip(126 - (a >> 23), 14, 24)
    m = (a & 0x7FFFFF) | 0x800000
    hs = m >> shift
    rs = m & ((1 << shift) - 1)
    halfway = 1 << (shift - 1)
    sub = hs + ((rs > halfway) | ((rs == halfway) & ((hs & 1) == 1)))
    out = np.where(a > 0x7F800000, nan,
                   np.where(a >= 0x47800000, 0x7C00, np.where(a >= 0x38800000, normal, np.where(a < 0x33000000, 0, sub))))
    return (sign | out).astype(np.uint16)


def samples(rgba, channels, typ, alpha_scale=1.0):
    """(H, nch, W) unsigned integers in file channel order (A B G R or B G R)."""
    px = np.ascontiguousarray(rgba, np.float32)
    comps = [px[..., 0], px[..., 1], px[..., 2]]
    if channels == RGBA:
        w = px[..., 3]
        scale = np.float32(alpha_scale)
        if scale.view(np.uint32) != 0x3F800000:
            w = w * scale                                   # one float32 product
        comps.append(w)
    planes = np.stack(comps[::-1], 1)                       # name order is the reverse of x y z w
    bits = np.ascontiguousarray(planes).view(np.uint32)
    return half_bits(bits) if typ == HALF else bits


def header(w, h, channels, typ, compression):
    def attr(name, kind, value):
        return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value
    names = (b"A", b"B", b"G", b"R") if channels == RGBA else (b"B", b"G", b"R")
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", typ, 0, 1, 1) for n in names) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (bytes([0x76, 0x2F, 0x31, 0x01]) + struct.pack("<I", 2) + attr(b"channels", b"chlist", chlist) +
            attr(b"compression", b"compression", bytes([compression])) + attr(b"dataWindow", b"box2i", box) +
            attr(b"displayWindow", b"box2i", box) + attr(b"lineOrder", b"lineOrder", b"\0") +
            attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) +
            attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0)) +
            attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def predicted(raw):
    """Rule 5's d of a chunk's raw bytes."""
    r = np.frombuffer(raw, np.uint8).astype(np.int64)
    t = np.concatenate([r[0::2], r[1::2]])
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 255
    return d.astype(np.uint8)


def zip_stream(raw):
    d = predicted(raw)
    return png_enc_ref.band_data(d, True, True) + png_enc_ref.adler32(d.tobytes()).to_bytes(4, "big")


def info(rgba, channels=RGBA, typ=HALF, compression=ZIP, alpha_scale=1.0):
    """-> (the file, per chunk a record: "raw" where its data is the raw bytes, "bytes" the data's length)."""
    s = samples(rgba, channels, typ, alpha_scale)
    h, _, w = s.shape
    lines = ZIP_LINES if compression == ZIP else 1
    le = s.astype("<u2" if typ == HALF else "<u4")
    chunks, notes = [], []
    for y in range(0, h, lines):
        raw = le[y:y + lines].tobytes()
        data = raw
        if compression == ZIP:
            z = zip_stream(raw)
            if len(z) < len(raw):
                data = z
        chunks.append(struct.pack("<ii", y, len(data)) + data)
        notes.append({"raw": data is raw, "bytes": len(data)})
    head = header(w, h, channels, typ, compression)
    at, table = len(head) + 8 * len(chunks), b""
    for c in chunks:
        table += struct.pack("<Q", at)
        at += len(c)
    return head + table + b"".join(chunks), notes


def encode(rgba, channels=RGBA, typ=HALF, compression=ZIP, alpha_scale=1.0):
    return info(rgba, channels, typ, compression, alpha_scale)[0]


# ---- (b) a reader from the file layout alone -----------------------------------------------------
def _cstr(data, p):
    e = data.index(b"\0", p)
    return data[p:e], e + 1


def read(data):
    """-> dict(width, height, type, compression, names, planes {name: (H, W) uint16 / uint32 bits},
    raw_chunks, chunks); asserts the layout on the way."""
    data = bytes(data)
    assert data[:4] == b"\x76\x2f\x31\x01", "magic"
    assert data[4:8] == b"\x02\x00\x00\x00", "version 2, no flags: a single-part scanline file"
    p, attrs = 8, {}
    while data[p]:
        name, p = _cstr(data, p)
        kind, p = _cstr(data, p)
        size, = struct.unpack_from("<i", data, p)
        attrs[name] = (kind, data[p + 4:p + 4 + size])
        assert len(attrs[name][1]) == size
        p += 4 + size
    p += 1
    want = {b"channels": b"chlist", b"compression": b"compression", b"dataWindow": b"box2i", b"displayWindow": b"box2i",
            b"lineOrder": b"lineOrder", b"pixelAspectRatio": b"float", b"screenWindowCenter": b"v2f",
            b"screenWindowWidth": b"float"}
    assert {k: v[0] for k, v in attrs.items()} == want, "the required attributes and their types"
    ch, q, names, types = attrs[b"channels"][1], 0, [], []
    while ch[q]:
        name, q = _cstr(ch, q)
        typ, lin, xs, ys = struct.unpack_from("<iB3xii", ch, q)
        q += 16
        assert (lin, xs, ys) == (0, 1, 1)
        names.append(name.decode())
        types.append(typ)
    assert q + 1 == len(ch)
    assert names in (["A", "B", "G", "R"], ["B", "G", "R"]) and len(set(types)) == 1 and types[0] in (HALF, FLOAT), "channels"
    typ = types[0]
    comp = attrs[b"compression"][1][0]
    assert comp in (NONE, ZIP)
    x0, y0, x1, y1 = struct.unpack("<4i", attrs[b"dataWindow"][1])
    assert (x0, y0) == (0, 0) and attrs[b"displayWindow"][1] == attrs[b"dataWindow"][1]
    assert attrs[b"lineOrder"][1] == b"\0" and struct.unpack("<f", attrs[b"pixelAspectRatio"][1]) == (1.0,)
    assert struct.unpack("<2f", attrs[b"screenWindowCenter"][1]) == (0.0, 0.0)
    assert struct.unpack("<f", attrs[b"screenWindowWidth"][1]) == (1.0,)
    w, h = x1 + 1, y1 + 1
    lines = 16 if comp == ZIP else 1
    nchunks = -(-h // lines)
    table = struct.unpack_from(f"<{nchunks}Q", data, p)
    p += 8 * nchunks
    bps = 2 if typ == HALF else 4
    rows = np.zeros((h, len(names), w), np.uint16 if typ == HALF else np.uint32)
    raw_chunks = 0
    for k in range(nchunks):
        assert table[k] == p, f"table entry {k} does not point at its chunk"
        y, n = struct.unpack_from("<ii", data, p)
        assert y == k * lines, "a chunk's first y"
        nrows = min(lines, h - y)
        full = nrows * len(names) * w * bps
        body = data[p + 8:p + 8 + n]
        assert len(body) == n, "a chunk runs past the file"
        assert n == full or (comp == ZIP and 0 < n < full), "a chunk's length"
        if n == full:
            raw = body
            raw_chunks += comp == ZIP
        else:
            d = np.frombuffer(zlib.decompress(body), np.uint8).astype(np.int64)
            assert d.size == full, "a stream's length"
            t = (np.cumsum(d) - 128 * np.arange(full)) & 255
            out = np.zeros(full, np.uint8)
            out[0::2] = t[:(full + 1) // 2]
            out[1::2] = t[(full + 1) // 2:]
            raw = out.tobytes()
        rows[y:y + nrows] = np.frombuffer(raw, "<u2" if typ == HALF else "<u4").reshape(nrows, len(names), w)
        p += 8 + n
    assert p == len(data), "the file ends at its last chunk"
    return {"width": w, "height": h, "type": typ, "compression": comp, "names": names, "chunks": nchunks,
            "raw_chunks": int(raw_chunks), "planes": {nm: rows[:, i] for i, nm in enumerate(names)}}


def expected_planes(rgba, channels, typ, alpha_scale=1.0):
    """What read() must return for a picture, from numpy's own conversion: FLOAT the bits, HALF astype(float16)."""
    px = np.ascontiguousarray(rgba, np.float32)
    comps = {"R": px[..., 0], "G": px[..., 1], "B": px[..., 2]}
    if channels == RGBA:
        s = np.float32(alpha_scale)
        comps["A"] = px[..., 3] if s.view(np.uint32) == 0x3F800000 else px[..., 3] * s
    with np.errstate(over="ignore", invalid="ignore"):
        return {k: (np.ascontiguousarray(v).view(np.uint32) if typ == FLOAT else v.astype(np.float16).view(np.uint16))
                for k, v in comps.items()}
