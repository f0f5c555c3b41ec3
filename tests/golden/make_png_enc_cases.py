"""Regenerates tests/golden/png_enc_cases.json: per case of the PNG encoder's tests, the SHA-256 and
the length of the file the numpy restatement (tests/png_enc_ref.py) writes.  A case is recorded
only if decoders that share no code with the library accept that file and return the input: a
chunk walk with zlib.crc32, zlib.decompress of the joined IDAT data (the Adler-32 and every
Huffman code), un-filtering in numpy, and Pillow.  The inputs come from inputs() below, explicit
integer recurrences, so the tests rebuild them without Pillow.

    python tests/golden/make_png_enc_cases.py            # rewrite the JSON
    python tests/golden/make_png_enc_cases.py --check    # compare with the committed JSON
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_enc_ref as ref  # noqa: E402

PATH = os.path.join(HERE, "png_enc_cases.json")

# (H, W): what the size catches
SIZES = {
    (1, 1): "fewer bytes to the left than bpp; one row",
    (1, 2): "one pixel to the left",
    (2, 1): "a row above, nothing to the left",
    (15, 5): "one short band",
    (16, 5): "exactly one band",
    (17, 5): "one row over a band",
    (33, 7): "three bands, the last of one row",
    (5, 64): "a band shorter than a piece of 1024 bytes, rows longer than a filter workgroup's stride",
    (40, 65): "three bands of several pieces",
    (17, 1400): "a 16-row RGB band is 65,584 bytes (RGBA 89,616): the stored fallback needs two blocks",
    (20, 900): "a band's dynamic block is longer than the 16,384 bytes of its bit string a workgroup holds",
}
BIG = ((17, 1400), (20, 900))                       # the sizes a row of which holds the run pattern
FILTER_SIZES = ((33, 7), (40, 65))                  # the sizes that also run every fixed filter
COLOURS = (ref.RGB, ref.RGBA)
FIB_SIZE = (17, 1400)                               # the size a band of which holds the Fibonacci frequencies
RUNS = (1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517)


def pcg32(n, seed, seq=54):
    """n outputs of PCG-XSH-RR 64/32 (pcg32_srandom_r(seed, seq), then pcg32_random_r n times).  The
    states by doubling: s_{k+m} = A_m s_k + C_m, (A_2m, C_2m) = (A_m^2, A_m C_m + C_m), mod 2^64."""
    mask = (1 << 64) - 1
    mul, inc = 6364136223846793005, ((seq << 1) | 1) & mask
    s0 = ((inc + seed) * mul + inc) & mask                     # the state the first output is made from
    with np.errstate(over="ignore"):
        st = np.array([s0], np.uint64)
        a, c = mul, inc
        while st.size < n:
            st = np.concatenate([st, st * np.uint64(a) + np.uint64(c)])
            a, c = (a * a) & mask, (a * c + c) & mask
        st = st[:n]
        x = (((st >> np.uint64(18)) ^ st) >> np.uint64(27)) & np.uint64(0xFFFFFFFF)
        rot = st >> np.uint64(59)
        return ((x >> rot) | (x << ((np.uint64(32) - rot) & np.uint64(31)))) & np.uint64(0xFFFFFFFF)


def _pack(px):
    """(H, W, 4) R G B A -> uint32 ARGB8888."""
    px = px.astype(np.uint32)
    return (px[..., 3] << 24) | (px[..., 0] << 16) | (px[..., 1] << 8) | px[..., 2]


def _patch(h, w):
    """A crop of the raytracer's golden screenshot at (60, 90), wrapping past its 320 x 256."""
    with open(os.path.join(HERE, "rt_screenshot_320x256.bmp"), "rb") as f:
        b = f.read()
    off = int.from_bytes(b[10:14], "little")
    bw, bh, bits = int.from_bytes(b[18:22], "little"), int.from_bytes(b[22:26], "little", signed=True), b[28] | b[29] << 8
    assert (bw, abs(bh), bits) == (320, 256, 32), (bw, bh, bits)
    img = np.frombuffer(b, np.uint8, 320 * 256 * 4, off).reshape(256, 320, 4)
    if bh > 0:
        img = img[::-1]
    y, x = np.mgrid[0:h, 0:w]
    c = img[(60 + y) % 256, (90 + x) % 320]                    # B G R A
    return np.stack([c[..., 2], c[..., 1], c[..., 0], c[..., 3]], -1)


def inputs(h, w, content, colour):
    """uint32 (H, W) ARGB8888.  The colour only matters to "runs" and "fib", which lay out bytes."""
    bpp = 4 if colour == ref.RGBA else 3
    y, x = np.mgrid[0:h, 0:w]
    if content == "zero":
        return np.zeros((h, w), np.uint32)
    if content == "constant":
        return np.full((h, w), 0xC86432FA, np.uint32)
    if content == "hgrad":
        return _pack(np.stack([x * 255 // max(w - 1, 1), x % 256, 255 - x % 256, 128 + x % 128], -1))
    if content == "vgrad":
        return _pack(np.stack([y * 255 // max(h - 1, 1), y % 256, 255 - y % 256, 255 - y % 256], -1))
    if content == "noise":
        return pcg32(h * w, 42 + 131 * h + w).astype(np.uint32).reshape(h, w)
    if content == "nibble":            # 16 values a byte: half the bytes as a dynamic block, no runs to speak of
        v = pcg32(h * w, 7 + 131 * h + w)
        return (((v & np.uint64(0x0F0F0F0F)) * np.uint64(17)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(h, w)
    if content == "patch":
        return _pack(_patch(h, w))
    if content in ("runs", "fib"):
        n = w * bpp
        rows = np.zeros((h, n), np.int64)
        if content == "runs":          # under filter 0: every length of RUNS in every row, then bytes that never repeat
            for r in range(h):
                vals = np.concatenate([np.full(k, (37 * i + 11 * r + 1) % 251 + 1) for i, k in enumerate(RUNS)])
                assert vals.size <= n, "the row is too short for the run pattern"
                rest = (np.arange(n - vals.size) * 7 + r) % 256
                rows[r] = np.concatenate([vals, rest])
        else:
            # Under filter 0 the first band's symbols have exactly the Fibonacci numbers F1 .. F22 as
            # frequencies: the end-of-block is F1 = 1, 21 byte values take F2 .. F22 (value 0 has F8 = 21:
            # the 16 type bytes and 5 more), and 8 more values share the rest of the band evenly.  The
            # bytes are shuffled by a PCG stream; then every run of 4 is broken by a swap with a later
            # byte, since a match would be a symbol outside the Fibonacci numbers -- a Huffman tree is
            # only as deep as its leaves when each frequency exceeds the sum of all smaller ones by 1.
            fibs = [1, 1]
            while len(fibs) < 22:
                fibs.append(fibs[-1] + fibs[-2])
            vals = [3 + 5 * i for i in range(21)]
            vals[6] = 0                                        # F8 = 21
            counts = fibs[1:]
            counts[6] -= 16
            per_band = 16 * n
            assert sum(counts) + 8 * fibs[16] <= per_band, "the band is too short: the other values must outweigh F17"
            band = np.concatenate([np.full(f, v) for v, f in zip(vals, counts)] + [200 + np.arange(per_band - sum(counts)) % 8])
            band = band[np.argsort(pcg32(per_band, 1000 + h + w), kind="stable")].reshape(16, n)
            flat = np.concatenate([np.zeros((16, 1), np.int64), band], 1).reshape(-1)
            for i in range(3, flat.size):
                if flat[i] == flat[i - 1] == flat[i - 2] == flat[i - 3]:
                    j = i + 1
                    while j % (n + 1) == 0 or flat[j] == flat[i]:
                        j += 1
                    flat[i], flat[j] = flat[j], flat[i]
            rows[:16] = flat.reshape(16, n + 1)[:, 1:]
            rows[16:] = rows[:h - 16]
        px = rows.reshape(h, w, bpp)
        if bpp == 3:
            px = np.concatenate([px, np.full((h, w, 1), 255)], -1)
        return _pack(px)
    raise ValueError(content)


def case_name(h, w, content, colour, filt):
    return f"{h}x{w}-{content}-c{colour}-f{'a' if filt == ref.ADAPTIVE else filt}"


def groups():
    """(h, w, colour, filter) -> the contents that are the frames of one device call."""
    out = {}
    for (h, w) in SIZES:
        for colour in COLOURS:
            out[(h, w, colour, ref.ADAPTIVE)] = ["zero", "constant", "hgrad", "vgrad", "noise", "nibble", "patch"]
            if (h, w) in FILTER_SIZES:
                for filt in range(5):
                    out[(h, w, colour, filt)] = ["hgrad", "patch", "nibble"]
            if (h, w) in BIG:
                out[(h, w, colour, 0)] = ["runs", "nibble"] + (["fib"] if (h, w) == FIB_SIZE else [])
    return out


def all_cases():
    for (h, w, colour, filt), contents in groups().items():
        for content in contents:
            yield h, w, content, colour, filt


def accepted(data, argb, colour):
    """The four checks of the docstring; raises where one fails."""
    from PIL import Image
    want = argb if colour == ref.RGBA else argb | np.uint32(0xFF000000)
    got = ref.decode(data)                                     # chunk walk, zlib, un-filtering
    assert np.array_equal(got, want), "zlib and numpy do not return the input"
    im = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA")).astype(np.uint32)
    pil = (im[..., 3] << 24) | (im[..., 0] << 16) | (im[..., 1] << 8) | im[..., 2]
    assert np.array_equal(pil, want), "Pillow does not return the input"


def make():
    out = {}
    for h, w, content, colour, filt in all_cases():
        argb = inputs(h, w, content, colour)
        data, bands = ref.info(argb, colour, filt)
        accepted(data, argb, colour)
        if content == "noise":
            assert all(b["stored"] for b in bands), "noise must take the stored fallback"
        if content == "fib":
            assert bands[0]["depth"] > 15 and not bands[0]["stored"], "the Fibonacci band must run the limiter"
        if content == "nibble" and (h, w) == (20, 900):
            assert not bands[0]["stored"] and bands[0]["dyn_bits"] > 8 * 16384, "the band must outgrow the window"
        out[case_name(h, w, content, colour, filt)] = {
            "h": h, "w": w, "content": content, "colour": colour, "filter": filt, "sha256": hashlib.sha256(data).hexdigest(),
            "length": len(data), "stored_bands": sum(b["stored"] for b in bands), "bands": len(bands)}
    return out


if __name__ == "__main__":
    doc = {"sizes": {f"{h}x{w}": why for (h, w), why in SIZES.items()}, "cases": make()}
    if "--check" in sys.argv:
        with open(PATH) as f:
            old = json.load(f)
        bad = [k for k in doc["cases"] if old["cases"].get(k) != doc["cases"][k]]
        print(f"{len(doc['cases'])} cases, {len(bad)} differ", *bad[:10])
        sys.exit(1 if bad or len(old["cases"]) != len(doc["cases"]) else 0)
    with open(PATH, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(doc['cases'])} cases to {PATH}")
