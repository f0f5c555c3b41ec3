"""Regenerates tests/golden/exr_enc_cases.json: per case of the EXR encoder's tests, the SHA-256 and
the length of the file the numpy restatement (tests/exr_enc_ref.py, part a) writes -- hashes only.
A case is recorded only if the reader of part b, which shares nothing with it (struct, zlib and
numpy from the OpenEXR file layout), accepts the file and returns the input: FLOAT samples bit for
bit, HALF samples equal to numpy's astype(float16).  The inputs come from inputs() below, integer
recurrences and exact float32 operations, so the tests rebuild them.

    python tests/golden/make_exr_enc_cases.py            # rewrite the JSON
    python tests/golden/make_exr_enc_cases.py --check    # compare with the committed JSON
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import exr_enc_ref as ref  # noqa: E402
from make_png_enc_cases import pcg32  # noqa: E402

PATH = os.path.join(HERE, "exr_enc_cases.json")
PIECE = 1024       # bytes of a chunk its workgroup takes at a time (cg_image_exr_enc_limits; the tests assert it)
WINDOW = 16384     # bytes of a chunk's bit string the workgroup holds in LDS

# (H, W): what the size catches
SIZES = {
    (1, 1): "one sample a channel: every ZIP chunk falls back to raw",
    (1, 2): "one scanline, two samples",
    (15, 3): "one short chunk",
    (16, 3): "exactly one chunk",
    (17, 5): "one scanline over a chunk",
    (33, 7): "three chunks, the last of one scanline",
    (18, 7): "a 16-line RGBA half chunk is 896 bytes: just under a piece of 1024",
    (18, 9): "a 16-line RGBA half chunk is 1152 bytes: it crosses a piece",
    (40, 65): "three chunks of several pieces, the middle one able to stay raw between deflated ones",
    (20, 900): "a chunk's dynamic block is longer than the 16,384 bytes of its bit string a workgroup holds",
    (17, 1400): "a 16-line RGBA float chunk is 358,400 bytes, more than 65,535",
}
BIG = ((20, 900), (17, 1400))
FULL = ((17, 5), (33, 7))                      # the sizes that run both types, compressions and channel sets
DEFAULT = (ref.RGBA, ref.HALF, ref.ZIP)
ALL_CONTENTS = ["zero", "constant", "hgrad", "vgrad", "noise", "specials", "patch"]
PATCH_ALPHA = 1.0 / 9.0                        # the raytracer app's scale for its w of 0 .. 9

# rule 1's table, then +-0, +-inf, NaNs with high and low payloads, float subnormals, the range of
# half subnormals with its ties, values around 65504 and 65520, ties of normal halves
SPECIALS = np.array([
    0x7F800001, 0x7FC00000, 0x477FEFFF, 0x477FF000, 0x33000000, 0x33000001, 0x387FC000, 0x3F801000, 0x3F803000,
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0xFFC12345, 0x7F801FFF, 0xFF802000, 0x7FFFFFFF,
    0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00800000,
    0x33800000, 0x33C00000, 0x34200000, 0x38000000, 0x387FE000, 0x387FDFFF, 0x387FF000, 0x38800000, 0xB8800FFF,
    0x477FE000, 0x477FE001, 0x477FFFFF, 0x47800000, 0xC77FF000, 0xC77FEFFF, 0x3F800000, 0x3F802000, 0x3F802001,
    0xBF801000, 0x3F800FFF, 0x40490FDB], np.uint32)
assert SPECIALS.size % 2 == 1                  # odd: every component of a pixel meets every value


def inputs(h, w, content, typ=ref.HALF):
    """float32 (H, W, 4).  The type only matters to the noise: bits that are noise as the file stores them."""
    y, x = np.mgrid[0:h, 0:w]
    one = np.ones((h, w), np.float32)
    if content == "zero":
        return np.zeros((h, w, 4), np.float32)
    if content == "constant":
        return np.stack([0.25 * one, 0.5 * one, 1.5 * one, 9.0 * one], -1)
    if content == "hgrad":
        g = x.astype(np.float32) / np.float32(max(w - 1, 1))
        return np.stack([g, np.float32(1) - g, g * np.float32(4), (x % 10).astype(np.float32)], -1)
    if content == "vgrad":
        g = y.astype(np.float32) / np.float32(max(h - 1, 1))
        return np.stack([g, np.float32(1) - g, g * np.float32(4), (y % 10).astype(np.float32)], -1)
    if content == "noise":
        v = pcg32(h * w * 4, 42 + 131 * h + w).astype(np.uint32)
        if typ == ref.HALF:                    # every half, widened: the conversion gives these 16 bits back
            v = np.ascontiguousarray((v & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float32)).view(np.uint32)
            # widening quiets a signalling NaN on some hosts: rebuild those from the half's bits
            hb = (pcg32(h * w * 4, 42 + 131 * h + w).astype(np.uint32) & np.uint32(0xFFFF))
            nan = ((hb & 0x7C00) == 0x7C00) & ((hb & 0x3FF) != 0)
            v = np.where(nan, ((hb & 0x8000) << 16) | 0x7F800000 | ((hb & 0x3FF) << 13), v).astype(np.uint32)
        return v.view(np.float32).reshape(h, w, 4)
    if content == "mixed":                     # scanlines 16 .. 31 noise between smooth chunks
        px = inputs(h, w, "hgrad", typ).copy()
        px[16:32] = inputs(h, w, "noise", typ)[16:32]
        return px
    if content == "specials":
        idx = (4 * (y * w + x))[..., None] + np.arange(4)
        return SPECIALS[idx % SPECIALS.size].view(np.float32)
    if content == "patch":                     # shading with texture in the low bits, a spot beyond half's range, w in 0 .. 9
        base = ((x * 13 + y * 7) % 64).astype(np.float32) / np.float32(64) + ((x * x + 3 * y) % 7).astype(np.float32) / np.float32(1024)
        spot = (x - w // 2) ** 2 + (y - h // 2) ** 2 <= (min(h, w) // 4) ** 2
        r = np.where(spot, np.float32(1e5), base)
        g = np.where(spot, np.float32(40.0), base * np.float32(0.5))
        b = np.where(spot, np.float32(65519.0), np.float32(1) - base)
        return np.stack([r, g, b, ((x + 2 * y) % 10).astype(np.float32)], -1).astype(np.float32)
    raise ValueError(content)


def alpha_of(content):
    return PATCH_ALPHA if content == "patch" else 1.0


def case_name(h, w, content, channels, typ, comp):
    return f"{h}x{w}-{content}-{'rgba' if channels == ref.RGBA else 'rgb'}-{'half' if typ == ref.HALF else 'float'}-" \
           f"{'zip' if comp == ref.ZIP else 'none'}"


def groups():
    """(h, w, channels, type, compression) -> the contents that are the frames of one device call."""
    out = {}
    for (h, w) in SIZES:
        contents = ["zero", "hgrad", "noise", "patch"] if (h, w) in BIG else ALL_CONTENTS + (["mixed"] if h >= 40 else [])
        out[(h, w) + DEFAULT] = contents
        if (h, w) in FULL:
            for ch in (ref.RGB, ref.RGBA):
                for typ in (ref.HALF, ref.FLOAT):
                    for comp in (ref.NONE, ref.ZIP):
                        out[(h, w, ch, typ, comp)] = contents
    out[(17, 1400, ref.RGBA, ref.FLOAT, ref.ZIP)] = ["hgrad", "noise", "patch"]
    return out


def all_cases():
    for (h, w, ch, typ, comp), contents in groups().items():
        for content in contents:
            yield h, w, content, ch, typ, comp


def accepted(data, px, ch, typ, comp, alpha):
    """The reader's checks and the samples it returns; raises where one fails.  -> the reader's record."""
    got = ref.read(data)
    assert (got["height"], got["width"]) == px.shape[:2] and got["type"] == typ and got["compression"] == comp
    want = ref.expected_planes(px, ch, typ, alpha)
    assert sorted(got["planes"]) == sorted(want)
    for k, v in want.items():
        assert np.array_equal(got["planes"][k], v), f"channel {k}: the reader does not return the input"
    return got


def make():
    out = {}
    for h, w, content, ch, typ, comp in all_cases():
        px = inputs(h, w, content, typ)
        alpha = alpha_of(content)
        data, notes = ref.info(px, ch, typ, comp, alpha)
        is_raw = [c["raw"] for c in notes]
        got = accepted(data, px, ch, typ, comp, alpha)
        if comp == ref.ZIP:
            assert got["raw_chunks"] == sum(is_raw)
            if content == "noise" or (h, w) == (1, 1):
                assert all(is_raw), "noise and a single sample must take the raw fallback"
            if content == "mixed":
                assert is_raw == [False, True, False], "a raw chunk between deflated ones"
            if (h, w) == (20, 900) and content == "patch":
                assert not is_raw[0] and notes[0]["bytes"] > WINDOW, "the chunk's stream must outgrow the window"
        out[case_name(h, w, content, ch, typ, comp)] = {
            "h": h, "w": w, "content": content, "channels": ch, "type": typ, "compression": comp,
            "sha256": hashlib.sha256(data).hexdigest(), "length": len(data), "raw_chunks": int(sum(is_raw)) if comp == ref.ZIP else 0,
            "chunks": len(is_raw)}
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
