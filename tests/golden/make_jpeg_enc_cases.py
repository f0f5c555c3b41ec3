"""Regenerates tests/golden/jpeg_enc_cases.json: per case of the JPEG encoder's tests, the SHA-256
and the length of the file Pillow writes (needs Pillow; the GPU machine may not have it, so
Pillow's bytes travel as hashes).  The inputs come from inputs() below, an explicit integer
recurrence, so the tests rebuild them without this script's dependencies.

    python tests/golden/make_jpeg_enc_cases.py            # rewrite the JSON
    python tests/golden/make_jpeg_enc_cases.py --check    # compare with the committed JSON
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "jpeg_enc_cases.json")

# (H, W): what the size catches
SIZES = {
    (1, 1): "everything is padding",
    (2, 3): "everything is padding, odd width",
    (8, 8): "exactly one 4:4:4 MCU",
    (16, 16): "exactly one 4:2:0 MCU",
    (9, 24): "a bottom edge one row into an MCU",
    (17, 33): "edges in both directions; odd chroma width",
    (31, 15): "edges one short of the MCU; odd chroma width",
    (20, 35): "4:2:0: dummy Y blocks on the right and at the bottom",
    (88, 24): "4:4:4: 11 MCU rows, the RST number wraps past 7",
    (150, 40): "4:2:0: 10 MCU rows, the RST number wraps past 7",
    (16, 1100): "4:4:4: 414 blocks in one restart interval",
}
CONTENTS = ("random", "gradient", "noise", "constant")
QUALITIES = (1, 10, 50, 75, 90, 100)
SUBSAMPLINGS = (0, 2)


def lcg(n, seed):
    """x_{k+1} = (1103515245 x_k + 12345) mod 2^32 from x_0 = seed: x_1 .. x_n.  Built by doubling --
    x_{k+m} = A_m x_k + C_m with (A_2m, C_2m) = (A_m^2, A_m C_m + C_m) -- which is the recurrence itself."""
    mask = (1 << 32) - 1
    x = np.array([(1103515245 * seed + 12345) & mask], np.uint64)
    a, c = 1103515245, 12345
    while x.size < n:
        x = np.concatenate([x, (x * np.uint64(a) + np.uint64(c)) & np.uint64(mask)])
        a, c = (a * a) & mask, (a * c + c) & mask
    return x[:n]


def inputs(h, w, content):
    """uint32 (H, W) ARGB8888, alpha 255."""
    n = h * w * 3
    if content == "random":            # bits 16-23 of the recurrence
        rgb = ((lcg(n, 20241 + 131 * h + w) >> np.uint64(16)) & np.uint64(255)).reshape(h, w, 3)
    elif content == "noise":           # 0 or 255 by bit 20: long codes, FF bytes, runs of zeros at low quality
        rgb = (((lcg(n, 977 + 131 * h + w) >> np.uint64(20)) & np.uint64(1)) * np.uint64(255)).reshape(h, w, 3)
    elif content == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        rgb = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1)
    elif content == "constant":        # EOB only, DC difference 0 after the first block
        rgb = np.empty((h, w, 3), np.int64)
        rgb[:] = (200, 100, 50)
    else:
        raise ValueError(content)
    rgb = rgb.astype(np.uint32)
    return np.uint32(0xFF000000) | (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]


def case_name(h, w, content, quality, sub):
    return f"{h}x{w}-{content}-q{quality}-s{sub}"


def all_cases():
    for (h, w) in SIZES:
        for content in CONTENTS:
            for q in QUALITIES:
                for sub in SUBSAMPLINGS:
                    yield h, w, content, q, sub


def rgb_of(argb):
    return np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255], -1).astype(np.uint8)


def pillow_bytes(argb, quality, sub):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(rgb_of(argb)).save(f, format="JPEG", quality=quality, subsampling=sub, restart_marker_rows=1)
    return f.getvalue()


def make():
    out = {}
    for h, w, content, q, sub in all_cases():
        data = pillow_bytes(inputs(h, w, content), q, sub)
        out[case_name(h, w, content, q, sub)] = {"h": h, "w": w, "content": content, "quality": q, "subsampling": sub,
                                                 "sha256": hashlib.sha256(data).hexdigest(), "length": len(data)}
    return out


if __name__ == "__main__":
    import PIL
    doc = {"pillow": PIL.__version__, "sizes": {f"{h}x{w}": why for (h, w), why in SIZES.items()}, "cases": make()}
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
