"""Writes tests/golden/jpeg_cases.npz and tests/golden/jpeg_san/*.jpg (needs Pillow):

  python tests/golden/make_jpeg_cases.py

For each Pillow-encoded case (tests/jpeg_cases.py pillow_case_params) the file's bytes, and
for each of those and of the synthetic cases in which no component is scaled, the SHA-256
of what libjpeg 9 decodes it to -- derived from Pillow (libjpeg-turbo), whose entropy
decoder and islow 8x8 IDCT are bit-identical to libjpeg 9's:
  one component     Pillow's mode L
  YCbCr files       Pillow's raw YCbCr planes (draft) through jdcolor9(), libjpeg 9's own
                    colour constants (turbo's differ in G by 1 at scattered pixels)
  RGB files         Pillow's RGB (no conversion), swapped to BGR
Which of the last two a three-component file is, is Pillow's (libjpeg's
default_decompress_parms) decision, not this script's.  The 4:2:0 files carry no hash:
libjpeg 9 scales their chroma in the IDCT, turbo upsamples it.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_cases as jc  # noqa: E402


def pillow_expected(data):
    """What libjpeg 9 makes of the file `data` (no scaled component), derived from Pillow:
    uint8 (H, W) gray or (H, W, 3) BGR."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if im.mode == "L":
        return np.asarray(im)
    assert im.mode == "RGB", im.mode
    rgb = np.asarray(im)
    ycc = Image.open(io.BytesIO(data))
    ycc.draft("YCbCr", None)
    try:
        ycc.load()
    except OSError:
        # the file's own colour space is RGB: libjpeg converts nothing (and refuses RGB -> YCbCr)
        return np.ascontiguousarray(rgb[..., ::-1])
    assert ycc.mode == "YCbCr"
    out = jc.jdcolor9(np.asarray(ycc))
    assert np.abs(out[..., ::-1].astype(int) - rgb.astype(int)).max() <= 1     # turbo's own constants
    return out


def source_image(w, h, colour):
    """A smooth field with some noise and a few saturated pixels, deterministic per size."""
    rng = np.random.default_rng(1000 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    ch = []
    for k in range(3 if colour else 1):
        f = 128 + 90 * np.sin((x * (k + 1) + 2 * y) / 7.0 + k) + 40 * np.cos(y / (3.0 + k)) + rng.normal(0, 12, (h, w))
        ch.append(f)
    a = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    a[rng.random((h, w)) < 0.03] = 255
    a[rng.random((h, w)) < 0.03] = 0
    return a if colour else a[..., 0]


def pillow_encode(size, mode, progressive, restart, qkind):
    from PIL import Image
    w, h = size
    im = Image.fromarray(source_image(w, h, mode != "gray"))
    kw = dict(quality=35, optimize=True) if qkind == "q35opt" else dict(quality=100)
    if mode != "gray":
        kw["subsampling"] = 0 if mode == "444" else 2
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", progressive=progressive, **kw)
    return buf.getvalue()


# a handful of baseline / restart files as plain .jpg for the stand-alone sanitizer programs
SAN_FILES = ["pil_gray_base_r1_q35opt_33x31", "pil_444_base_r3_q100_17x15", "pil_420_base_r1_q35opt_65x40",
             "pil_420_prog_r3_q35opt_33x31", "rst1_420_ni_65x40", "perscan_444_r3_65x40", "clamp_420_65x40",
             "gray_declared_2x2_r2_17x15"]


def main():
    names, hashes, blobs = [], [], []
    for name, size, mode, prog, r, qk in jc.pillow_case_params():
        data = pillow_encode(size, mode, prog, r, qk)
        names.append(name)
        blobs.append(data)
        hashes.append("" if mode == "420" else jc.sha(pillow_expected(data)))
    syn = jc.synthetic_cases()
    syn_hashes = ["" if c.any_scaled else jc.sha(pillow_expected(c.jpeg)) for c in syn]
    offsets = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    np.savez_compressed(jc.FIXTURE, blob=np.frombuffer(b"".join(blobs), np.uint8), offsets=offsets,
                        names=np.array(names), hashes=np.array(hashes), syn_names=np.array([c.name for c in syn]),
                        syn_sha=np.array([jc.sha(np.frombuffer(c.jpeg, np.uint8)) for c in syn]),
                        syn_hashes=np.array(syn_hashes))
    os.makedirs(jc.SAN_DIR, exist_ok=True)
    files = dict(zip(names, blobs))
    files.update({c.name: c.jpeg for c in syn})
    for n in SAN_FILES:
        with open(os.path.join(jc.SAN_DIR, n + ".jpg"), "wb") as f:
            f.write(files[n])
    print(f"{len(names)} Pillow files ({offsets[-1]} bytes, {sum(bool(x) for x in hashes)} hashed), "
          f"{len(syn)} synthetic ({sum(bool(x) for x in syn_hashes)} hashed) -> "
          f"{os.path.getsize(jc.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
