"""GPU: `raytracer --exr` and `rasteriser --exr`.  The file goes through the independent reader
(tests/exr_enc_ref.py part b): with --exr-type float its R, G, B are the floats of the PFM that
--pfm writes in the same run, bit for bit; halves are numpy's; with --batch every frame of the run
is also written as a numbered file."""
import os
import subprocess

import numpy as np
import pytest

import exr_enc_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "computer-graphics_amd", "_build")
SIZES = {"raytracer": (128, 96, "96"), "rasteriser": (160, 120, "90")}
KEYS = {"raytracer": "dm", "rasteriser": " U"}      # a light move and a yaw; a colour mode 1 frame and a camera move


def _pfm(path, w, h):
    """float32 (H, W, 3) bits, top row first."""
    with open(path, "rb") as f:
        data = f.read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 12
    return np.frombuffer(data, "<u4", w * h * 3, len(head)).reshape(h, w, 3)[::-1]


def _run(app, tmp_path, name, keys, *flags):
    w, h, focal = SIZES[app]
    pfm, exr = str(tmp_path / f"{name}.pfm"), str(tmp_path / f"{name}.exr")
    r = subprocess.run([os.path.join(BUILD, app), "--width", str(w), "--height", str(h), "--focal", focal, "--keys", keys,
                        "--out", str(tmp_path / f"{name}.bmp"), "--pfm", pfm, "--exr", exr, *flags],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with open(exr, "rb") as f:
        return _pfm(pfm, w, h), ref.read(f.read())


def _half(bits):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(bits).view(np.float32).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("app", ["raytracer", "rasteriser"])
def test_float_exr_holds_the_pfm_s_floats(app, tmp_path):
    w, h, _ = SIZES[app]
    pfm, got = _run(app, tmp_path, "float", KEYS[app], "--exr-type", "float")
    assert (got["width"], got["height"], got["type"], got["compression"]) == (w, h, ref.FLOAT, ref.ZIP)
    assert got["names"] == ["A", "B", "G", "R"]
    for c, name in enumerate("RGB"):
        assert np.array_equal(got["planes"][name], pfm[..., c]), name
    a = got["planes"]["A"].view(np.float32)
    assert a.min() >= 0.0 and a.max() == 1.0                       # coverage: w / 9 of the raytracer, 1 inside the rasteriser's border
    pfm, got = _run(app, tmp_path, "plain", KEYS[app], "--exr-colour", "rgb", "--exr-compression", "none")
    assert (got["type"], got["compression"], got["names"]) == (ref.HALF, ref.NONE, ["B", "G", "R"])
    for c, name in enumerate("RGB"):
        assert np.array_equal(got["planes"][name], _half(pfm[..., c])), name


@pytest.mark.parametrize("app", ["raytracer", "rasteriser"])
def test_batch_writes_one_numbered_file_per_frame(app, tmp_path):
    """Frame k of a --batch run is the picture of the run over the first k + 1 keys."""
    keys = KEYS[app]
    first, _ = _run(app, tmp_path, "first", keys[:1], "--batch", "--exr-type", "float")
    last, shot = _run(app, tmp_path, "both", keys, "--batch", "--exr-type", "float")
    assert first.tobytes() != last.tobytes()
    names = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("both."))
    assert names == ["both.0000.exr", "both.0001.exr", "both.bmp", "both.exr", "both.pfm"]
    for k, want in enumerate((first, last)):
        got = ref.read((tmp_path / f"both.{k:04d}.exr").read_bytes())
        for c, name in enumerate("RGB"):
            assert np.array_equal(got["planes"][name], want[..., c]), (k, name)
    assert (tmp_path / "both.0001.exr").read_bytes() == (tmp_path / "both.exr").read_bytes()


def test_bad_values_are_refused(tmp_path):
    for app in ("raytracer", "rasteriser"):
        for flags in (["--exr-type", "double"], ["--exr-compression", "piz"], ["--exr-colour", "grey"], ["--exr"]):
            r = subprocess.run([os.path.join(BUILD, app), "--width", "64", "--height", "48", *flags], capture_output=True,
                               text=True, timeout=120, cwd=str(tmp_path))
            assert r.returncode == 1 and "--exr FILE" in r.stderr, (app, flags)
