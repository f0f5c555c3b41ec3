"""GPU: `raytracer --jpeg` and `rasteriser --jpeg`.  The file is the host encoder's
(cg_image_encode_jpeg_host, held to Pillow's bytes by tests/test_jpeg_encode.py) on the pixels of the
BMP that --out writes in the same run; with --batch it is every frame's file, one after the other."""
import os
import subprocess

import pytest

import cgamd
import make_golden as mg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "computer-graphics_amd", "_build")
SIZES = {"raytracer": (128, 96, "96"), "rasteriser": (160, 120, "90")}
KEYS = {"raytracer": "dm", "rasteriser": " U"}      # a light move and a yaw; a colour mode 1 frame and a camera move


def _run(app, tmp_path, name, keys, *flags):
    w, h, focal = SIZES[app]
    bmp, jpg = str(tmp_path / f"{name}.bmp"), str(tmp_path / f"{name}.jpg")
    r = subprocess.run([os.path.join(BUILD, app), "--width", str(w), "--height", str(h), "--focal", focal, "--keys", keys,
                        "--out", bmp, "--jpeg", jpg, *flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with open(jpg, "rb") as f:
        return mg.screenshot_argb(bmp).reshape(h, w), f.read()


@pytest.mark.parametrize("app", ["raytracer", "rasteriser"])
def test_jpeg_is_the_screenshot_encoded(app, tmp_path):
    argb, data = _run(app, tmp_path, "plain", KEYS[app])
    assert data == cgamd.image_encode_jpeg_host(argb, 75, cgamd.JPEG_420)
    assert cgamd.jpeg_info(data) == (*SIZES[app][:2], 3)
    argb, data = _run(app, tmp_path, "q90", KEYS[app], "--quality", "90", "--subsampling", "444")
    assert data == cgamd.image_encode_jpeg_host(argb, 90, cgamd.JPEG_444)


@pytest.mark.parametrize("app", ["raytracer", "rasteriser"])
def test_batch_is_the_concatenation(app, tmp_path):
    """Frame k of a --batch run is the screenshot of the run over the first k + 1 keys."""
    keys = KEYS[app]
    first, _ = _run(app, tmp_path, "first", keys[:1], "--batch")
    last, stream = _run(app, tmp_path, "both", keys, "--batch", "--quality", "50")
    assert first.tobytes() != last.tobytes()
    assert stream == (cgamd.image_encode_jpeg_host(first, 50, cgamd.JPEG_420) +
                      cgamd.image_encode_jpeg_host(last, 50, cgamd.JPEG_420))


@pytest.mark.parametrize("app", ["raytracer", "rasteriser"])
def test_composes_with_the_exposure_flags(app, tmp_path):
    argb, data = _run(app, tmp_path, "bloom", KEYS[app], "--auto-exposure", "990", "--tonemap", "reinhard", "--bloom",
                      "0.5,0.5")
    assert data == cgamd.image_encode_jpeg_host(argb, 75, cgamd.JPEG_420)


def test_bad_values_are_refused(tmp_path):
    for app in ("raytracer", "rasteriser"):
        for flags in (["--quality", "0"], ["--quality", "101"], ["--subsampling", "422"], ["--jpeg"]):
            r = subprocess.run([os.path.join(BUILD, app), "--width", "64", "--height", "48", *flags], capture_output=True,
                               text=True, timeout=120, cwd=str(tmp_path))
            assert r.returncode == 1 and "--jpeg FILE" in r.stderr, (app, flags)
