"""GPU: `rasteriser --batch` -- Update() over the whole key script, then one cg_rast_draw_sequence
call -- writes the BMP the per-frame app writes, byte for byte: colour modes (the rand() chain),
camera and light keys, the indirect keys around the 0.15 -> 0.2 rewrite, yaw."""
import os
import subprocess

import numpy as np
import pytest

import make_golden as mg
import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "computer-graphics_amd", "_build", "rasteriser")
SIZE = ["--width", "320", "--height", "240", "--focal", "180"]


def _run(keys, tmp_path, batch):
    out = str(tmp_path / ("batch.bmp" if batch else "frames.bmp"))
    # the flag first: a parser that took it for an option with a value would misread the rest
    r = subprocess.run([APP] + (["--batch"] if batch else []) + [*SIZE, "--keys", keys, "--out", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with open(out, "rb") as f:
        return out, f.read()


@pytest.mark.parametrize("keys", [" U ", "Ud", "1 2m", "2 U 1n "])
def test_batch_writes_the_per_frame_bmp(tmp_path, keys):
    out, got = _run(keys, tmp_path, True)
    assert got == _run(keys, tmp_path, False)[1]
    if keys != " U ":
        return
    # the oracle's frame, as tests/test_host_apps.py::test_rasteriser_app_colour_modes computes it
    f32 = lambda x: float(np.float32(x))   # noqa: E731
    ind, off = f32(0.15), 0
    cams = [-3.001, f32(np.float32(-3.001) + np.float32(0.1)), f32(np.float32(-3.001) + np.float32(0.1))]
    for mode, z in zip((1, 1, 2), cams):
        p = oracle.rast_params(320, 240, 180.0, (0.0, 0.0, f32(z), 1.0), indirect_first=ind, colour_mode=mode,
                               rand_offset=off)
        ref, _, _, cnt = oracle.rast_draw(p, counters=True)
        off += 3 * cnt.n_shaded
    assert np.array_equal(mg.screenshot_argb(out), ref)


def test_batch_flag_last(tmp_path):
    out = str(tmp_path / "last.bmp")
    r = subprocess.run([APP, *SIZE, "--keys", "Ud", "--out", out, "--batch"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    with open(out, "rb") as f:
        assert f.read() == _run("Ud", tmp_path, True)[1]
