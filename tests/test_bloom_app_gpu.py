"""GPU: raytracer / rasteriser --bloom.  The BMP is the last frame of the library's exposed call with
bloom over the globals the key script leaves; without the flag the apps write today's BMPs."""
import os
import subprocess

import numpy as np
import pytest

import cgamd
import hdr_ref as ref
import make_golden as mg
import rt_seq_states as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "computer-graphics_amd", "_build")
W, H = 160, 128
f32 = lambda x: float(np.float32(x))   # noqa: E731


def _run(app, args, out):
    r = subprocess.run([os.path.join(BUILD, app), *args, "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _scales(stdout):
    return [float(line.split(":")[1]) for line in stdout.splitlines() if line.startswith("Exposure scale")]


SIZE = ["--width", str(W), "--height", str(H)]
EXPOSED = ["--auto-exposure", "990", "--tonemap", "reinhard"]


def test_raytracer_app_writes_the_bloomed_frame(ctx, tmp_path):
    out, plain = str(tmp_path / "bloom.bmp"), str(tmp_path / "exposed.bmp")
    stdout = _run("raytracer", ["--keys", "Ud", *SIZE, *EXPOSED, "--bloom", "1,0.25"], out)
    _run("raytracer", ["--keys", "Ud", *SIZE, *EXPOSED], plain)
    states = S.key_states(["U", "d"], 256.0)                     # the app's globals at each of the two frames
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    cams = [S.camera(st, W, H) for st in states]
    lights = [S.light_array(st.lights()) for st in states]
    frames, scales = ctx.rt_render_exposed_bloom(cams, cgamd.hdr_bloom_params(4, 1.0, 64.0, 0.25), lights, True,
                                                 permille=990, op=ref.TONE_REINHARD)
    assert np.array_equal(mg.screenshot_argb(out), frames[-1].reshape(-1))
    assert np.allclose(_scales(stdout), scales, rtol=1e-5, atol=0) and len(_scales(stdout)) == 2
    without, _ = ctx.rt_render_exposed(cams, lights, True, permille=990, op=ref.TONE_REINHARD)
    assert np.array_equal(mg.screenshot_argb(plain), without[-1].reshape(-1))
    assert (frames[-1] != without[-1]).any()                      # not the frame without bloom
    # levels and cap given; --bloom alone: every scale is 1
    stdout = _run("raytracer", ["--keys", "Ud", *SIZE, "--bloom", "0.5,0.5,2,8"], out)
    frames, scales = ctx.rt_render_exposed_bloom(cams, cgamd.hdr_bloom_params(2, 0.5, 8.0, 0.5), lights, True,
                                                 scale_min=1.0, scale_max=1.0)
    assert np.array_equal(mg.screenshot_argb(out), frames[-1].reshape(-1))
    assert _scales(stdout) == [1.0, 1.0] and (scales == 1.0).all()


def test_rasteriser_app_writes_the_bloomed_frame(ctx, tmp_path):
    out, plain = str(tmp_path / "bloom.bmp"), str(tmp_path / "exposed.bmp")
    focal = ["--focal", "96"]
    stdout = _run("rasteriser", ["--keys", "Ud", *SIZE, *focal, *EXPOSED, "--bloom", "1,0.25"], out)
    _run("rasteriser", ["--keys", "Ud", *SIZE, *focal, *EXPOSED], plain)
    # the app's globals at the two frames of the keys "Ud": camera forward, then the light to the right;
    # Draw leaves indirectLightPowerPerArea at 0.2 after the first mode-0 frame
    z = f32(np.float32(-3.001) + np.float32(0.1))
    lx = f32(np.float32(0.0) + np.float32(0.1))
    ps = [cgamd.rast_params(W, H, 96.0, cam=(0.0, 0.0, z, 1.0), indirect_first=f32(0.15)),
          cgamd.rast_params(W, H, 96.0, cam=(0.0, 0.0, z, 1.0), light=(lx, -0.5, 0.0, 1.0), indirect_first=f32(0.2))]
    ctx.rast_set_scene()
    frames, scales, _, rc = ctx.rast_draw_exposed_bloom(ps, cgamd.hdr_bloom_params(4, 1.0, 64.0, 0.25), permille=990,
                                                        op=ref.TONE_REINHARD)
    assert rc == cgamd.CG_OK
    assert np.array_equal(mg.screenshot_argb(out), frames[-1].reshape(-1))
    assert np.allclose(_scales(stdout), scales, rtol=1e-5, atol=0) and len(_scales(stdout)) == 2
    without, _, _, _ = ctx.rast_draw_exposed(ps, permille=990, op=ref.TONE_REINHARD)
    assert np.array_equal(mg.screenshot_argb(plain), without[-1].reshape(-1))
    assert (frames[-1] != without[-1]).any()                      # not the frame without bloom


def test_apps_without_the_flag_are_unchanged(ctx, tmp_path):
    out = str(tmp_path / "plain.bmp")
    _run("rasteriser", ["--keys", "U", "--width", "70", "--height", "50", "--focal", "40"], out)
    ctx.rast_set_scene()
    z = f32(np.float32(-3.001) + np.float32(0.1))
    want = ctx.rast_draw(cgamd.rast_params(70, 50, 40.0, cam=(0.0, 0.0, z, 1.0), indirect_first=f32(0.15)))[0]
    assert np.array_equal(mg.screenshot_argb(out), want)          # today's screenshot: cg_rast_draw's frame
    stdout = _run("raytracer", ["--keys", "U"], out)
    with open(out, "rb") as f, open(os.path.join(ROOT, "tests", "golden", "rt_screenshot_320x256.bmp"), "rb") as g:
        assert f.read() == g.read()
    assert "Exposure scale" not in stdout
    r = subprocess.run([os.path.join(BUILD, "raytracer"), "--bloom", "1,2,3,4,5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--bloom" in r.stderr
    r = subprocess.run([os.path.join(BUILD, "rasteriser"), "--keys", "U", "--bloom"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--bloom" in r.stderr            # the flag without its value
