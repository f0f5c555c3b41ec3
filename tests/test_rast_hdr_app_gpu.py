"""GPU: rasteriser --auto-exposure / --tonemap / --pfm.  The BMP is the run's last frame exposed and
tone mapped, the library call's last frame; the PFM is cg_rast_draw_picture of the globals the key
script leaves.  Without the flags the app writes today's screenshot."""
import os
import subprocess

import numpy as np
import pytest

import cgamd
import hdr_ref as ref
import make_golden as mg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "computer-graphics_amd", "_build", "rasteriser")
W, H, FOCAL = 70, 50, 40.0
f32 = lambda x: float(np.float32(x))   # noqa: E731


def _run(args, out):
    r = subprocess.run([APP, "--width", str(W), "--height", str(H), "--focal", str(int(FOCAL)), *args, "--out", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _frames():
    """The app's globals at the three frames of the keys "U d": camera forward, colour mode 1, light
    to the right.  Draw leaves indirectLightPowerPerArea at 0.2 after the first mode-0 frame (:585)."""
    z = f32(np.float32(-3.001) + np.float32(0.1))
    lx = f32(np.float32(0.0) + np.float32(0.1))
    return [cgamd.rast_params(W, H, FOCAL, cam=(0.0, 0.0, z, 1.0), indirect_first=f32(0.15)),
            cgamd.rast_params(W, H, FOCAL, cam=(0.0, 0.0, z, 1.0), indirect_first=f32(0.2), colour_mode=1),
            cgamd.rast_params(W, H, FOCAL, cam=(0.0, 0.0, z, 1.0), light=(lx, -0.5, 0.0, 1.0), indirect_first=f32(0.2),
                              colour_mode=1)]


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(v) for v in f.readline().split())
        assert f.readline() == b"-1.0\n"
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1]      # rows are bottom-up


@pytest.mark.parametrize("flags, permille, target, op, white2", [
    (["--auto-exposure", "990", "--tonemap", "reinhard"], 990, 1.0, ref.TONE_REINHARD, 1.0),
    (["--auto-exposure", "500,0.5", "--tonemap", "reinhard-white:3"], 500, 0.5, ref.TONE_REINHARD_WHITE, 9.0),
])
def test_rasteriser_app_writes_the_exposed_frame(ctx, tmp_path, flags, permille, target, op, white2):
    out, pfm = str(tmp_path / "exposed.bmp"), str(tmp_path / "last.pfm")
    stdout = _run(["--keys", "U d", *flags, "--pfm", pfm], out)
    ctx.rast_set_scene()
    frames, scales, info, rc = ctx.rast_draw_exposed(_frames(), permille=permille, target=target, op=op, white2=white2)
    assert rc == cgamd.CG_OK
    assert np.array_equal(mg.screenshot_argb(out), frames[-1].reshape(-1))
    printed = [float(line.split(":")[1]) for line in stdout.splitlines() if line.startswith("Exposure scale")]
    assert len(printed) == 3
    assert np.allclose(printed, scales, rtol=1e-5, atol=0)        # the stream's six significant digits
    last = _frames()[-1]
    last.rand_offset = int(info["rand_offset"][2])
    assert last.rand_offset > 0                                   # frame 1 drew rand() values
    pic, _ = ctx.rast_draw_picture(last)
    got = _read_pfm(pfm)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(pic[..., :3]).view(np.uint32))
    assert (frames[-1].reshape(-1) != ctx.rast_draw(last)[0]).any()   # not the plain frame


def test_rasteriser_app_pfm_alone_and_without_the_flags(ctx, tmp_path):
    plain, with_pfm, pfm = str(tmp_path / "plain.bmp"), str(tmp_path / "pfm.bmp"), str(tmp_path / "frame.pfm")
    stdout = _run(["--keys", "U"], plain)
    assert "Exposure scale" not in stdout
    _run(["--keys", "U", "--pfm", pfm], with_pfm)
    ctx.rast_set_scene()
    p = _frames()[0]
    want = ctx.rast_draw(p)[0]
    assert np.array_equal(mg.screenshot_argb(plain), want)        # today's screenshot: cg_rast_draw's frame
    with open(plain, "rb") as f, open(with_pfm, "rb") as g:
        assert f.read() == g.read()                               # --pfm leaves the BMP alone
    pic, _ = ctx.rast_draw_picture(p)
    assert np.array_equal(_read_pfm(pfm).view(np.uint32), np.ascontiguousarray(pic[..., :3]).view(np.uint32))
