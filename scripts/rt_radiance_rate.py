"""What the float format costs beside ARGB: frames/s of cg_rt_render_frames_device in
CG_PIX_ARGB8888 and in CG_PIX_RGBA_F32 on the same build, at 1920 x 1080 on one GPU, for
  c2        the reference scene, the reference light, unrotated (20 frames a call, one launch)
  c2_yaw    the same after one yaw key
  c2_2x2    the same under a 2 x 2 light set
  random_N  cg_rt_random_scene(0x5EED, N) (default N = 1e6; 2 frames a call)
A float frame is 33.2 MB of stores against 8.3 MB.  Per configuration: windows of about one second
of enqueued calls closed by a device synchronise, the two formats alternating, the median of
--repeats windows each, with min and max.  Also the device time of cg_rt_pack_radiance_device on one
frame (HIP events around 50 launches).  Usage:
  python scripts/rt_radiance_rate.py [--repeats 5] [--tris 1000000] [--out profiles/rt_radiance_rate.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "computer-graphics_amd"))
import cgamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_radiance_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

W, H, F = 1920, 1080, 1080.0
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ctx = cgamd.Context(0)
NF = 20
d_out = torch.zeros(NF * W * H * 4, dtype=torch.float32, device=dev)    # either format
d_argb = torch.zeros(W * H, dtype=torch.int32, device=dev)
result = {"workload": f"cg_rt_render_frames_device, {W}x{H}, ARGB8888 against RGBA_F32 on one build",
          "bytes_per_frame": {"argb": W * H * 4, "f32": W * H * 16}, "repeats": args.repeats,
          "window_s": args.window_s, "configs": {}}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def window(call, calls):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def measure(name, cam, lights, frames):
    cams = [cam] * frames
    call = {fmt: (lambda fmt=fmt: ctx.rt_render_frames_device(cams, d_out.data_ptr(), lights=lights, pix_format=fmt))
            for fmt in (cgamd.PIX_ARGB8888, cgamd.PIX_RGBA_F32)}
    calls = {}
    for fmt, fn in call.items():                     # code objects, pools and scratch; then the window's size
        window(fn, 2)
        t = window(fn, 4) / 4
        calls[fmt] = max(2, int(round(args.window_s / t)))
    rate = {fmt: [] for fmt in call}
    for r in range(args.repeats):
        for fmt, fn in call.items():
            rate[fmt].append(calls[fmt] * frames / window(fn, calls[fmt]))
        print(f"{name} repeat {r}: argb {rate[cgamd.PIX_ARGB8888][-1]:.1f} f32 {rate[cgamd.PIX_RGBA_F32][-1]:.1f} frames/s",
              flush=True)
    a, f = rate[cgamd.PIX_ARGB8888], rate[cgamd.PIX_RGBA_F32]
    result["configs"][name] = {
        "frames_per_call": frames, "calls_per_window": {"argb": calls[cgamd.PIX_ARGB8888], "f32": calls[cgamd.PIX_RGBA_F32]},
        "argb_frames_per_s": spread(a), "f32_frames_per_s": spread(f),
        "argb_frame_us": 1e6 / statistics.median(a), "f32_frame_us": 1e6 / statistics.median(f),
        "f32_over_argb_time": statistics.median(a) / statistics.median(f)}


def pack_time():
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, F)], d_out.data_ptr(), pix_format=cgamd.PIX_RGBA_F32)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for r in range(args.repeats + 1):
        e0.record(s)
        for _ in range(50):
            ctx.rt_pack_radiance_device(d_out.data_ptr(), W * H, d_argb.data_ptr(), 1.0, stream=s.cuda_stream)
        e1.record(s)
        s.synchronize()
        ms.append(e0.elapsed_time(e1) / 50)
    ms = ms[1:]                                      # the first round loads the code object
    us = 1e3 * statistics.median(ms)
    result["pack_radiance"] = {"us_per_frame": spread([1e3 * m for m in ms]), "bytes": W * H * 20,
                               "gb_per_s": W * H * 20 / (us * 1e-6) / 1e9}


try:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    one = cgamd.default_lights()
    measure("c2", cgamd.rt_camera(W, H, F), one, NF)
    yaw = float(np.float32(0.0) - np.float32(0.174533))
    measure("c2_yaw", cgamd.rt_camera(W, H, F, R=cgamd.yaw_matrix(yaw)), one, NF)
    measure("c2_2x2", cgamd.rt_camera(W, H, F), cgamd.area_lights(None, 0.1, 2), NF)
    pack_time()
    big = torch.from_numpy(np.frombuffer(cgamd.random_scene(args.tris), np.float32).reshape(args.tris, 19).copy()).to(dev)
    ctx.rt_set_scene_device(big.data_ptr(), args.tris)
    measure(f"random_{args.tris}", cgamd.rt_camera(W, H, F), one, 2)
finally:
    ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
