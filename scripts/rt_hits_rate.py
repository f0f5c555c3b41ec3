"""What a frame of hit planes costs beside a rendered frame: cg_rt_hits_device (centre sub-ray, all
three planes) against cg_rt_render_device (the reference light) on the same build, at 1920 x 1080,
on the reference scene (28 triangles and the sphere: rt_hits_small_kernel) and on
cg_rt_random_scene(0x5EED, 1e6) (a hits-only pass of the binned path).
Per scene: windows of --calls enqueued calls closed by a stream synchronise, the two calls
alternating, the median of --repeats windows each, with min and max.  For the large scene also the
device time per call of the pass, its walk and its gather, and of the frame and its walk, through
cg_kernel_timing; and the wall time of one cg_rt_pick (median of 20).  The expectation to confirm or
refute: the large scene's call costs about the frame's certificate and list passes plus a walk of
one ray per pixel.  Usage:
  python scripts/rt_hits_rate.py [--repeats 3] [--tris 1000000] [--out profiles/rt_hits_rate.json]"""
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
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_hits_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

W, H, F = 1920, 1080, 1080.0
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ctx = cgamd.Context(0)
cam = cgamd.rt_camera(W, H, F)
lights = cgamd.default_lights()
d_out = torch.zeros(W * H, dtype=torch.int32, device=dev)
d_rec = torch.zeros(W * H * 28, dtype=torch.uint8, device=dev)
d_idx = torch.zeros(W * H, dtype=torch.int32, device=dev)
d_dst = torch.zeros(W * H, dtype=torch.float32, device=dev)
result = {"workload": f"cg_rt_hits_device (sub-ray 4, three planes) against cg_rt_render_device, {W}x{H}",
          "repeats": args.repeats, "scenes": {}}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def hits():
    ctx.rt_hits_device(cam, 4, None, d_rec.data_ptr(), d_idx.data_ptr(), d_dst.data_ptr())


def render():
    ctx.rt_render_device(cam, d_out.data_ptr(), lights=lights)


def window(fn, calls):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize(dev)
    return calls / (time.perf_counter() - t0)


def measure(name, calls, large):
    for fn in (hits, render, hits, render):          # code objects, pools and scratch of both calls
        fn()
    torch.cuda.synchronize(dev)
    r_hits, r_render = [], []
    for r in range(args.repeats):
        r_hits.append(window(hits, calls))
        r_render.append(window(render, calls))
        print(f"{name} repeat {r}: hits {r_hits[-1]:.1f} /s, render {r_render[-1]:.1f} /s", flush=True)
    idx = d_idx.cpu().numpy()
    rec = {"calls_per_window": calls, "hits_per_s": spread(r_hits), "frames_per_s": spread(r_render),
           "hits_ms": 1e3 / statistics.median(r_hits), "frame_ms": 1e3 / statistics.median(r_render),
           "hits_over_frame_time": statistics.median(r_render) / statistics.median(r_hits),
           "pixels_hit": int((idx != cgamd.HIT_NONE).sum())}
    if large:
        names = ("rt_hits_pass", "rt_hits_walk", "rt_hits_gather", "rt_big_frame", "rt_big_primary_kernel",
                 "rt_shadow_hints_kernel")
        cgamd.kernel_timing(True)
        for _ in range(calls):
            hits()
            render()
        torch.cuda.synchronize(dev)
        per = {}
        for k in names:
            ms, busy, n = cgamd.kernel_time(k)
            per[k] = {"ms_per_call": ms / max(n, 1), "launches": n}
        cgamd.kernel_timing(False)
        rec["device_ms"] = per
        # the pass without its walk and gather is the certificate and list passes, which a frame runs too
        rec["hits_lists_ms"] = per["rt_hits_pass"]["ms_per_call"] - per["rt_hits_walk"]["ms_per_call"] - \
            per["rt_hits_gather"]["ms_per_call"]
        info = ctx.rt_scratch_info()
        rec["scratch"] = {k: int(v) for k, v in info.items()}
    t = []
    for k in range(20):
        x, y = (W // 2 + 37 * k) % W, (H // 2 + 11 * k) % H
        t0 = time.perf_counter()
        ctx.rt_pick(cam, x, y, 4)
        t.append(1e3 * (time.perf_counter() - t0))
    rec["pick_ms"] = spread(t[1:])
    result["scenes"][name] = rec


try:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    measure("reference_28_triangles_and_sphere", 200, False)
    big = torch.from_numpy(np.frombuffer(cgamd.random_scene(args.tris), np.float32).reshape(args.tris, 19).copy()).to(dev)
    ctx.rt_set_scene_device(big.data_ptr(), args.tris)
    measure(f"random_{args.tris}_triangles", 20, True)
finally:
    ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
