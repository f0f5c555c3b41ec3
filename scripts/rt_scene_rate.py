"""What installing a large raytracer scene costs: cg_rt_set_scene from a host array against
cg_rt_set_scene_device from a device copy of the same bytes (bounds and grid built by
cg_rt_grid.hip), on cg_rt_random_scene(0x5EED, n), n = 1e4, 1e5, 1e6.
Per size: the wall time of each form (a host clock around the call, which ends in a stream
synchronise), the two forms alternating, medians over --repeats with min and max; the device
build's phases from HIP events (bounds, ranges, count, offsets, fill / order); candidates B,
entries E, cells and the builder's scratch; and whether the two grids are equal byte for byte.
For the largest size at 1920 x 1080: the rate of "move a tenth of the triangles on the device,
install the scene, render one frame", the device form against the same loop through the host form
(which downloads the triangles first).  Usage:
  python scripts/rt_scene_rate.py [--repeats 3] [--sizes 10000,100000,1000000]
                                  [--out profiles/rt_scene_rate.json]"""
import argparse
import ctypes as C
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
ap.add_argument("--sizes", default="10000,100000,1000000")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_scene_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

W, H, F = 1920, 1080, 1080.0
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
sizes = [int(s) for s in args.sizes.split(",") if s]
lib = cgamd.load()
ctx = cgamd.Context(0)
cam = cgamd.rt_camera(W, H, F)
lights = cgamd.default_lights()
d_out = torch.zeros(W * H, dtype=torch.int32, device=dev)
result = {"workload": "cg_rt_set_scene (host array) against cg_rt_set_scene_device (device copy), "
                      "cg_rt_random_scene(0x5EED, n)", "repeats": args.repeats, "sizes": {}}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def host_install(ptr, n):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = lib.cg_rt_set_scene(ctx.h, C.cast(ptr, C.POINTER(cgamd.Tri)), n, None, 0)
    dt = time.perf_counter() - t0
    if rc:
        raise SystemExit(f"cg_rt_set_scene failed: {rc}")
    return 1e3 * dt


def device_install(d, n):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ctx.rt_set_scene_device(d.data_ptr(), n)
    return 1e3 * (time.perf_counter() - t0)


def grid_bytes():
    g = ctx.rt_grid()
    return None if g is None else b"".join(g[k].tobytes() for k in ("res", "lo", "start", "tris")) + g["h"].tobytes()


try:
    # warm-up: code objects and host paths of both forms at a small size
    small = cgamd.random_scene(2000)
    ctx.rt_set_scene(small, 2000, None, 0)
    d_small = torch.frombuffer(bytearray(bytes(small)), dtype=torch.uint8).to(dev)
    ctx.rt_set_scene_device(d_small.data_ptr(), 2000)
    for n in sizes:
        tris = cgamd.random_scene(n)
        host = np.frombuffer(tris, np.float32).reshape(n, 19)
        d = torch.from_numpy(host).to(dev)
        device_install(d, n)                      # allocations of this size
        grid_dev = grid_bytes()
        info = ctx.rt_grid_info()
        phases = {k: [] for k in ("bounds", "ranges", "count", "offsets", "fill_order")}
        t_host, t_dev = [], []
        for r in range(args.repeats):
            t_host.append(host_install(host.ctypes.data, n))
            if r == 0:
                grid_host = grid_bytes()
            t_dev.append(device_install(d, n))
            for k, v in ctx.rt_grid_phase_ms().items():
                phases[k].append(v)
            print(f"n {n} repeat {r}: host {t_host[-1]:.1f} ms, device {t_dev[-1]:.2f} ms", flush=True)
        if grid_dev is None or grid_dev != grid_host:
            raise SystemExit(f"{n} triangles: the two forms' grids differ")
        hs, ds = spread(t_host), spread(t_dev)
        result["sizes"][str(n)] = {
            "host_install_ms": hs, "device_install_ms": ds,
            "host_over_device": hs["median"] / ds["median"],
            "device_faster_beyond_spreads": bool(hs["median"] - ds["median"] > hs["spread"] + ds["spread"]),
            "device_phase_ms": {k: spread(v) for k, v in phases.items()},
            "device_phase_ms_sum": sum(statistics.median(v) for v in phases.values()),
            "candidates_B": info["candidates"], "entries_E": info["entries"], "cells": info["cells"],
            "builder_scratch_bytes": info["bytes"], "grids_equal": True,
        }

    # a moving scene: a tenth of the triangles translated on the device, installed, one frame
    n = max(sizes)
    base = torch.from_numpy(np.frombuffer(cgamd.random_scene(n), np.float32).reshape(n, 19).copy()).to(dev)
    move = torch.zeros(n // 10, 3, 4, device=dev)
    move[:, :, :3] = 0.001
    staging = np.zeros((n, 19), np.float32)

    def step_device(k):
        sel = slice((k % 10) * (n // 10), (k % 10 + 1) * (n // 10))
        base[sel, 0:12] += move.reshape(n // 10, 12)
        ctx.rt_set_scene_device(base.data_ptr(), n)
        ctx.rt_render_device(cam, d_out.data_ptr(), lights=lights)
        torch.cuda.synchronize(dev)

    def step_host(k):
        sel = slice((k % 10) * (n // 10), (k % 10 + 1) * (n // 10))
        base[sel, 0:12] += move.reshape(n // 10, 12)
        staging[:] = base.cpu().numpy()
        rc = lib.cg_rt_set_scene(ctx.h, C.cast(staging.ctypes.data, C.POINTER(cgamd.Tri)), n, None, 0)
        if rc:
            raise SystemExit(f"cg_rt_set_scene failed: {rc}")
        ctx.rt_render_device(cam, d_out.data_ptr(), lights=lights)
        torch.cuda.synchronize(dev)

    def timed(fn, k, calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for j in range(calls):
            fn(k + j)
        return calls / (time.perf_counter() - t0)

    step_device(0)                                # warm-up: the frame's pools at this size
    step_device(1)
    r_dev, r_host = [], []
    for r in range(args.repeats):
        r_host.append(timed(step_host, 2 + 6 * r, 1))
        r_dev.append(timed(step_device, 3 + 6 * r, 5))
        print(f"moving scene repeat {r}: host form {r_host[-1]:.3f} /s, device form {r_dev[-1]:.2f} /s", flush=True)
    result["moving_scene"] = {
        "workload": f"{n} triangles, a tenth translated per step on the device, install, one {W}x{H} frame",
        "device_form_steps_per_s": spread(r_dev), "host_form_steps_per_s": spread(r_host),
        "device_over_host": statistics.median(r_dev) / statistics.median(r_host),
    }
finally:
    ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
