"""What the rasteriser's buffers cost beside a plain frame: cg_rast_draw_device alone against
cg_rast_draw_buffers_device with all nine planes, then with only `clip`, at 1920 x 1080, focal 768,
colour mode 0, on the reference scene (dense route) and on cg_rast_random_scene(0x5EED, 1e6, 0.02)
as the room (compact route); and the wall time of one cg_rast_pick (median of 20).
Per scene: windows of --calls enqueued calls closed by a stream synchronise, the three calls taking
turns, the median of --repeats windows each, with min and max (scripts/rt_hits_rate.py's method).
The difference of a buffers call and the plain frame is the buffers kernel (a buffers call runs the
same frame, then that one kernel).  The expectation to confirm or refute: the kernel is bound by
its stores -- three 24.9 MB float planes, 33.2 MB of pos, 16.6 MB of ids, about 125 MB at 1080p --
plus one state word and one record read per pixel.  Usage:
  python scripts/rast_buffers_rate.py [--repeats 3] [--tris 1000000] [--out profiles/rast_buffers_rate.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "computer-graphics_amd"))
import cgamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rast_buffers_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

W, H, F = 1920, 1080, 768.0
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ctx = cgamd.Context(0)
p = cgamd.rast_params(W, H, F)
npx = W * H
d = {n: torch.zeros(npx * k, dtype=torch.float32 if dt.__name__ == "float32" else torch.int32, device=dev)
     for n, dt, k in cgamd.RAST_PLANES}
ptr = {n: t.data_ptr() for n, t in d.items()}
store_bytes = sum(t.numel() * 4 for n, t in d.items() if n not in ("argb", "depth", "shadow"))
result = {"workload": f"cg_rast_draw_device against cg_rast_draw_buffers_device, {W}x{H}, focal {F}, colour mode 0",
          "repeats": args.repeats, "buffers_kernel_store_bytes": store_bytes, "scenes": {}}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def plain():
    ctx.rast_draw_device(p, ptr["argb"], ptr["depth"], ptr["shadow"])


def buffers_all():
    ctx.rast_draw_buffers_device(p, **ptr)


def buffers_clip():
    ctx.rast_draw_buffers_device(p, argb=ptr["argb"], depth=ptr["depth"], shadow=ptr["shadow"], clip=ptr["clip"])


CALLS = (("frame", plain), ("buffers_all", buffers_all), ("buffers_clip", buffers_clip))


def window(fn, calls):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize(dev)
    return calls / (time.perf_counter() - t0)


def measure(name, calls):
    for _ in range(2):                                   # code objects and scratch of every call
        for _, fn in CALLS:
            fn()
    torch.cuda.synchronize(dev)
    rates = {k: [] for k, _ in CALLS}
    for r in range(args.repeats):
        for k, fn in CALLS:
            rates[k].append(window(fn, calls))
        print(f"{name} repeat {r}: " + ", ".join(f"{k} {v[-1]:.1f} /s" for k, v in rates.items()), flush=True)
    ms = {k: 1e3 / statistics.median(v) for k, v in rates.items()}
    info = ctx.rast_scratch_info()
    rec = {"calls_per_window": calls, "per_s": {k: spread(v) for k, v in rates.items()}, "ms": ms,
           "buffers_kernel_ms": ms["buffers_all"] - ms["frame"], "clip_only_kernel_ms": ms["buffers_clip"] - ms["frame"],
           "route": int(info["route"]), "clipped": int(info["tris"]), "records": int(info["recs"]),
           "owned_pixels": int((d["clip"] >= 0).sum().item())}
    extra = rec["buffers_kernel_ms"]
    rec["store_GB_per_s"] = store_bytes / (extra * 1e-3) / 1e9 if extra > 0 else None
    t = []
    for k in range(20):
        x, y = (W // 2 + 37 * k) % W, (H // 2 + 11 * k) % H
        t0 = time.perf_counter()
        ctx.rast_pick(p, x, y)
        t.append(1e3 * (time.perf_counter() - t0))
    rec["pick_ms"] = spread(t[1:])
    result["scenes"][name] = rec


try:
    ctx.rast_set_scene(*cgamd.rast_scene())
    measure("reference_scene", 100)
    room = cgamd.rast_random_scene(args.tris, 0.02, 0x5EED)
    ctx.rast_set_scene(room, args.tris, (cgamd.RTri * 1)(), 0)
    measure(f"random_{args.tris}_triangles", 10)
finally:
    ctx.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
