"""What the rasteriser's float picture and exposure chain cost, at 1920 x 1080 on one GPU.

Scenes: the reference scene (dense route) and cg_rast_random_scene(0x5EED, N, 0.02) as the room
(N = --tris, compact route).  Each call draws --frames colour-mode-0 frames, the camera stepping
0.01 in z.  Legs, timed over windows of about --window-s seconds of enqueued calls closed by a
device synchronise, the legs alternating, medians of --repeats windows:
  sequence_argb     cg_rast_draw_sequence_device (8.3 MB a frame stored by the post-pass)
  sequence_picture  cg_rast_draw_sequence_picture_device (33.2 MB a frame)
  exposed           cg_rast_draw_exposed_device (Reinhard, rate 0.5): the float sequence in chunks
                    of 8, histogram, exposure, pack; the microseconds a frame it adds to the plain
                    sequence are reported
and, on one rendered chunk of 8 float frames, HIP events around 50 calls of
cg_rast_tonemap_pack_device beside cg_rt_tonemap_pack_device on the same planes (16 bytes in, 4 out
a pixel), medians of --repeats rounds.  Nothing here is a threshold.
Usage: python scripts/rast_hdr_rate.py [--repeats 5] [--frames 16] [--tris 1000000] [--out profiles/rast_hdr_rate.json]"""
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
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rast_hdr_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

W, H, F, N = 1920, 1080, 768.0, args.frames
PX = W * H
f32 = lambda x: float(np.float32(x))   # noqa: E731
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.Stream(dev)   # a stream of the script's own: a null stream argument would mean the context's
ps = [cgamd.rast_params(W, H, F, (0.0, 0.0, f32(-3.001 + 0.01 * k), 1.0)) for k in range(N)]
expo = cgamd.hdr_params(rate=0.5)
d_argb = torch.zeros(N * PX, dtype=torch.int32, device=dev)
d_rgba = torch.zeros(N * PX * 4, dtype=torch.float32, device=dev)
d_scales = torch.zeros(N, dtype=torch.float32, device=dev)
d_info = torch.zeros(3 * (N + 1), dtype=torch.int64, device=dev)


def windows(legs):
    """frames/s of each leg: calls for about window_s seconds, closed by a synchronise."""
    rates = {k: [] for k in legs}
    for fn in legs.values():   # every shape once: allocations, lanes, code objects
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for k, fn in legs.items():
            calls, t0 = 0, time.perf_counter()
            while True:
                fn()
                calls += 1
                if calls % 4 == 0:
                    torch.cuda.synchronize(dev)   # bound the queue: a window is host time over finished work
                    if time.perf_counter() - t0 >= args.window_s:
                        break
            torch.cuda.synchronize(dev)
            rates[k].append(calls * N / (time.perf_counter() - t0))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rates.items()}


def scene_legs(ctx):
    return {
        "sequence_argb": lambda: ctx.rast_draw_sequence_device(ps, d_argb.data_ptr(), d_info=d_info.data_ptr(),
                                                               stream=st.cuda_stream),
        "sequence_picture": lambda: ctx.rast_draw_sequence_picture_device(ps, d_rgba.data_ptr(), d_info=d_info.data_ptr(),
                                                                          stream=st.cuda_stream),
        "exposed": lambda: ctx.rast_draw_exposed_device(ps, d_argb.data_ptr(), d_scales.data_ptr(), expo,
                                                        d_info.data_ptr(), op=cgamd.TONE_REINHARD, stream=st.cuda_stream),
    }


def summarise(fps):
    a, p, e = (fps[k]["median"] for k in ("sequence_argb", "sequence_picture", "exposed"))
    return {"frames_per_s": fps, "picture_over_argb": p / a, "exposed_over_argb": e / a,
            "picture_added_us_per_frame": 1e6 * (1 / p - 1 / a), "exposed_added_us_per_frame": 1e6 * (1 / e - 1 / a)}


out = {"size": [W, H], "frames_per_call": N, "repeats": args.repeats, "window_s": args.window_s,
       "bytes_per_frame": {"argb_store": PX * 4, "picture_store": PX * 16}, "scenes": {}}
with cgamd.Context(0) as ctx:
    ctx.rast_set_scene()
    out["scenes"]["reference"] = summarise(windows(scene_legs(ctx)))
    out["scenes"]["reference"]["route"] = ctx.rast_scratch_info()["route"]
    print("reference", json.dumps(out["scenes"]["reference"]), flush=True)

    # the pack kernels on a chunk of 8 rendered float frames
    nf = min(8, N)
    ctx.rast_draw_sequence_picture_device(ps[:nf], d_rgba.data_ptr(), d_info=d_info.data_ptr(), stream=st.cuda_stream)
    d_scales.fill_(1.7)
    torch.cuda.synchronize(dev)
    packs = {
        "rast_tonemap_pack_kernel": lambda: ctx.rast_tonemap_pack_device(d_rgba.data_ptr(), PX, nf, d_scales.data_ptr(),
                                                                         d_argb.data_ptr(), cgamd.TONE_REINHARD,
                                                                         stream=st.cuda_stream),
        "rt_tonemap_pack_kernel": lambda: ctx.rt_tonemap_pack_device(d_rgba.data_ptr(), PX, nf, d_scales.data_ptr(),
                                                                     d_argb.data_ptr(), cgamd.TONE_REINHARD,
                                                                     stream=st.cuda_stream),
    }
    us = {k: [] for k in packs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.repeats + 1):      # the first round warms up
        for k, fn in packs.items():
            e0.record(st)
            for _ in range(50):
                fn()
            e1.record(st)
            torch.cuda.synchronize(dev)
            us[k].append(1e3 * e0.elapsed_time(e1) / (50 * nf))
    out["pack"] = {k: {"us_per_frame": statistics.median(v[1:]), "bytes_per_s": PX * 20 / (1e-6 * statistics.median(v[1:]))}
                   for k, v in us.items()}
    out["pack"]["frames_per_call"] = nf
    print("pack", json.dumps(out["pack"]), flush=True)

if args.tris > 0:
    with cgamd.Context(0) as ctx:
        room = cgamd.rast_random_scene(args.tris, 0.02, 0x5EED)
        ctx.rast_set_scene(room, args.tris, (cgamd.RTri * 1)(), 0)
        key = f"random_{args.tris}"
        out["scenes"][key] = summarise(windows(scene_legs(ctx)))
        out["scenes"][key]["route"] = ctx.rast_scratch_info()["route"]
        print(key, json.dumps(out["scenes"][key]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
