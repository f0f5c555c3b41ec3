"""What bloom costs on top of the exposed chain, at 1920 x 1080 on one GPU.

1. The kernels alone under HIP events, on the 8 rendered CG_PIX_RGBA_F32 frames of one chunk:
   cg_hdr_bloom_device with 1 level (bright pass with the first box, one blur) and with 4 levels (all
   eight launches), cg_hdr_bloom_pack_device, and rt_tonemap_pack_kernel on the same planes in the
   same run -- the yardstick: it streams 20 bytes a pixel.  Microseconds per frame, the median of
   --repeats rounds of 50 calls.
2. cg_rt_render_exposed_bloom_device against cg_rt_render_exposed_device, 16 frames a call, on C2, on
   C2 after one yaw key and on cg_rt_random_scene(0x5EED, N); cg_rast_draw_exposed_bloom_device against
   cg_rast_draw_exposed_device on the reference scene and on cg_rast_random_scene(0x5EED, N, 0.02) as
   the room.  Windows of about one second of enqueued calls closed by a device synchronise, the two
   variants alternating, medians of --repeats windows after every shape has run once.
Traffic model, levels 4: the bright pass reads 16 bytes a frame pixel and writes 16 a level-1 pixel
(33.2 + 8.3 MB), the further boxes and every level's blur read and write their level once (level 1:
8.3 MB each way, the coarser levels a third of that again, the up-add's taps another read of the
coarser level), the composite reads U_1 (8.3 MB) beside what the pack reads anyway.
Usage: python scripts/bloom_rate.py [--repeats 5] [--tris 1000000] [--out profiles/bloom_rate.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "computer-graphics_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cgamd  # noqa: E402

W, H, F = 1920, 1080, 1080.0
PX = W * H
NF = 16
LEVELS = 4
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.Stream(dev)   # a stream of the script's own: a null stream argument would mean the context's
f32 = lambda x: float(np.float32(x))   # noqa: E731
bloom = cgamd.hdr_bloom_params(LEVELS, 1.0, 64.0, 0.25)
expo = cgamd.hdr_params(permille=990, target=1.0, rate=0.5)
ws, hs, _, TOTAL = cgamd.hdr_bloom_layout(W, H, LEVELS)
level_px = [w * h for w, h in zip(ws, hs)]
# bytes a frame.  MODEL: bright pass with the first box, every level's blur (read B_k, write U_k), the composite's
# taps.  MODEL_ALL adds what that leaves out: the boxes of levels 2.. and the up-add's taps of level k + 1.
MODEL = 16 * (PX + level_px[0]) + 16 * 2 * sum(level_px) + 16 * level_px[0]
MODEL_ALL = MODEL + 16 * sum(level_px[k - 1] + level_px[k] for k in range(1, LEVELS)) + 16 * sum(level_px[1:])
result = {"workload": f"bloom on the exposed chain at {W}x{H} on one GPU, levels {LEVELS}", "repeats": args.repeats,
          "window_s": args.window_s, "frames_per_call": NF, "pyramid_pixels": TOTAL, "model_bytes_per_frame": MODEL,
          "model_bytes_per_frame_with_boxes_and_taps": MODEL_ALL,
          "several_levels_per_workgroup_box": "not built: one launch per level"}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_us(call, frames, n=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(args.repeats + 1):
        e0.record(st)
        for _ in range(n):
            call()
        e1.record(st)
        torch.cuda.synchronize(dev)
        us.append(1e3 * e0.elapsed_time(e1) / (n * frames))
    return us[1:]                                # the first round loads the code object


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
            rates[k].append(calls * NF / (time.perf_counter() - t0))
    return {k: spread(v) for k, v in rates.items()}


def summarise(fps, pack_bytes_per_s):
    e, b = fps["exposed"]["median"], fps["exposed_bloom"]["median"]
    added_us = 1e6 * (1 / b - 1 / e)
    model_us = 1e6 * MODEL / pack_bytes_per_s
    return {"frames_per_s": fps, "bloom_over_exposed": b / e, "added_us_per_frame": added_us,
            "added_bytes_over_added_time_gb_per_s": MODEL / (added_us * 1e-6) / 1e9 if added_us > 0 else None,
            "model_us_per_frame_at_the_pack_rate": model_us, "added_over_model": added_us / model_us}


d_argb = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
d_scales = torch.zeros(NF, dtype=torch.float32, device=dev)
d_info = torch.zeros(3 * (NF + 1), dtype=torch.int64, device=dev)

with cgamd.Context(0) as ctx:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    # 1. the kernels alone, on the 8 frames of a chunk
    nf = 8
    rendered = torch.zeros(nf * PX * 4, dtype=torch.float32, device=dev)
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, F)] * nf, rendered.data_ptr(), pix_format=cgamd.PIX_RGBA_F32,
                                stream=st.cuda_stream)
    d_pyr = torch.zeros(nf * TOTAL * 4, dtype=torch.float32, device=dev)
    d_scales.fill_(1.7)
    torch.cuda.synchronize(dev)
    one = cgamd.hdr_bloom_params(1, 1.0, 64.0, 0.25)
    kernels = {
        "rt_tonemap_pack_kernel": lambda: ctx.rt_tonemap_pack_device(rendered.data_ptr(), PX, nf, d_scales.data_ptr(),
                                                                     d_argb.data_ptr(), cgamd.TONE_REINHARD, stream=st.cuda_stream),
        "bloom_pyramid_levels_1": lambda: ctx.hdr_bloom_device(rendered.data_ptr(), W, H, nf, d_scales.data_ptr(), one,
                                                               d_pyr.data_ptr(), stream=st.cuda_stream),
        f"bloom_pyramid_levels_{LEVELS}": lambda: ctx.hdr_bloom_device(rendered.data_ptr(), W, H, nf, d_scales.data_ptr(), bloom,
                                                                       d_pyr.data_ptr(), stream=st.cuda_stream),
        "bloom_pack_kernel": lambda: ctx.hdr_bloom_pack_device(rendered.data_ptr(), d_pyr.data_ptr(), W, H, nf,
                                                               d_scales.data_ptr(), bloom, d_argb.data_ptr(), cgamd.BLOOM_RULE_RT,
                                                               cgamd.TONE_REINHARD, stream=st.cuda_stream),
    }
    us = {k: spread(event_us(fn, nf)) for k, fn in kernels.items()}
    pack_rate = PX * 20 / (us["rt_tonemap_pack_kernel"]["median"] * 1e-6)
    result["kernels_us_per_frame"] = us
    result["pack_bytes_per_s"] = pack_rate
    result["kernels_gb_per_s"] = {
        "bloom_pyramid_levels_1": 16 * (PX + 3 * level_px[0]) / (us["bloom_pyramid_levels_1"]["median"] * 1e-6) / 1e9,
        f"bloom_pyramid_levels_{LEVELS}": (MODEL_ALL - 16 * level_px[0]) / (us[f"bloom_pyramid_levels_{LEVELS}"]["median"] * 1e-6) / 1e9,
        "bloom_pack_kernel": (PX * 20 + 16 * level_px[0]) / (us["bloom_pack_kernel"]["median"] * 1e-6) / 1e9,
    }
    print("kernels", json.dumps(us), flush=True)
    del rendered, d_pyr

    # 2. the exposed calls with and without bloom
    def rt_legs(cam):
        cams = [cam] * NF
        return {"exposed": lambda: ctx.rt_render_exposed_device(cams, d_argb.data_ptr(), d_scales.data_ptr(), expo,
                                                                op=cgamd.TONE_REINHARD, stream=st.cuda_stream),
                "exposed_bloom": lambda: ctx.rt_render_exposed_bloom_device(cams, d_argb.data_ptr(), d_scales.data_ptr(), expo,
                                                                            bloom, op=cgamd.TONE_REINHARD, stream=st.cuda_stream)}
    result["rt"] = {}
    yaw = float(np.float32(0.0) - np.float32(0.174533))
    for name, cam in (("c2", cgamd.rt_camera(W, H, F)), ("c2_yaw", cgamd.rt_camera(W, H, F, R=cgamd.yaw_matrix(yaw)))):
        result["rt"][name] = summarise(windows(rt_legs(cam)), pack_rate)
        print(name, json.dumps(result["rt"][name]), flush=True)
    if args.tris > 0:
        big = torch.from_numpy(np.frombuffer(cgamd.random_scene(args.tris), np.float32).reshape(args.tris, 19).copy()).to(dev)
        ctx.rt_set_scene_device(big.data_ptr(), args.tris)
        key = f"random_{args.tris}"
        result["rt"][key] = summarise(windows(rt_legs(cgamd.rt_camera(W, H, F))), pack_rate)
        print(key, json.dumps(result["rt"][key]), flush=True)

ps = [cgamd.rast_params(W, H, 768.0, (0.0, 0.0, f32(-3.001 + 0.01 * k), 1.0)) for k in range(NF)]


def rast_legs(ctx):
    return {"exposed": lambda: ctx.rast_draw_exposed_device(ps, d_argb.data_ptr(), d_scales.data_ptr(), expo, d_info.data_ptr(),
                                                            op=cgamd.TONE_REINHARD, stream=st.cuda_stream),
            "exposed_bloom": lambda: ctx.rast_draw_exposed_bloom_device(ps, d_argb.data_ptr(), d_scales.data_ptr(), expo, bloom,
                                                                        d_info.data_ptr(), op=cgamd.TONE_REINHARD,
                                                                        stream=st.cuda_stream)}


result["rast"] = {}
with cgamd.Context(0) as ctx:
    ctx.rast_set_scene()
    result["rast"]["reference"] = summarise(windows(rast_legs(ctx)), pack_rate)
    print("rast reference", json.dumps(result["rast"]["reference"]), flush=True)
if args.tris > 0:
    with cgamd.Context(0) as ctx:
        room = cgamd.rast_random_scene(args.tris, 0.02, 0x5EED)
        ctx.rast_set_scene(room, args.tris, (cgamd.RTri * 1)(), 0)
        key = f"random_{args.tris}"
        result["rast"][key] = summarise(windows(rast_legs(ctx)), pack_rate)
        print("rast", key, json.dumps(result["rast"][key]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
