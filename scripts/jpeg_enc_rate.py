"""What the JPEG encoder costs and what compressed delivery gains, at 1920 x 1080 on one GPU.

(a) The encoder alone under HIP events: cg_image_encode_jpeg_device over 8 rendered frames a call, at
    Q = 75 and 90, 4:2:0 and 4:4:4, on a C2 raytracer frame and on a rasteriser frame, beside
    rt_tonemap_pack_kernel on the same frame count (the project's yardstick: 20 bytes a pixel).
    Microseconds per frame for the four kernels together, the median of --repeats rounds of 20
    calls, and the compressed bytes per frame.  The split between the four kernels comes from a
    kernel trace of `--kernels-only` (a short run of the same calls), summarised by the caller.
(b) cg_rt_render_sequence_jpeg against cg_rt_render_sequence and cg_rast_draw_sequence_jpeg against
    cg_rast_draw_sequence, 64 frames a call, into pageable and into pinned memory, in the same run:
    windows of about one second, the variants alternating, medians of --repeats windows after every
    shape has run once.
Usage: python scripts/jpeg_enc_rate.py [--repeats 5] [--kernels-only] [--out profiles/jpeg_enc_rate.json]"""
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
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--kernels-only", action="store_true", help="a few encoder calls and nothing else (for a kernel trace)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_enc_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cgamd  # noqa: E402

W, H = 1920, 1080
PX = W * H
NF = 8           # frames of an encoder call
SEQ = 64         # frames of a delivery call
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.Stream(dev)
f32 = lambda x: float(np.float32(x))   # noqa: E731
VARIANTS = [(75, cgamd.JPEG_420), (90, cgamd.JPEG_420), (75, cgamd.JPEG_444), (90, cgamd.JPEG_444)]
result = {"workload": f"JPEG encoder and compressed delivery at {W}x{H} on one GPU", "repeats": args.repeats,
          "window_s": args.window_s, "frames_per_encoder_call": NF, "frames_per_delivery_call": SEQ}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_us(call, frames, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(args.repeats + 1):
        e0.record(st)
        for _ in range(n):
            call()
        e1.record(st)
        torch.cuda.synchronize(dev)
        us.append(1e3 * e0.elapsed_time(e1) / (n * frames))
    return us[1:]                                # the first round loads the code object and allocates


def windows(legs, frames):
    rates = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for k, fn in legs.items():
            calls, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < args.window_s:   # the delivery calls return when the frames are there
                fn()
                calls += 1
            rates[k].append(calls * frames / (time.perf_counter() - t0))
    return {k: spread(v) for k, v in rates.items()}


slot = PX
d_out = torch.zeros(NF * slot, dtype=torch.uint8, device=dev)
d_bytes = torch.zeros(NF, dtype=torch.int64, device=dev)

with cgamd.Context(0) as ctx:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    ctx.rast_set_scene()
    rt_frames = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, 1080.0)] * NF, rt_frames.data_ptr(), stream=st.cuda_stream)
    rast_ps = [cgamd.rast_params(W, H, 768.0, (0.0, 0.0, f32(-3.001 + 0.01 * k), 1.0)) for k in range(SEQ)]
    rast_frames = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
    d_info = torch.zeros(3 * (NF + 1), dtype=torch.int64, device=dev)
    ctx.rast_draw_sequence_device(rast_ps[:NF], rast_frames.data_ptr(), d_info=d_info.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize(dev)

    def encode(frames, q, sub):
        return lambda: ctx.image_encode_jpeg_device(frames.data_ptr(), W, H, NF, d_out.data_ptr(), slot, d_bytes.data_ptr(),
                                                    q, sub, stream=st.cuda_stream)

    if args.kernels_only:
        for frames in (rt_frames, rast_frames):
            for q, sub in VARIANTS:
                for _ in range(5):
                    encode(frames, q, sub)()
        torch.cuda.synchronize(dev)
        raise SystemExit(0)

    # (a) the encoder alone
    rgba = torch.zeros(NF * PX * 4, dtype=torch.float32, device=dev)
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, 1080.0)] * NF, rgba.data_ptr(), pix_format=cgamd.PIX_RGBA_F32,
                                stream=st.cuda_stream)
    d_scales = torch.ones(NF, dtype=torch.float32, device=dev)
    d_argb = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    result["rt_tonemap_pack_kernel_us_per_frame"] = spread(event_us(
        lambda: ctx.rt_tonemap_pack_device(rgba.data_ptr(), PX, NF, d_scales.data_ptr(), d_argb.data_ptr(),
                                           cgamd.TONE_REINHARD, stream=st.cuda_stream), NF))
    del rgba, d_argb
    result["encoder"] = {}
    for name, frames in (("rt_c2", rt_frames), ("rast", rast_frames)):
        for q, sub in VARIANTS:
            us = spread(event_us(encode(frames, q, sub), NF))
            lens = d_bytes.cpu().numpy()
            key = f"{name}_q{q}_{'420' if sub else '444'}"
            result["encoder"][key] = {"us_per_frame": us, "bytes_per_frame": float(lens.mean()),
                                      "overflowed_slots": int((lens < 0).sum())}
            print(key, json.dumps(result["encoder"][key]), flush=True)

    # (b) compressed against raw delivery
    states = [cgamd.rt_camera(W, H, 1080.0, (0.0, 0.0, f32(-3.0 + 0.005 * k), 1.0)) for k in range(SEQ)]
    lights = [cgamd.default_lights()] * SEQ
    raw_page = np.zeros(SEQ * PX, np.uint32)
    raw_pin = torch.zeros(SEQ * PX, dtype=torch.int32).pin_memory()
    jpg_page = np.zeros(SEQ * PX // 2, np.uint8)
    jpg_pin = torch.zeros(SEQ * PX // 2, dtype=torch.uint8).pin_memory()
    q, sub = 75, cgamd.JPEG_420
    rt_legs = {
        "raw_pageable": lambda: ctx.rt_render_sequence(states, lights, out=raw_page),
        "jpeg_pageable": lambda: ctx.rt_render_sequence_jpeg(states, lights, q, sub, out=jpg_page, full=True),
        "raw_pinned": lambda: ctx.rt_render_sequence(states, lights, out=raw_pin),
        "jpeg_pinned": lambda: ctx.rt_render_sequence_jpeg(states, lights, q, sub, out=jpg_pin, full=True),
    }
    fps = windows(rt_legs, SEQ)
    rc, files, offsets, _ = rt_legs["jpeg_pinned"]()
    result["rt_sequence"] = {"frames_per_s": fps, "status": rc, "bytes_per_frame": int(offsets[SEQ]) / SEQ,
                             "jpeg_over_raw_pageable": fps["jpeg_pageable"]["median"] / fps["raw_pageable"]["median"],
                             "jpeg_over_raw_pinned": fps["jpeg_pinned"]["median"] / fps["raw_pinned"]["median"]}
    print("rt_sequence", json.dumps(result["rt_sequence"]), flush=True)
    rast_legs = {
        "raw_pageable": lambda: ctx.rast_draw_sequence(rast_ps, out=raw_page),
        "jpeg_pageable": lambda: ctx.rast_draw_sequence_jpeg(rast_ps, q, sub, out=jpg_page, full=True),
        "raw_pinned": lambda: ctx.rast_draw_sequence(rast_ps, out=raw_pin),
        "jpeg_pinned": lambda: ctx.rast_draw_sequence_jpeg(rast_ps, q, sub, out=jpg_pin, full=True),
    }
    fps = windows(rast_legs, SEQ)
    rc, files, offsets, _, _ = rast_legs["jpeg_pinned"]()
    result["rast_sequence"] = {"frames_per_s": fps, "status": rc, "bytes_per_frame": int(offsets[SEQ]) / SEQ,
                               "jpeg_over_raw_pageable": fps["jpeg_pageable"]["median"] / fps["raw_pageable"]["median"],
                               "jpeg_over_raw_pinned": fps["jpeg_pinned"]["median"] / fps["raw_pinned"]["median"]}
    print("rast_sequence", json.dumps(result["rast_sequence"]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
