"""What the PNG encoder costs and whether exact delivery beats raw delivery, at 1920 x 1080 on one GPU.

(a) The encoder alone under HIP events: cg_image_encode_png_device over 8 rendered frames a call
    (RGB adaptive, RGB filter 0, RGBA adaptive) on a C2 raytracer frame, beside
    rt_tonemap_pack_kernel and the JPEG encoder (Q = 75, 4:2:0) on the same frames in the same run.
    Microseconds per frame, the median of --repeats rounds of 10 calls.
(b) The split between the four kernels from cg_kernel_time over a few calls of each variant.
(c) File sizes: the C2 frame, a yawed frame and the rasteriser's reference scene in colour modes 0
    and 1, RGB adaptive.
(d) cg_rt_render_sequence_png against cg_rt_render_sequence and cg_rt_render_sequence_jpeg, and the
    rasteriser's three, 64 frames a call, into pageable and into pinned memory, in the same run:
    windows of about one second, the variants alternating, medians of --repeats windows after every
    shape has run once.
Usage: python scripts/png_enc_rate.py [--repeats 5] [--out profiles/png_enc_rate.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_enc_rate.json"))
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
A = cgamd.PNG_FILTER_ADAPTIVE
VARIANTS = [("rgb_adaptive", cgamd.PNG_RGB, A), ("rgb_filter0", cgamd.PNG_RGB, 0), ("rgba_adaptive", cgamd.PNG_RGBA, A)]
KERNELS = ("png_enc_filter_kernel", "png_enc_band_kernel", "png_enc_scan_kernel", "png_enc_gather_kernel")
result = {"workload": f"PNG encoder and exact delivery at {W}x{H} on one GPU", "repeats": args.repeats,
          "window_s": args.window_s, "frames_per_encoder_call": NF, "frames_per_delivery_call": SEQ}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_us(call, frames, n=10):
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


slot = cgamd.image_png_bound(W, H, cgamd.PNG_RGBA)
d_out = torch.zeros(NF * slot, dtype=torch.uint8, device=dev)
d_bytes = torch.zeros(NF, dtype=torch.int64, device=dev)

with cgamd.Context(0) as ctx:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    ctx.rast_set_scene()
    rt_frames = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, 1080.0)] * NF, rt_frames.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize(dev)

    def encode(frames, colour, filt, nf=NF):
        return lambda: ctx.image_encode_png_device(frames.data_ptr(), W, H, nf, d_out.data_ptr(), slot, d_bytes.data_ptr(),
                                                   colour, filt, stream=st.cuda_stream)

    # (a) the encoder alone, beside the pack kernel and the JPEG encoder
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
    result["jpeg_q75_420_us_per_frame"] = spread(event_us(
        lambda: ctx.image_encode_jpeg_device(rt_frames.data_ptr(), W, H, NF, d_out.data_ptr(), PX, d_bytes.data_ptr(), 75,
                                             cgamd.JPEG_420, stream=st.cuda_stream), NF))
    result["encoder"] = {}
    for name, colour, filt in VARIANTS:
        us = spread(event_us(encode(rt_frames, colour, filt), NF))
        lens = d_bytes.cpu().numpy()
        # (b) the split, from the library's own per-kernel timing over five more calls
        cgamd.kernel_timing(True)
        for _ in range(5):
            encode(rt_frames, colour, filt)()
        torch.cuda.synchronize(dev)
        split = {k: 1e3 * cgamd.kernel_time(k)[0] / (5 * NF) for k in KERNELS}
        cgamd.kernel_timing(False)
        result["encoder"][name] = {"us_per_frame": us, "bytes_per_frame": float(lens.mean()),
                                   "kernel_us_per_frame": split}
        print(name, json.dumps(result["encoder"][name]), flush=True)

    # (c) file sizes, RGB adaptive, one frame a call
    def size_of(frame_tensor):
        encode(frame_tensor, cgamd.PNG_RGB, A, 1)()
        torch.cuda.synchronize(dev)
        return int(d_bytes.cpu().numpy()[0])

    one = torch.zeros(PX, dtype=torch.int32, device=dev)
    sizes = {"rt_c2": size_of(rt_frames)}
    import ctypes as C
    import math
    c, s_ = f32(math.cos(0.3)), f32(math.sin(0.3))
    yaw = cgamd.rt_camera(W, H, 1080.0, R=(C.c_float * 16)(c, 0, s_, 0, 0, 1, 0, 0, -s_, 0, c, 0, 0, 0, 0, 1))
    ctx.rt_render_frames_device([yaw], one.data_ptr(), stream=st.cuda_stream)
    sizes["rt_yawed"] = size_of(one)
    d_info = torch.zeros(3 * 2, dtype=torch.int64, device=dev)
    for mode in (0, 1):
        p = cgamd.rast_params(W, H, 768.0)
        p.colour_mode = mode
        ctx.rast_draw_sequence_device([p], one.data_ptr(), d_info=d_info.data_ptr(), stream=st.cuda_stream)
        sizes[f"rast_mode{mode}"] = size_of(one)
    result["bytes"] = sizes
    result["raw_bytes_per_frame"] = PX * 4
    print("bytes", json.dumps(sizes), flush=True)

    # (d) exact against raw and JPEG delivery
    states = [cgamd.rt_camera(W, H, 1080.0, (0.0, 0.0, f32(-3.0 + 0.005 * k), 1.0)) for k in range(SEQ)]
    lights = [cgamd.default_lights()] * SEQ
    rast_ps = [cgamd.rast_params(W, H, 768.0, (0.0, 0.0, f32(-3.001 + 0.01 * k), 1.0)) for k in range(SEQ)]
    raw_page = np.zeros(SEQ * PX, np.uint32)
    raw_pin = torch.zeros(SEQ * PX, dtype=torch.int32).pin_memory()
    file_page = np.zeros(SEQ * PX, np.uint8)
    file_pin = torch.zeros(SEQ * PX, dtype=torch.uint8).pin_memory()
    rt_legs = {
        "raw_pageable": lambda: ctx.rt_render_sequence(states, lights, out=raw_page),
        "jpeg_pageable": lambda: ctx.rt_render_sequence_jpeg(states, lights, 75, cgamd.JPEG_420, out=file_page, full=True),
        "png_pageable": lambda: ctx.rt_render_sequence_png(states, lights, out=file_page, full=True),
        "raw_pinned": lambda: ctx.rt_render_sequence(states, lights, out=raw_pin),
        "jpeg_pinned": lambda: ctx.rt_render_sequence_jpeg(states, lights, 75, cgamd.JPEG_420, out=file_pin, full=True),
        "png_pinned": lambda: ctx.rt_render_sequence_png(states, lights, out=file_pin, full=True),
    }
    fps = windows(rt_legs, SEQ)
    rc, files, offsets, _ = rt_legs["png_pinned"]()
    result["rt_sequence"] = {"frames_per_s": fps, "status": rc, "bytes_per_frame": int(offsets[SEQ]) / SEQ,
                             "png_over_raw_pageable": fps["png_pageable"]["median"] / fps["raw_pageable"]["median"],
                             "png_over_raw_pinned": fps["png_pinned"]["median"] / fps["raw_pinned"]["median"]}
    print("rt_sequence", json.dumps(result["rt_sequence"]), flush=True)
    rast_legs = {
        "raw_pageable": lambda: ctx.rast_draw_sequence(rast_ps, out=raw_page),
        "jpeg_pageable": lambda: ctx.rast_draw_sequence_jpeg(rast_ps, 75, cgamd.JPEG_420, out=file_page, full=True),
        "png_pageable": lambda: ctx.rast_draw_sequence_png(rast_ps, out=file_page, full=True),
        "raw_pinned": lambda: ctx.rast_draw_sequence(rast_ps, out=raw_pin),
        "jpeg_pinned": lambda: ctx.rast_draw_sequence_jpeg(rast_ps, 75, cgamd.JPEG_420, out=file_pin, full=True),
        "png_pinned": lambda: ctx.rast_draw_sequence_png(rast_ps, out=file_pin, full=True),
    }
    fps = windows(rast_legs, SEQ)
    rc, files, offsets, _, _ = rast_legs["png_pinned"]()
    result["rast_sequence"] = {"frames_per_s": fps, "status": rc, "bytes_per_frame": int(offsets[SEQ]) / SEQ,
                               "png_over_raw_pageable": fps["png_pageable"]["median"] / fps["raw_pageable"]["median"],
                               "png_over_raw_pinned": fps["png_pinned"]["median"] / fps["raw_pinned"]["median"]}
    print("rast_sequence", json.dumps(result["rast_sequence"]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
