"""What the EXR encoder costs and whether float pictures delivered as files beat copying the floats,
at 1920 x 1080 on one GPU.

(a) The encoder alone under HIP events: cg_image_encode_exr_device over 8 rendered pictures a call
    (RGBA; half and float, ZIP and NONE) on a C2 raytracer frame, beside rt_tonemap_pack_kernel and
    the PNG encoder (RGB, adaptive) on the same frame in the same run.  Microseconds per frame, the
    median of --repeats rounds of 5 calls.
(b) The split between the four kernels from cg_kernel_time over a few calls of each variant.
(c) File sizes (RGBA half ZIP): the C2 frame, a yawed frame and the rasteriser's reference scene in
    colour modes 0 and 1, with the share of chunks that fell back to raw bytes (counted by the
    tests' independent reader, which also checks each file).
(d) cg_rt_render_sequence_exr (half ZIP, and half NONE: half the floats' bytes behind a trivial
    encoder) against the raw float baseline -- chunks of 8 float
    pictures from cg_rt_render_sequence_device copied whole to the host, the copy of one chunk
    overlapping the render of the next on two buffers -- and against cg_rt_render_sequence (8-bit
    raw); the rasteriser's three likewise.  32 frames a call, into pageable and into pinned memory,
    in the same run: windows of about one second, the variants alternating, medians of --repeats
    windows after every shape has run once.
Usage: python scripts/exr_enc_rate.py [--repeats 5] [--out profiles/exr_enc_rate.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "computer-graphics_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exr_enc_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cgamd  # noqa: E402
import exr_enc_ref  # noqa: E402

W, H = 1920, 1080
PX = W * H
NF = 8           # frames of an encoder call, and of a chunk of the float baseline
SEQ = 32         # frames of a delivery call
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.Stream(dev)
cp = torch.cuda.Stream(dev)
f32 = lambda x: float(np.float32(x))   # noqa: E731
VARIANTS = [("half_zip", cgamd.EXR_HALF, cgamd.EXR_ZIP), ("float_zip", cgamd.EXR_FLOAT, cgamd.EXR_ZIP),
            ("half_none", cgamd.EXR_HALF, cgamd.EXR_NONE), ("float_none", cgamd.EXR_FLOAT, cgamd.EXR_NONE)]
KERNELS = ("exr_enc_plane_kernel", "exr_enc_chunk_kernel", "exr_enc_scan_kernel", "exr_enc_gather_kernel")
RT_ALPHA = 1.0 / 9.0
result = {"workload": f"EXR encoder and float-picture delivery at {W}x{H} on one GPU", "repeats": args.repeats,
          "window_s": args.window_s, "frames_per_encoder_call": NF, "frames_per_delivery_call": SEQ}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_us(call, frames, n=5):
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
            while time.perf_counter() - t0 < args.window_s:   # every leg returns when the frames are in host memory
                fn()
                calls += 1
            rates[k].append(calls * frames / (time.perf_counter() - t0))
    return {k: spread(v) for k, v in rates.items()}


slot = cgamd.image_exr_bound(W, H, cgamd.EXR_RGBA, cgamd.EXR_FLOAT)
d_out = torch.zeros(NF * slot, dtype=torch.uint8, device=dev)
d_bytes = torch.zeros(NF, dtype=torch.int64, device=dev)

with cgamd.Context(0) as ctx:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    ctx.rast_set_scene()
    rows = cgamd.load().cg_rt_shard_rows(H, None)
    assert rows == H, "the float frames are packed W * H apart"
    rgba = torch.zeros(NF * PX * 4, dtype=torch.float32, device=dev)
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, 1080.0)] * NF, rgba.data_ptr(), pix_format=cgamd.PIX_RGBA_F32,
                                stream=st.cuda_stream)
    torch.cuda.synchronize(dev)

    def encode(frames, typ, comp, nf=NF, alpha=RT_ALPHA):
        return lambda: ctx.image_encode_exr_device(frames.data_ptr(), W, H, nf, d_out.data_ptr(), slot, d_bytes.data_ptr(),
                                                   cgamd.EXR_RGBA, typ, comp, alpha, stream=st.cuda_stream)

    # (a) the encoder alone, beside the pack kernel and the PNG encoder
    d_scales = torch.ones(NF, dtype=torch.float32, device=dev)
    d_argb = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
    result["rt_tonemap_pack_kernel_us_per_frame"] = spread(event_us(
        lambda: ctx.rt_tonemap_pack_device(rgba.data_ptr(), PX, NF, d_scales.data_ptr(), d_argb.data_ptr(),
                                           cgamd.TONE_REINHARD, stream=st.cuda_stream), NF))
    png_slot = cgamd.image_png_bound(W, H, cgamd.PNG_RGB)
    result["png_rgb_adaptive_us_per_frame"] = spread(event_us(
        lambda: ctx.image_encode_png_device(d_argb.data_ptr(), W, H, NF, d_out.data_ptr(), png_slot, d_bytes.data_ptr(),
                                            cgamd.PNG_RGB, cgamd.PNG_FILTER_ADAPTIVE, stream=st.cuda_stream), NF))
    del d_argb
    result["encoder"] = {}
    for name, typ, comp in VARIANTS:
        us = spread(event_us(encode(rgba, typ, comp), NF))
        lens = d_bytes.cpu().numpy()
        # (b) the split, from the library's own per-kernel timing over three more calls
        cgamd.kernel_timing(True)
        for _ in range(3):
            encode(rgba, typ, comp)()
        torch.cuda.synchronize(dev)
        split = {k: 1e3 * cgamd.kernel_time(k)[0] / (3 * NF) for k in KERNELS}
        cgamd.kernel_timing(False)
        result["encoder"][name] = {"us_per_frame": us, "bytes_per_frame": float(lens.mean()), "kernel_us_per_frame": split}
        print(name, json.dumps(result["encoder"][name]), flush=True)

    # (c) file sizes and the share of raw chunks, RGBA half ZIP, one frame a call
    def size_of(frame_tensor, alpha):
        encode(frame_tensor, cgamd.EXR_HALF, cgamd.EXR_ZIP, 1, alpha)()
        torch.cuda.synchronize(dev)
        nbytes = int(d_bytes.cpu().numpy()[0])
        got = exr_enc_ref.read(d_out[:nbytes].cpu().numpy().tobytes())
        return {"bytes": nbytes, "chunks": got["chunks"], "raw_chunks": got["raw_chunks"]}

    one = torch.zeros(PX * 4, dtype=torch.float32, device=dev)
    sizes = {"rt_c2": size_of(rgba, RT_ALPHA)}
    c, s_ = f32(math.cos(0.3)), f32(math.sin(0.3))
    yaw = cgamd.rt_camera(W, H, 1080.0, R=(C.c_float * 16)(c, 0, s_, 0, 0, 1, 0, 0, -s_, 0, c, 0, 0, 0, 0, 1))
    ctx.rt_render_frames_device([yaw], one.data_ptr(), pix_format=cgamd.PIX_RGBA_F32, stream=st.cuda_stream)
    sizes["rt_yawed"] = size_of(one, RT_ALPHA)
    d_info = torch.zeros((NF + 1) * 3, dtype=torch.int64, device=dev)
    for mode in (0, 1):
        p = cgamd.rast_params(W, H, 768.0)
        p.colour_mode = mode
        ctx.rast_draw_sequence_picture_device([p], one.data_ptr(), d_info=d_info.data_ptr(), stream=st.cuda_stream)
        sizes[f"rast_mode{mode}"] = size_of(one, 1.0)
    result["files_rgba_half_zip"] = sizes
    result["raw_float_bytes_per_frame"] = PX * 16
    result["raw_half_bytes_per_frame"] = PX * 8
    print("files", json.dumps(sizes), flush=True)
    del rgba, one

    # (d) files against the raw float baseline and 8-bit raw delivery
    states = [cgamd.rt_camera(W, H, 1080.0, (0.0, 0.0, f32(-3.0 + 0.005 * k), 1.0)) for k in range(SEQ)]
    lights = [cgamd.default_lights()] * SEQ
    rast_ps = [cgamd.rast_params(W, H, 768.0, (0.0, 0.0, f32(-3.001 + 0.01 * k), 1.0)) for k in range(SEQ)]
    chunk = [torch.zeros(NF * PX * 4, dtype=torch.float32, device=dev) for _ in range(2)]

    def float_baseline(render, host):
        """Chunks of NF float pictures rendered on `st` into two buffers in turn, each copied whole to
        `host` on `cp` while the next renders; returns when all of them are there."""
        def run():
            done = [None, None]
            for j in range(0, SEQ, NF):
                s = (j // NF) & 1
                if done[s] is not None:
                    st.wait_event(done[s])
                render(j, chunk[s])
                ready = torch.cuda.Event()
                ready.record(st)
                cp.wait_event(ready)
                with torch.cuda.stream(cp):
                    host[j * PX * 4:(j + NF) * PX * 4].copy_(chunk[s], non_blocking=True)
                    done[s] = torch.cuda.Event()
                    done[s].record(cp)
            torch.cuda.synchronize(dev)
        return run

    rt_render = lambda j, buf: ctx.rt_render_sequence_device(   # noqa: E731
        states[j:j + NF], lights[j:j + NF], buf.data_ptr(), pix_format=cgamd.PIX_RGBA_F32, stream=st.cuda_stream)
    rast_render = lambda j, buf: ctx.rast_draw_sequence_picture_device(   # noqa: E731
        rast_ps[j:j + NF], buf.data_ptr(), d_info=d_info.data_ptr(), stream=st.cuda_stream)
    raw_page = np.zeros(SEQ * PX, np.uint32)
    raw_pin = torch.zeros(SEQ * PX, dtype=torch.int32).pin_memory()
    float_page = torch.zeros(SEQ * PX * 4, dtype=torch.float32)
    float_pin = torch.zeros(SEQ * PX * 4, dtype=torch.float32).pin_memory()
    cap = SEQ * cgamd.image_exr_bound(W, H, cgamd.EXR_RGBA, cgamd.EXR_HALF)   # holds the NONE files exactly
    file_page = np.zeros(cap, np.uint8)
    file_pin = torch.zeros(cap, dtype=torch.uint8).pin_memory()
    offs = np.zeros(SEQ + 1, np.uint64)
    offs_p = C.cast(offs.ctypes.data, C.POINTER(C.c_size_t))
    larr, n_lights = cgamd.sequence_lights(lights)
    cam_arr = (cgamd.RtCamera * SEQ)(*states)
    rast_arr = (cgamd.RastParams * SEQ)(*rast_ps)

    def exr_rt(out_ptr, comp=cgamd.EXR_ZIP):
        """The C call itself: the binding's list of files would copy every byte once more."""
        prm = cgamd.ExrParams(cgamd.EXR_RGBA, cgamd.EXR_HALF, comp, RT_ALPHA)

        def run():
            rc = ctx.lib.cg_rt_render_sequence_exr(ctx.h, larr, n_lights, cam_arr, SEQ, C.byref(prm), cgamd.P(out_ptr), cap,
                                                   offs_p, 0, None)
            assert rc == cgamd.CG_OK, rc
        return run

    def exr_rast(out_ptr, comp=cgamd.EXR_ZIP):
        prm = cgamd.ExrParams(cgamd.EXR_RGBA, cgamd.EXR_HALF, comp, 1.0)

        def run():
            rc = ctx.lib.cg_rast_draw_sequence_exr(ctx.h, rast_arr, SEQ, C.byref(prm), cgamd.P(out_ptr), cap, offs_p, 0, None,
                                                   None)
            assert rc == cgamd.CG_OK, rc
        return run

    rt_legs = {
        "raw8_pageable": lambda: ctx.rt_render_sequence(states, lights, out=raw_page),
        "float_pageable": float_baseline(rt_render, float_page),
        "exr_pageable": exr_rt(file_page.ctypes.data),
        "exr_none_pageable": exr_rt(file_page.ctypes.data, cgamd.EXR_NONE),
        "raw8_pinned": lambda: ctx.rt_render_sequence(states, lights, out=raw_pin),
        "float_pinned": float_baseline(rt_render, float_pin),
        "exr_pinned": exr_rt(file_pin.data_ptr()),
        "exr_none_pinned": exr_rt(file_pin.data_ptr(), cgamd.EXR_NONE),
    }
    fps = windows(rt_legs, SEQ)
    rt_legs["exr_pinned"]()
    result["rt_sequence"] = {"frames_per_s": fps, "bytes_per_frame": int(offs[SEQ]) / SEQ,
                             "exr_over_float_pageable": fps["exr_pageable"]["median"] / fps["float_pageable"]["median"],
                             "exr_over_float_pinned": fps["exr_pinned"]["median"] / fps["float_pinned"]["median"]}
    print("rt_sequence", json.dumps(result["rt_sequence"]), flush=True)
    rast_legs = {
        "raw8_pageable": lambda: ctx.rast_draw_sequence(rast_ps, out=raw_page),
        "float_pageable": float_baseline(rast_render, float_page),
        "exr_pageable": exr_rast(file_page.ctypes.data),
        "exr_none_pageable": exr_rast(file_page.ctypes.data, cgamd.EXR_NONE),
        "raw8_pinned": lambda: ctx.rast_draw_sequence(rast_ps, out=raw_pin),
        "float_pinned": float_baseline(rast_render, float_pin),
        "exr_pinned": exr_rast(file_pin.data_ptr()),
        "exr_none_pinned": exr_rast(file_pin.data_ptr(), cgamd.EXR_NONE),
    }
    fps = windows(rast_legs, SEQ)
    rast_legs["exr_pinned"]()
    result["rast_sequence"] = {"frames_per_s": fps, "bytes_per_frame": int(offs[SEQ]) / SEQ,
                               "exr_over_float_pageable": fps["exr_pageable"]["median"] / fps["float_pageable"]["median"],
                               "exr_over_float_pinned": fps["exr_pinned"]["median"] / fps["float_pinned"]["median"]}
    print("rast_sequence", json.dumps(result["rast_sequence"]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
