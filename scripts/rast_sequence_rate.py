"""Frame rate of a colour-mode-1 frame sequence, two ways in one process:
  (a) a loop of cg_rast_draw that adds 3 * stats.n_shaded to the rand() offset
      (planes downloaded, the host waits inside every frame);
  (b) one cg_rast_draw_sequence_device call (planes stay on the device, the
      offset is chained on the device);
and, for context, (c) the same poses in colour mode 0 through
cg_rast_draw_frames_device.  Workload: 64 frames of the 1920 x 1080, focal 768
pose, the camera stepping 0.01 in z.  The legs alternate, each closed by a
device synchronise.  Usage:
  python scripts/rast_sequence_rate.py [--frames 64] [--repeats 5] [--out profiles/rast_sequence_rate.json]"""
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
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rast_sequence_rate.json"))
args = ap.parse_args()

W, H, F, N = 1920, 1080, 768.0, args.frames
npx = W * H
f32 = lambda x: float(np.float32(x))   # noqa: E731
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def params(mode):
    return [cgamd.rast_params(W, H, F, (0.0, 0.0, f32(-3.001 + 0.01 * k), 1.0), colour_mode=mode) for k in range(N)]


with cgamd.Context(0) as ctx:
    ctx.rast_set_scene()
    d_a = torch.zeros(N * npx, dtype=torch.int32, device=dev)
    d_d = torch.zeros(N * npx, dtype=torch.float32, device=dev)
    d_s = torch.zeros(N * npx, dtype=torch.int32, device=dev)
    d_info = torch.zeros(3 * (N + 1), dtype=torch.int64, device=dev)
    h_a, h_d, h_s = np.zeros(npx, np.uint32), np.zeros(npx, np.float32), np.zeros(npx, np.int32)
    st = torch.cuda.current_stream(dev)
    p1, p0 = params(1), params(0)

    def leg_loop():
        off, stats = 0, cgamd.Stats()
        for p in p1:
            p.rand_offset = off
            ctx._check(ctx.lib.cg_rast_draw(ctx.h, C.byref(p), h_a.ctypes.data_as(cgamd.P), h_d.ctypes.data_as(cgamd.P),
                                            h_s.ctypes.data_as(cgamd.P), C.byref(stats)), "cg_rast_draw")
            off += 3 * stats.n_shaded
        return off

    def leg_sequence():
        p1[0].rand_offset = 0
        ctx.rast_draw_sequence_device(p1, d_a.data_ptr(), d_d.data_ptr(), d_s.data_ptr(), 0, d_info.data_ptr(),
                                      st.cuda_stream)

    def leg_mode0():
        ctx.rast_draw_frames_device(p0, d_a.data_ptr(), d_d.data_ptr(), d_s.data_ptr(), 0, st.cuda_stream)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        return N / (time.perf_counter() - t0), r

    legs = {"mode0_frames_device": leg_mode0, "loop_rast_draw": leg_loop, "sequence_device": leg_sequence}
    for fn in legs.values():   # every shape once: allocations, tables, code objects
        timed(fn)
    rates = {k: [] for k in legs}
    closing = None
    for _ in range(args.repeats):
        for k, fn in legs.items():
            r, v = timed(fn)
            rates[k].append(r)
            if k == "loop_rast_draw":
                closing = v
    info = d_info.cpu().numpy()
    seq_closing, status = int(info[3 * N]), info[2::3][:N] & 0xffffffff
    last = d_a[(N - 1) * npx:].cpu().numpy().view(np.uint32)
    if seq_closing != closing or status.any() or not np.array_equal(last, h_a):
        raise SystemExit(f"the two legs disagree: closing offset {seq_closing} vs {closing}, statuses {status.tolist()}")

out = {"workload": f"{N} frames {W}x{H} focal {F}, camera z -3.001 + 0.01 k, colour mode 1", "repeats": args.repeats,
       "closing_rand_offset": closing, "frames_per_s": {
           k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rates.items()}}
out["sequence_over_loop"] = out["frames_per_s"]["sequence_device"]["median"] / out["frames_per_s"]["loop_rast_draw"]["median"]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
