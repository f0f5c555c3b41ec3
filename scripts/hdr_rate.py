"""What the exposure chain costs, at 1920 x 1080 on one GPU.

1. cg_hdr_histogram_device (its clear launch and its histogram launch, d_stats NULL) on one
   CG_PIX_RGBA_F32 frame of three kinds -- (a) a rendered C2 frame, (b) luminances spread evenly
   over every bin, (c) every pixel in one bin -- beside cg_rt_pack_radiance_device and
   cg_rt_tonemap_pack_device on the same frame in the same run: HIP events around 50 calls, the
   median of --repeats rounds.  Both kernels read the same 33.2 MB once.  Also eight rendered frames
   in one call, as a chunk of cg_rt_render_exposed_device has them, per frame.  With --peels the
   histogram part runs again in a child process per value of CG_HDR_PEEL (the merge rounds before
   the LDS add; 0 = none), the variants of the design.
2. cg_rt_render_exposed_device against cg_rt_render_frames_device in CG_PIX_ARGB8888, 20 frames a
   call, on C2, on C2 after one yaw key and on cg_rt_random_scene(0x5EED, N): windows of about one
   second of enqueued calls closed by a device synchronise, the two alternating, medians of
   --repeats windows.  Expected extra traffic per frame: the float store (33.2 MB) instead of the
   ARGB store (8.3 MB), one read for the histogram (33.2 MB), one read (33.2 MB) and one ARGB store
   (8.3 MB) for the pack.
Usage: python scripts/hdr_rate.py [--repeats 5] [--tris 1000000] [--peels 0,1,2,4] [--out profiles/hdr_rate.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "computer-graphics_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--peels", default="0,1,2,4")
ap.add_argument("--histogram-only", action="store_true", help="part 1 only, JSON on the last line (the children of --peels)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdr_rate.json"))
args = ap.parse_args()
if args.repeats < 3:
    raise SystemExit("--repeats must be at least 3 (medians)")

variants = {}
if not args.histogram_only and args.peels:
    for peel in args.peels.split(","):          # before this process opens the GPU: one process at a time
        env = dict(os.environ, CG_HDR_PEEL=peel)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--histogram-only", "--repeats", str(args.repeats)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"CG_HDR_PEEL={peel} child failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        variants[peel] = json.loads(r.stdout.strip().splitlines()[-1])["histogram_us"]
        print(f"CG_HDR_PEEL={peel}: {variants[peel]}", flush=True)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cgamd  # noqa: E402

W, H, F = 1920, 1080, 1080.0
PX = W * H
NF = 20
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ctx = cgamd.Context(0)
result = {"workload": f"exposure chain at {W}x{H} on one GPU", "repeats": args.repeats, "window_s": args.window_s,
          "bytes_per_frame": {"argb": PX * 4, "f32": PX * 16}, "peel_default": int(os.environ.get("CG_HDR_PEEL", "1"))}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_us(call, stream, n=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for r in range(args.repeats + 1):
        e0.record(stream)
        for _ in range(n):
            call()
        e1.record(stream)
        stream.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / n)
    return us[1:]                                # the first round loads the code object


def histogram_part():
    rng = np.random.default_rng(5)
    rendered = torch.zeros(PX * 4, dtype=torch.float32, device=dev)
    ctx.rt_render_frames_device([cgamd.rt_camera(W, H, F)], rendered.data_ptr(), pix_format=cgamd.PIX_RGBA_F32)
    g = rng.integers(0x37800000, 0x47800000, PX).astype(np.uint32).view(np.float32)   # every bin as often
    uniform = torch.from_numpy(np.stack([g, g, g, np.ones(PX, np.float32)], axis=1).reshape(-1).copy()).to(dev)
    one_bin = torch.ones(PX * 4, dtype=torch.float32, device=dev)
    d_hist = torch.zeros(256, dtype=torch.int32, device=dev)
    d_argb = torch.zeros(PX, dtype=torch.int32, device=dev)
    d_one = torch.ones(1, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    out = {"histogram_us": {}, "bins_hit": {}}
    for name, buf in (("rendered_c2", rendered), ("uniform_bins", uniform), ("one_bin", one_bin)):
        us = event_us(lambda: ctx.hdr_histogram_device(buf.data_ptr(), 4, PX, 1, d_hist.data_ptr(), stream=s.cuda_stream), s)
        out["histogram_us"][name] = spread(us)
        h = d_hist.cpu().numpy()
        out["bins_hit"][name] = {"bins": int((h > 0).sum()), "counted": int(h.sum()), "largest_bin_share": float(h.max() / max(1, h.sum()))}
    # the chain's own shape: the 8 frames of one chunk in one call, per frame
    eight = rendered.repeat(8)
    d_hist8 = torch.zeros(8 * 256, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    us = event_us(lambda: ctx.hdr_histogram_device(eight.data_ptr(), 4, PX, 8, d_hist8.data_ptr(), stream=s.cuda_stream), s, 20)
    out["histogram_us"]["rendered_c2_8_frames_per_frame"] = spread([u / 8 for u in us])
    del eight
    if args.histogram_only:
        return out
    pk = event_us(lambda: ctx.rt_pack_radiance_device(rendered.data_ptr(), PX, d_argb.data_ptr(), 1.0, stream=s.cuda_stream), s)
    tp = event_us(lambda: ctx.rt_tonemap_pack_device(rendered.data_ptr(), PX, 1, d_one.data_ptr(), d_argb.data_ptr(),
                                                     cgamd.TONE_REINHARD, stream=s.cuda_stream), s)
    out["pack_radiance_us"] = spread(pk)
    out["tonemap_pack_reinhard_us"] = spread(tp)
    p, u = statistics.median(pk), out["histogram_us"]["uniform_bins"]["median"]
    out["histogram_over_pack_radiance"] = {k: v["median"] / p for k, v in out["histogram_us"].items()}
    out["histogram_over_uniform_bins"] = {k: v["median"] / u for k, v in out["histogram_us"].items() if "8_frames" not in k}
    out["histogram_gb_per_s"] = {k: PX * 16 / (v["median"] * 1e-6) / 1e9 for k, v in out["histogram_us"].items()}
    out["pack_radiance_gb_per_s"] = PX * 20 / (p * 1e-6) / 1e9
    return out


def window(call, calls):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def exposed_part(name, cam, d_argb, d_scales):
    cams = [cam] * NF
    params = cgamd.hdr_params(permille=990, target=1.0, rate=0.5)
    call = {"plain": lambda: ctx.rt_render_frames_device(cams, d_argb.data_ptr()),
            "exposed": lambda: ctx.rt_render_exposed_device(cams, d_argb.data_ptr(), d_scales.data_ptr(), params,
                                                            op=cgamd.TONE_REINHARD)}
    calls = {}
    for k, fn in call.items():                   # code objects, pools and scratch; then the window's size
        window(fn, 2)
        calls[k] = max(2, int(round(args.window_s / (window(fn, 4) / 4))))
    rate = {k: [] for k in call}
    for r in range(args.repeats):
        for k, fn in call.items():
            rate[k].append(calls[k] * NF / window(fn, calls[k]))
        print(f"{name} repeat {r}: plain {rate['plain'][-1]:.1f} exposed {rate['exposed'][-1]:.1f} frames/s", flush=True)
    p, e = statistics.median(rate["plain"]), statistics.median(rate["exposed"])
    added_us = 1e6 / e - 1e6 / p
    extra = PX * (16 - 4 + 16 + 16 + 4)
    return {"frames_per_call": NF, "calls_per_window": calls, "plain_frames_per_s": spread(rate["plain"]),
            "exposed_frames_per_s": spread(rate["exposed"]), "added_us_per_frame": added_us,
            "expected_extra_bytes_per_frame": extra, "achieved_gb_per_s_on_extra_bytes": extra / (added_us * 1e-6) / 1e9}


try:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    result.update(histogram_part())
    if not args.histogram_only:
        result["histogram_us_by_peel"] = variants
        d_argb = torch.zeros(NF * PX, dtype=torch.int32, device=dev)
        d_scales = torch.zeros(NF, dtype=torch.float32, device=dev)
        result["exposed"] = {}
        result["exposed"]["c2"] = exposed_part("c2", cgamd.rt_camera(W, H, F), d_argb, d_scales)
        yaw = float(np.float32(0.0) - np.float32(0.174533))
        result["exposed"]["c2_yaw"] = exposed_part("c2_yaw", cgamd.rt_camera(W, H, F, R=cgamd.yaw_matrix(yaw)), d_argb, d_scales)
        big = torch.from_numpy(np.frombuffer(cgamd.random_scene(args.tris), np.float32).reshape(args.tris, 19).copy()).to(dev)
        ctx.rt_set_scene_device(big.data_ptr(), args.tris)
        result["exposed"][f"random_{args.tris}"] = exposed_part(f"random_{args.tris}", cgamd.rt_camera(W, H, F), d_argb, d_scales)
finally:
    ctx.close()

if not args.histogram_only:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
