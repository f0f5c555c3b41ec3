"""Frame rate, phase times and scratch of the rasteriser's compact route (cg_rast_big.hip).
cg_rast_draw_device at 1920 x 1080, focal 768, colour mode 0 (and, with --colour-modes, the random
scenes in modes 1-2 beside it on the same build: legs random_<n>_mode<m>, their time over mode 0's):
  reference scene   the dense route against the forced compact route: what the indirection
                    and the compact route's three host waits cost on a small frame;
  random scenes     cg_rast_random_scene(0x5EED, n, 0.02) as the room, n = 1e4, 1e5, 1e6, on the
                    automatic (compact) route.
Every leg is warmed up, then timed over windows of about --window seconds; the legs alternate
and each window is closed by a device synchronise; medians over --repeats windows.  Per leg:
frames/s, the phases' milliseconds from HIP events (cg_kernel_timing: rast_big_clip / _setup /
_rows / _fill / _post, in modes 1-2 also _count / _rand / _shade; each a scope over its launches),
cg_rast_scratch_info, and the row-list
pass's work (spans tested and records written) beside the dense formulas H x 32 n_in header
tests and 2560 n_in H bytes.  The 1e6 scene is also rendered once at 96 x 54 on both routes
and compared whole.  Usage:
  python scripts/rast_big_rate.py [--repeats 3] [--window 0.5] [--sizes 10000,100000,1000000]
                                  [--colour-modes 0,1] [--out profiles/rast_big_rate.json]"""
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
ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
ap.add_argument("--sizes", default="10000,100000,1000000")
ap.add_argument("--colour-modes", default="0", help="colour modes of the random scenes' legs, e.g. 0,1")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rast_big_rate.json"))
args = ap.parse_args()

W, H, F = 1920, 1080, 768.0
PHASES = ("rast_big_clip", "rast_big_setup", "rast_big_rows", "rast_big_fill", "rast_big_post")
COLOUR_PHASES = ("rast_big_count", "rast_big_rand", "rast_big_shade")
DENSE_KERNELS = ("rast_fill_kernel", "rast_post_kernel")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
p = cgamd.rast_params(W, H, F)
d_argb = torch.zeros(W * H, dtype=torch.int32, device=dev)
no_boxes = (cgamd.RTri * 1)()
sizes = [int(s) for s in args.sizes.split(",") if s]
modes = [int(m) for m in args.colour_modes.split(",") if m]
batch, chunk = cgamd.rast_row_blocks()
result = {"workload": f"cg_rast_draw_device, {W}x{H}, focal {F}, colour mode 0 (random scenes: modes {modes})", "repeats": args.repeats,
          "window_s": args.window, "row_blocks": {"batch": batch, "chunk": chunk}, "legs": {}}


def window(fn, calls):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize(dev)
    return calls / (time.perf_counter() - t0)


def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[:3], b[:3]))


ctxs = {"reference": cgamd.Context(0)}
ctxs["reference"].rast_set_scene()
n_in = {"reference": 150}
rooms = {}
for n in sizes:
    c = cgamd.Context(0)
    rooms[n] = cgamd.rast_random_scene(n, 0.02, 0x5EED)
    c.rast_set_scene(rooms[n], n, no_boxes, 0)
    ctxs[f"random_{n}"] = c
    n_in[f"random_{n}"] = n


def make_leg(ctx, route, mode=0):
    pm = cgamd.rast_params(W, H, F, colour_mode=mode)

    def fn():
        ctx.rast_set_route(route)
        ctx.rast_draw_device(pm, d_argb.data_ptr())
    return fn


legs = {"reference_dense": (ctxs["reference"], make_leg(ctxs["reference"], cgamd.RAST_ROUTE_DENSE), "reference"),
        "reference_compact": (ctxs["reference"], make_leg(ctxs["reference"], cgamd.RAST_ROUTE_COMPACT), "reference")}
leg_mode = {}
for n in sizes:
    for m in modes:   # a scene's modes are neighbours in the round: they alternate
        k = f"random_{n}" if m == 0 else f"random_{n}_mode{m}"
        legs[k] = (ctxs[f"random_{n}"], make_leg(ctxs[f"random_{n}"], -1, m), f"random_{n}")
        leg_mode[k] = m

try:
    # the reference frame is the same on both routes before anything is timed
    planes = {}
    for route in (cgamd.RAST_ROUTE_DENSE, cgamd.RAST_ROUTE_COMPACT):
        ctxs["reference"].rast_set_route(route)
        planes[route] = ctxs["reference"].rast_draw(p)
    if not same(planes[0], planes[1]):
        raise SystemExit("reference scene: the routes disagree")

    calls = {}
    for k, (ctx, fn, _) in legs.items():   # warm-up: allocations and code objects, then the calls a window needs
        window(fn, 1)
        r = window(fn, 2)
        calls[k] = max(2, min(20000, int(round(args.window * r))))
    rates = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, (ctx, fn, _) in legs.items():
            rates[k].append(window(fn, calls[k]))

    for k, (ctx, fn, scene) in legs.items():
        frames = 5
        cgamd.kernel_timing(True)
        for _ in range(frames):
            fn()
        torch.cuda.synchronize(dev)
        names = DENSE_KERNELS if k == "reference_dense" else PHASES + (COLOUR_PHASES if leg_mode.get(k, 0) else ())
        phase_ms = {nm: cgamd.kernel_time(nm)[0] / frames for nm in names}
        cgamd.kernel_timing(False)
        info = ctx.rast_scratch_info()
        ni = n_in[scene]
        v = rates[k]
        result["legs"][k] = {
            "calls_per_window": calls[k],
            "frames_per_s": {"median": statistics.median(v), "min": min(v), "max": max(v)},
            "ms_per_frame": 1e3 / statistics.median(v),
            "phase_ms": phase_ms,
            "scratch": info,
            "n_in": ni,
            "colour_mode": leg_mode.get(k, 0),
            "dense_formula_bytes": 2560 * ni * H,
            "row_list_work": {"dense_header_tests": H * 32 * ni, "spans_tested": info["spans"],
                              "records_written": info["recs"], "chunks": -(-info["spans"] // chunk)},
        }
    ref = result["legs"]
    result["compact_over_dense_reference"] = (ref["reference_compact"]["frames_per_s"]["median"]
                                               / ref["reference_dense"]["frames_per_s"]["median"])

    # modes 1-2 beside mode 0 on the same scene: frame time over mode 0's, and the fragments that drew
    for k, m in leg_mode.items():
        base = k.split("_mode")[0]
        if m == 0 or base not in ref:
            continue
        ctx = legs[k][0]
        ctx.rast_set_route(-1)
        ref[k]["n_shaded"] = ctx.rast_draw(cgamd.rast_params(W, H, F, colour_mode=m))[3].n_shaded
        ref[k]["ms_over_mode_0"] = ref[k]["ms_per_frame"] / ref[base]["ms_per_frame"]

    # the largest scene once more at 96 x 54, both routes, compared whole
    if sizes:
        n = max(sizes)
        ctx = ctxs[f"random_{n}"]
        ps = cgamd.rast_params(96, 54, 38.4)
        tris, nc, light = cgamd.rast_prepare(ps, rooms[n], n, no_boxes, 0)
        need = nc * 54 * 80 + nc * (84 + 32)
        free = torch.cuda.mem_get_info(dev)[0]
        whole = {"n_in": n, "clipped": nc, "dense_scratch_bytes": need, "free_bytes": free}
        if need < 0.8 * free:
            ctx.rast_set_route(-1)
            got = ctx.rast_draw(ps)
            whole["compact_scratch"] = ctx.rast_scratch_info()
            ctx.rast_set_route(cgamd.RAST_ROUTE_DENSE)
            want = ctx.rast_render(tris, nc, ps, light)
            ctx.rast_set_route(-1)
            whole["equal"] = bool(same(got, want))
            if not whole["equal"]:
                raise SystemExit(f"{n} triangles at 96x54: the routes disagree")
        else:
            whole["equal"] = None   # the dense render does not fit beside the rest
        result["whole_frame_check_96x54"] = whole
finally:
    for c in ctxs.values():
        c.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
