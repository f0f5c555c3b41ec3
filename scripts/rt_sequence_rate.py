"""Frame rate of raytracer key scripts, the sequence call against what a build without it offers.
64 frames at 1920 x 1080, focal 1080, three scripts of Update() keys (one key per frame):
  light: the light moves every frame (d / a);
  focal: the focal length changes every frame (i / o);
  mixed: w U i m m a R n n n o q D e repeated (light, camera, yaw and focal).
Legs (each closed by a device synchronise, after one untimed pass):
  sequence: one cg_rt_render_sequence_device call;
  baseline: the light script as a loop of cg_rt_render_device, the others through
            cg_rt_render_frames_device (one call per stretch of frames that share their lights).
The baseline is measured on a build of the parent commit: --tree names the checkout whose
computer-graphics_amd (binding and library) a run loads, so the two builds alternate as separate
processes; --merge joins the runs' files, checks that both legs gave the same last frame, and
writes the medians and ratios.  Usage:
  python scripts/rt_sequence_rate.py --legs baseline --tree ../parent --build "parent commit" --out a1.json
  python scripts/rt_sequence_rate.py --legs both --out b1.json
  python scripts/rt_sequence_rate.py --merge a1.json b1.json ... --out profiles/rt_sequence_rate.json"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ap = argparse.ArgumentParser()
ap.add_argument("--legs", choices=["baseline", "sequence", "both"], default="both")
ap.add_argument("--tree", default=ROOT, help="the checkout whose build is measured")
ap.add_argument("--build", default=None, help="what to call that build in the files (default: by --tree)")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--merge", nargs="+", metavar="FILE")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_sequence_rate.json"))
args = ap.parse_args()


def merge(files):
    runs = [json.load(open(f)) for f in files]
    out = {"what": "scripts/rt_sequence_rate.py: frames/s of each leg over the merged runs (one process each, in the "
                   "order listed); the baseline legs are those of runs that measured nothing else (the parent "
                   "build), a run of both legs counts its own baseline apart as baseline_this_build",
           "workload": runs[0]["workload"], "repeats_per_run": runs[0]["repeats"],
           "runs": [{"build": r["build"], "legs": r["legs"]} for r in runs], "scripts": {}}
    # the baseline is the parent build's: a run of both legs counts its own baseline apart
    apart = any(r["legs"] == "baseline" for r in runs)
    for name in runs[0]["scripts"]:
        rates, shas = {"baseline": [], "sequence": [], "baseline_this_build": []}, set()
        for r in runs:
            for leg, v in r["scripts"][name]["frames_per_s"].items():
                rates["baseline_this_build" if apart and leg == "baseline" and r["legs"] == "both" else leg] += v
            shas |= set(r["scripts"][name]["last_frame_sha256"].values())
        if len(shas) != 1:
            raise SystemExit(f"{name}: the legs' last frames differ: {sorted(shas)}")
        rec = {leg: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
               for leg, v in rates.items() if v}
        if "baseline" in rec and "sequence" in rec:
            rec["sequence_over_baseline"] = rec["sequence"]["median"] / rec["baseline"]["median"]
        rec["last_frame_sha256"] = shas.pop()
        rec["launch_runs"] = next((r["scripts"][name]["launch_runs"] for r in runs if r["scripts"][name].get("launch_runs")), None)
        out["scripts"][name] = rec
    return out


if args.merge:
    out = merge(args.merge)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(args.tree, "computer-graphics_amd"))
import cgamd  # noqa: E402

W, H, F, N = 1920, 1080, 1080.0, args.frames
F32 = np.float32
LIGHT_KEYS = {"w": (2, 1), "s": (2, -1), "a": (0, -1), "d": (0, 1), "q": (1, -1), "e": (1, 1)}
CAM_KEYS = {"U": (2, 1), "D": (2, -1), "L": (0, -1), "R": (0, 1)}


def states(keys):
    """(camera, light tuple) per key, every state stepped in float32 as Update() steps its globals"""
    cam, light = [F32(0), F32(0), F32(-3), F32(1)], [F32(0), F32(-0.5), F32(-0.7), F32(1)]
    yaw, focal, out = F32(0), F32(F), []
    for k in keys:
        if k in LIGHT_KEYS:
            ax, sg = LIGHT_KEYS[k]
            light[ax] = F32(light[ax] + F32(sg) * F32(0.1))
        elif k in CAM_KEYS:
            ax, sg = CAM_KEYS[k]
            cam[ax] = F32(cam[ax] + F32(sg) * F32(0.1))
        elif k in "nm":
            yaw = F32(yaw + (F32(-0.174533) if k == "n" else F32(0.174533)))
        elif k in "io":
            focal = F32(focal + (F32(10) if k == "i" else F32(-10)))
        R = cgamd.yaw_matrix(float(yaw)) if float(yaw) != 0.0 else None
        out.append((cgamd.rt_camera(W, H, float(focal), tuple(float(x) for x in cam), R), tuple(float(x) for x in light)))
    return out


SCRIPTS = {
    "light": ("ddddaaaa" * N)[:N],
    "focal": ("iiiioooo" * N)[:N],
    "mixed": ("wUimmaRnnnoqDe" * N)[:N],
}


def light_array(pos):
    arr = (cgamd.Light * 1)()
    arr[0].position = cgamd.Vec4(*pos)
    arr[0].colour = cgamd.Vec3(14.0, 14.0, 14.0)
    return arr


dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
npx = W * H
# the build's name, never a path of the measuring machine
build = args.build or ("this commit" if os.path.abspath(args.tree) == os.path.abspath(ROOT) else "parent commit")
result = {"workload": f"{N} frames {W}x{H} focal {F}, one key of Update() per frame", "build": build,
          "legs": args.legs, "repeats": args.repeats, "scripts": {}}
with cgamd.Context(0) as ctx:
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    d_out = torch.zeros(N * npx, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return N / (time.perf_counter() - t0)

    for name, keys in SCRIPTS.items():
        seq = states(keys)
        cams = [c for c, _ in seq]
        arrays = [light_array(p) for _, p in seq]
        stretches = []           # frames that share their lights: one cg_rt_render_frames_device call each
        for f, (_, p) in enumerate(seq):
            if stretches and seq[stretches[-1][0]][1] == p:
                stretches[-1][1] = f + 1
            else:
                stretches.append([f, f + 1])

        def leg_baseline():
            if name == "light":
                for f in range(N):
                    ctx.rt_render_device(cams[f], d_out.data_ptr() + 4 * f * npx, None, st.cuda_stream, arrays[f])
            else:
                for a, b in stretches:
                    ctx.rt_render_frames_device(cams[a:b], d_out.data_ptr() + 4 * a * npx, None, st.cuda_stream, arrays[a])

        def leg_sequence():
            ctx.rt_render_sequence_device(cams, arrays, d_out.data_ptr(), None, st.cuda_stream)

        legs = {"baseline": leg_baseline, "sequence": leg_sequence}
        if args.legs != "both":
            legs = {args.legs: legs[args.legs]}
        rec = {"frames_per_s": {k: [] for k in legs}, "last_frame_sha256": {}, "launch_runs": None}
        if hasattr(cgamd, "rt_sequence_runs"):
            rec["launch_runs"] = [[a, b, r] for a, b, r in cgamd.rt_sequence_runs(cams, n, 1, 1)]
        for k, fn in legs.items():
            d_out.zero_()
            timed(fn)            # untimed: allocations, code objects
            rec["last_frame_sha256"][k] = hashlib.sha256(d_out[(N - 1) * npx:].cpu().numpy().tobytes()).hexdigest()
        for _ in range(args.repeats):
            for k, fn in legs.items():
                rec["frames_per_s"][k].append(timed(fn))
        result["scripts"][name] = rec

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result))
