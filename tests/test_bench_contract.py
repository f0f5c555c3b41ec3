"""CPU: the committed bench lines (latest profiles/rNN_bench_*.json, written by
bench.py on the MI355X) keep the driver's JSON contract: the required keys,
whole-job value = steps / elapsed, roofline and cpu_baseline objects, and the
parity flags the run checked."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config")


def _line(name):
    """The latest committed driver-shaped default line (profiles/rNN_bench_default.json): the C2
    metric line itself for "rt", its C3/C4/C5 sub-record otherwise (the
    contract is pinned on the current line, not on an old per-workload file)."""
    _, d = _default()
    return d if name == "rt" else d[name]


@pytest.mark.parametrize("name", ["rt", "rast", "c4", "c5"])
def test_bench_line_contract(name):
    d = _line(name)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] >= 1 and d["steps"] > 0 and d["value"] > 0
    assert d["higher_is_better"] is True and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6          # value = steps / elapsed
    assert "workload" in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    if r["frac"] is not None:
        assert 0.0 <= r["frac"] <= 1.0, "a roofline fraction is bounded by the peak"
        assert r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    cb = d["cpu_baseline"]
    assert cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["value"] > 0


def _default():
    """The latest committed driver-shaped default line (profiles/rNN_bench_default.json)."""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_default.json")))
    if not paths:
        pytest.skip("no profiles/rNN_bench_default.json collected")
    with open(paths[-1]) as f:
        return os.path.basename(paths[-1])[:3], json.loads(f.read().strip().splitlines()[-1])


def test_default_line_pins_every_config():
    """The default line (what the driver runs) carries C2 and the C3/C4/C5 sub-records, each
    with its roofline, its CPU baseline compared with the GPU's pixels, and its parity flags."""
    rnd, d = _default()
    for k in REQUIRED:
        assert k in d, k
    assert d["frame_sha256_matches_golden"] is True and d["frames_identical_in_call"] is True
    assert d["cpu_baseline"]["frame_matches_gpu"] is True
    for name in ("c4", "c5"):
        s = d[name]
        assert s["value"] > 0 and s["frames_identical_in_call"] is True
        assert s["cpu_baseline"]["sample_matches_gpu"] is True and s["cpu_baseline"]["value"] > 0
        assert "frac" in s["roofline"]
    assert d["rast"]["cpu_baseline"]["frame_matches_gpu"] is True and d["rast"]["frames_identical_in_batch"] is True


def test_default_line_roofline_is_the_kernels_own():
    """each workload's dominant-kernel fraction is its SQ lane-ops over that
    kernel's own live HIP-event time (frac), beside the call-span figure (frac_call) and the whole
    frame's (frac_frame); C5's CPU baseline is SURVEY 8d's 1,024-pixel stratified sample."""
    rnd, d = _default()
    if rnd < "r04":
        pytest.skip("the kernel-own fractions start with round 4's bench")
    for r, kern in ((d, "rt_lattice_kernel"), (d["c4"], "rt_lattice_lights_kernel"), (d["c5"], "rt_big_primary_kernel")):
        ro = r["roofline"]
        assert ro["kernel"] == kern and ro["kernel_ms"] > 0 and ro["kernel_launches"] >= 1
        assert ro["frac"] is not None and 0 < ro["frac"] <= 1
        assert ro["frac"] == pytest.approx(ro["achieved"] / ro["peak"])
        assert ro["frac_frame"] is not None and 0 < ro["frac_frame"] <= 1
        if ro.get("frac_call") is not None:
            assert ro["frac_call"] <= ro["frac"] * 1.001      # the call's span includes the kernel's
        live = r["kernel_ms_live"][kern]
        assert live["busy_ms"] / live["launches"] == pytest.approx(ro["kernel_ms"])
        assert live["busy_ms"] <= live["total_ms"] * (1 + 1e-9)
    if rnd >= "r05":   # every fraction also on the committed rocprofv3 mean
        for r in (d, d["c4"], d["c5"]):
            fp = r["roofline"]["frac_profile_mean"]
            assert fp is not None and 0 < fp <= 1 and "kernel_stats.csv" in r["roofline"]["frac_profile_mean_note"]
        assert d["c5"]["roofline"]["frac_profile_mean"] >= 0.30   # the C5 walk
    assert d["c5"]["cpu_baseline"]["sampled_pixels"] >= 1024
    assert d["c5"]["cpu_baseline"]["threads"] >= 1 and d["c5"]["cpu_baseline"]["cores"] == 1


def test_default_line_measures_the_boundary():
    """the host-buffer Draw (cg_rt_render / cg_rt_render_frames), pageable and
    pinned, single frame and pipelined, every frame golden."""
    rnd, d = _default()
    if rnd < "r04":
        pytest.skip("the draw record starts with round 4's bench")
    dr = d["draw"]
    assert dr["all_frames_golden"] is True
    assert dr["single_frame_ms"] > 0 and dr["fps_pageable"] > 0 and dr["fps_pinned"] > 0
    assert dr["fps_pinned"] < d["value"]          # the PCIe copy is never free


def test_headline_line_checks_parity_and_roofline():
    d = _line("rt")
    assert d["metric"].startswith("frames/sec") and d["unit"] == "frames/s"
    assert d["frame_sha256_matches_golden"] is True and d["cpu_baseline"]["frame_matches_gpu"] is True
    r = d["roofline"]
    assert r["bound"] == "valu" and r["peak"] == pytest.approx(78.6432)       # no-FMA wave64 issue peak
    assert 0 < r["frac"] <= 1 and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    assert 0 < r["hbm_frac"] <= 1
    assert r["traffic"] > r["hbm_algorithmic_bytes_per_launch"] * 0.9     # PMC bytes >= the output written
    assert r["effective_vs_bruteforce"]["algorithmic_ops_per_launch"] > 0
    # the default line also pins C3 (the rasteriser) with its own roofline and CPU baseline
    c3 = d["rast"]
    assert c3["value"] > 0 and c3["single_frame_ms"] > 0 and 0 < c3["roofline"]["frac"] <= 1
    assert c3["cpu_baseline"]["frame_matches_gpu"] is True


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_roofline_frac_is_tied_to_the_profiled_machine_code(monkeypatch):
    """the executed-work fraction scales SQ counters of one build of a
    kernel; a profile whose code_sha256 differs from this build's kernel code nulls it."""
    import cgamd
    import codeobj
    if not os.path.exists(cgamd.LIB_PATH):
        pytest.skip("libcgamd.so not built")
    b = _bench()
    have = codeobj.kernel_sha256("rt_lattice_kernel", cgamd.LIB_PATH)
    assert have and len(have) == 64
    prof = {"valu_lane_ops_per_launch": 5.7e10, "frames_per_launch": 32, "wave_state_frac": {}}
    monkeypatch.setattr(b, "load_sq", lambda kernel, section="rt": dict(prof, code_sha256="0" * 64))
    r = b.valu_roofline("rt_lattice_kernel", "rt", 32, 1.0, 1.5)
    assert r["frac"] is None and r["achieved"] is None and "re-profile" in r["frac_null_reason"]
    monkeypatch.setattr(b, "load_sq", lambda kernel, section="rt": dict(prof))          # no hash recorded
    assert b.valu_roofline("rt_lattice_kernel", "rt", 32, 1.0, 1.5)["frac"] is None
    monkeypatch.setattr(b, "load_sq", lambda kernel, section="rt": dict(prof, code_sha256=have))
    r = b.valu_roofline("rt_lattice_kernel", "rt", 32, 1.0, 1.5)
    assert r["frac"] == pytest.approx(5.7e10 / 1.5e-3 / 1e12 / r["peak"])


def test_kernel_hash_tracks_machine_code():
    """Template instances are hashed together, unknown kernels have no hash, and different
    kernels hash differently."""
    import cgamd
    import codeobj
    if not os.path.exists(cgamd.LIB_PATH):
        pytest.skip("libcgamd.so not built")
    hs = {k: codeobj.kernel_sha256(k, cgamd.LIB_PATH)
          for k in ("rt_lattice_kernel", "rt_lattice_lights_kernel", "rt_big_primary_kernel", "rast_fill_kernel")}
    assert all(hs.values()) and len(set(hs.values())) == len(hs)
    assert codeobj.kernel_sha256("no_such_kernel", cgamd.LIB_PATH) is None


def test_kernel_hash_ignores_descriptor_layout(monkeypatch):
    """The descriptor's code-entry offset (bytes 16-23: where the code sits, which moves when
    another kernel of the code object changes size) does not change the hash; the code bytes
    and the rest of the descriptor (registers, LDS, scratch) do."""
    import codeobj
    kd = bytes(range(64))
    base = {"_Z9my_kernelv": b"\x01\x02\x03\x04", "_Z9my_kernelv.kd": kd}

    def h(syms):
        monkeypatch.setattr(codeobj, "kernel_symbols", lambda lib_path=None: syms)
        return codeobj.kernel_sha256("my_kernel")
    moved = dict(base, **{"_Z9my_kernelv.kd": kd[:16] + b"\xff" * 8 + kd[24:]})
    regs = dict(base, **{"_Z9my_kernelv.kd": kd[:48] + b"\xff" + kd[49:]})
    code = dict(base, **{"_Z9my_kernelv": b"\x01\x02\x03\x05"})
    assert h(base) == h(moved)
    assert h(base) != h(regs) and h(base) != h(code)


def test_stratified_sample_covers_the_whole_frame():
    """C4/C5 CPU baselines: a fixed stratified sample -- one pixel
    per cell of an n x n grid over the whole frame, C5's 1,024 pixels -- every cell once, inside
    the frame, reaching both borders' cells."""
    b = _bench()
    for W, H, n in ((1920, 1080, 32), (3840, 2160, 128)):
        xy = b.stratified_pixels(W, H, n)
        assert len(xy) == n * n and len({(x, y) for x, y in xy}) == n * n
        assert xy[:, 0].min() >= 0 and xy[:, 0].max() < W and xy[:, 1].min() >= 0 and xy[:, 1].max() < H
        cells = {(x * n // W, y * n // H) for x, y in xy}
        assert cells == {(i, j) for i in range(n) for j in range(n)}
    assert b.CPU_STRATA["c5"] ** 2 == 1024


def test_cpu_info_reports_physical_cores():
    b = _bench()
    ci = b.cpu_info()
    assert 1 <= ci["usable_cores"] <= ci["physical_cores"] <= ci["logical_cpus"]


def test_default_line_useful_fraction_matches_counts():
    """C2's, C4's and C5's dominant-kernel rooflines carry useful_frac, the
    reference's own per-ray arithmetic the kernel performs over its time; its op count per frame is
    the committed counts file's (profiles/rNN_work_counts.json, scripts/work_counts.py) recomputed
    with SURVEY 8d's weights."""
    import glob
    rnd, d = _default()
    if rnd < "r06":
        pytest.skip("useful_frac starts with round 6's bench")
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_work_counts.json")))
    assert paths, "no committed work counts"
    with open(paths[-1]) as f:
        wc = json.load(f)
    weights = wc["weights"]
    for name, r in (("rt", d), ("c4", d["c4"]), ("c5", d["c5"])):
        ro, w = r["roofline"], wc["workloads"][name]
        assert w["dominant_kernel"] == ro["kernel"]
        ops = sum(weights[k] * w["counts_per_frame"][k] for k in w["dominant_kinds"])
        assert ops == pytest.approx(w["useful_ops_per_frame"])
        assert ro["useful_ops_per_frame"] == pytest.approx(ops)
        assert ro["useful_counts_file"] == "profiles/" + os.path.basename(paths[-1])
        assert 0 < ro["useful_frac"] <= 1
        assert ro["useful_frac"] == pytest.approx(ro["useful_achieved"] / ro["peak"])


def test_dump_outputs_formats_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: integer outputs as float64 (exact for a uint32 pixel), float ones as float32,
    whole and in shape under the byte budget; over it, the same seeded sample of every output's
    elements (in index order) from run to run, within the budget in all."""
    b = _bench()
    argb = np.arange(0xFFFFFF00, 0xFFFFFF00 + 96, dtype=np.uint64).astype(np.uint32).reshape(8, 12)
    depth = np.linspace(0.0, 1.0, 96, dtype=np.float32).reshape(8, 12)
    b.dump_outputs(str(tmp_path / "a"), {"argb": argb, "depth": depth})
    a, d = np.load(tmp_path / "a" / "argb.npy"), np.load(tmp_path / "a" / "depth.npy")
    assert a.dtype == np.float64 and a.shape == (8, 12) and np.array_equal(a.astype(np.uint32), argb)
    assert d.dtype == np.float32 and np.array_equal(d, depth)
    monkeypatch.setattr(b, "DUMP_BUDGET", 600)           # 96 x 8 + 96 x 4 = 1152 bytes: over
    b.dump_outputs(str(tmp_path / "b"), {"argb": argb, "depth": depth})
    b.dump_outputs(str(tmp_path / "c"), {"argb": argb + 0, "depth": depth})
    sb, sc = np.load(tmp_path / "b" / "argb.npy"), np.load(tmp_path / "c" / "argb.npy")
    assert np.array_equal(sb, sc) and 0 < sb.size < 96 and set(sb) <= set(a.reshape(-1))
    assert np.all(np.diff(sb) > 0)                       # index order of an increasing array
    assert sb.nbytes + np.load(tmp_path / "b" / "depth.npy").nbytes <= 600


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_frame(tmp_path, monkeypatch, capsys, golden):
    """A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line whose
    value and ms_per_step are of exactly K timed steps, without the records of --full, and the last
    step's frame in DIR/argb.npy as float64 -- the C2 golden frame, identical run to run."""
    import hashlib
    import sys
    import torch
    b = _bench()
    for run in ("a", "b"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2",
                                          "--dump-outputs", str(tmp_path / run)])
        try:
            b.main()
        finally:
            torch.cuda.set_stream(torch.cuda.default_stream())
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 2
    d = json.loads(lines[-1])
    for k in REQUIRED:
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["dtype"] == "f32"
    assert d["metric"].startswith("frames/sec") and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6
    assert d["kernel_ms_live"]["rt_lattice_kernel"]["launches"] >= 1      # the live kernel timing stays on
    for k in ("roofline", "cpu_baseline", "draw", "steady_fps_info", "rast", "c4", "c5", "frame_sha256_matches_golden"):
        assert k not in d, k
    fa, fb = np.load(tmp_path / "a" / "argb.npy"), np.load(tmp_path / "b" / "argb.npy")
    assert fa.dtype == np.float64 and fa.shape == (1080, 1920) and np.array_equal(fa, fb)
    want = golden["rt"]["rt_1920x1080_f1080"]["argb_sha256"]
    assert hashlib.sha256(fa.astype(np.uint32).tobytes()).hexdigest() == want
