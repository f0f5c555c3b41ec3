"""GPU: cg_image_decode_jpeg and cg_image_decode_jpeg_device on the files of
tests/test_jpeg_decode.py -- baseline and progressive, restarts, interleaved and
per-component scans, gray / 4:4:4 / 4:2:0, sizes from 1x1 that end inside a block, inside
an MCU and inside a workgroup's 8 (S = 1) or 4 (S = 2) blocks, the IDCT and colour clamps,
the Adobe-RGB and component-id colour rules -- against the oracle element by element, the
Pillow-derived libjpeg 9 hashes and the float64 inverse DCT; then the device entry, the
capacity error, and the grow-only scratch buffer across images of different sizes."""
import os

import numpy as np
import pytest

import cgamd
import jpeg_cases as jc
import oracle

pytestmark = pytest.mark.gpu

TEX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textures")


@pytest.fixture(scope="module")
def reference():
    """{name: the oracle's decode} of every fixture and synthetic file, computed once."""
    return {name: oracle.jpeg_decode(data) for name, data, _ in jc.all_files()}


@pytest.fixture(scope="module")
def gpu(ctx):
    """{name: the GPU's decode (host entry)} of every fixture and synthetic file, decoded in
    the list's order: sizes, channel counts and IDCT scales alternate on one scratch buffer."""
    return {name: ctx.decode_jpeg(data) for name, data, _ in jc.all_files()}


@pytest.fixture(scope="module")
def big():
    with open(os.path.join(TEX, "Metal_Grill_002_basecolor.jpg"), "rb") as f:
        data = f.read()
    return data, oracle.jpeg_decode(data)


def _same(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (f"{what}: {len(bad)} of {ref.size} samples differ, first at {bad[:4].tolist()} "
                           f"gpu {got[tuple(bad[0])]} oracle {ref[tuple(bad[0])]}")


def test_gpu_equals_oracle_on_every_file(gpu, reference):
    assert len(gpu) == 252 + len(jc.synthetic_cases())
    for name, _, _ in jc.all_files():
        _same(gpu[name], reference[name], name)


def test_gpu_matches_recorded_hashes(gpu):
    hashed = [(name, h) for name, _, h in jc.all_files() if h is not None]
    assert len(hashed) >= 168
    bad = [name for name, h in hashed if jc.sha(gpu[name]) != h]
    assert not bad, f"{len(bad)} files differ from the Pillow-derived libjpeg 9 result: {bad[:8]}"


def test_gpu_within_bound_of_ideal_idct(gpu):
    """The bound B of tests/test_jpeg_decode.py (from the oracle's own worst error in this
    run, 0.5 + 2 * (0.5784 - 0.5) = 0.6568 < 1), held by the GPU's samples of every planes
    file, the 16x16 scaled IDCT and the clamping set included."""
    B, worst = jc.bound_from(lambda data: oracle.jpeg_decode(data))
    assert B < 1.0
    seen = set()
    for c in jc.synthetic_cases():
        if not c.planes:
            continue
        err, excluded, _, _, _ = jc.ideal_errors(c, gpu[c.name])
        print(f"{c.name}: worst |sample - ideal| {err:.4f} (B {B:.4f})")
        assert excluded == 0
        assert err <= B, f"{c.name}: worst |sample - ideal| {err:.4f} > {B:.4f}"
        seen.add((c.any_scaled, c.clamping))
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_decode_is_deterministic(ctx, gpu):
    for name, data, _ in jc.all_files():
        if name.endswith("_65x40") or name.endswith("_1x1"):
            assert np.array_equal(ctx.decode_jpeg(data), gpu[name]), name


def _files(*names):
    by_name = {n: d for n, d, _ in jc.all_files()}
    return [(n, by_name[n]) for n in names]


DEVICE_FILES = ("pil_420_prog_r3_q35opt_65x40", "pil_gray_base_r1_q100_33x31", "pil_444_base_r0_q100_1x1",
                "clamp_420_65x40", "cs_b_nomarkers_idsRGB_444", "rst1_444_ni_65x40", "gray_declared_2x2_33x31")
GUARD = 64


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_entry_writes_the_same_bytes(ctx, gpu, own_stream):
    """cg_image_decode_jpeg_device on the context's stream (None) and on a caller's
    non-default stream: width * height * channels bytes equal to the host entry's, and the
    guard bytes behind them untouched.  The decodes are enqueued back to back, each into
    its own buffer, and read after one synchronisation."""
    import torch
    stream = torch.cuda.Stream() if own_stream else None
    outs = []
    for name, data in _files(*DEVICE_FILES):
        n = gpu[name].size
        buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        outs.append((name, n, buf))
    torch.cuda.synchronize()
    for (name, n, buf), (_, data) in zip(outs, _files(*DEVICE_FILES)):
        rc = ctx.decode_jpeg_device(data, buf.data_ptr(), n, stream.cuda_stream if own_stream else None)
        assert rc == cgamd.CG_OK
    torch.cuda.synchronize()
    for name, n, buf in outs:
        host = buf.cpu().numpy()
        _same(host[:n].reshape(gpu[name].shape), gpu[name], f"{name} (device entry)")
        assert (host[n:] == 0xA5).all(), f"{name}: the device entry wrote past width * height * channels"


def test_capacity_one_byte_short(ctx, gpu):
    """cap = width * height * channels - 1: CG_E_CAPACITY from both entries, nothing written."""
    import torch
    lib = cgamd.load()
    for name, data in _files("pil_444_base_r0_q100_17x15", "pil_gray_prog_r0_q100_1x1", "clamp_420_33x31"):
        n = gpu[name].size
        jpg = np.frombuffer(data, np.uint8)
        out = np.full(n + GUARD, 0xA5, np.uint8)
        rc = lib.cg_image_decode_jpeg(ctx.h, jpg.ctypes.data, jpg.size, out.ctypes.data, n - 1)
        assert rc == cgamd.CG_E_CAPACITY, name
        assert (out == 0xA5).all(), f"{name}: the host entry wrote despite CG_E_CAPACITY"
        buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert ctx.decode_jpeg_device(data, buf.data_ptr(), n - 1) == cgamd.CG_E_CAPACITY, name
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xA5).all(), f"{name}: the device entry wrote despite CG_E_CAPACITY"
        # and the exact capacity is enough
        assert lib.cg_image_decode_jpeg(ctx.h, jpg.ctypes.data, jpg.size, out.ctypes.data, n) == cgamd.CG_OK
        _same(out[:n].reshape(gpu[name].shape), gpu[name], name)
        assert (out[n:] == 0xA5).all()


def test_scratch_buffer_reuse_across_sizes(ctx, reference, big):
    """Large (a 1024x1024 texture), 1x1, 33x31 4:2:0, large again, then a gray file between
    two colour files: each equals its own reference -- no stale planes or coefficients from
    the grow-only scratch buffer."""
    big_data, big_ref = big
    small = dict(_files("pil_444_prog_r0_q35opt_1x1", "pil_420_base_r3_q100_33x31", "pil_444_base_r1_q100_65x40",
                        "pil_gray_prog_r1_q35opt_33x31", "perscan_420_r3_65x40", "pil_gray_base_r0_q100_1x1"))
    order = [("large", big_data, big_ref)]
    for n in ("pil_444_prog_r0_q35opt_1x1", "pil_420_base_r3_q100_33x31"):
        order.append((n, small[n], reference[n]))
    order.append(("large again", big_data, big_ref))
    for n in ("pil_444_base_r1_q100_65x40", "pil_gray_prog_r1_q35opt_33x31", "perscan_420_r3_65x40",
              "pil_gray_base_r0_q100_1x1"):
        order.append((n, small[n], reference[n]))
    for name, data, ref in order:
        _same(ctx.decode_jpeg(data), ref, f"{name} (scratch reuse)")
