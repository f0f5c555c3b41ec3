"""GPU: frame sequences delivered compressed (cg_rt_render_sequence_jpeg,
cg_rast_draw_sequence_jpeg).  Every delivered file must equal the host encoder
(cg_image_encode_jpeg_host, which tests/test_jpeg_encode.py holds to Pillow's bytes) on the frame the
uncompressed call delivers; the rasteriser's records must equal cg_rast_draw_sequence's."""
import numpy as np
import pytest

import cgamd
import rt_seq_states as S
from test_rast_sequence_gpu import _params

pytestmark = pytest.mark.gpu

W, H = 160, 120
# the reference scene, five frames: the start, a yaw, a light move, two yaws back past 0, the light again
RT_SCRIPT = ["", "m", "d", "nn", "w"]


@pytest.fixture(scope="module")
def rt(ctx):
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    states = S.key_states(RT_SCRIPT, 96.0)
    cams = [S.camera(st, W, H) for st in states]
    lights = [S.light_array(st.lights()) for st in states]
    raw, _ = ctx.rt_render_sequence(cams, lights, chunk=2)
    raw = raw.reshape(len(cams), H, W).copy()
    raw.setflags(write=False)
    assert len({f.tobytes() for f in raw}) == len(cams)           # every key changed the frame
    return ctx, cams, lights, raw


def _want(raw, q, sub):
    return [cgamd.image_encode_jpeg_host(f, q, sub) for f in raw]


@pytest.mark.parametrize("sub", [cgamd.JPEG_420, cgamd.JPEG_444])
def test_raytracer_sequence(rt, sub):
    """chunk = 2 over five frames: two chunk boundaries and an odd tail."""
    ctx, cams, lights, raw = rt
    files = ctx.rt_render_sequence_jpeg(cams, lights, 75, sub, chunk=2)
    want = _want(raw, 75, sub)
    assert len(files) == 5
    for f in range(5):
        assert files[f] == want[f], f"frame {f}"
    assert files == ctx.rt_render_sequence_jpeg(cams, lights, 75, sub, chunk=0)     # one chunk


def test_raytracer_files_longer_than_their_slot(rt):
    """Q = 100 at 4:4:4 on a small frame: whether a file is longer than its W * H byte device slot or
    not, it is delivered whole (a longer one is encoded again alone)."""
    ctx, cams, lights, raw = rt
    want = _want(raw, 100, cgamd.JPEG_444)
    print("file lengths", [len(x) for x in want], "slot", W * H)
    assert ctx.rt_render_sequence_jpeg(cams, lights, 100, cgamd.JPEG_444, chunk=2) == want


def test_capacity_holds_three_of_five(rt):
    ctx, cams, lights, raw = rt
    want = _want(raw, 90, cgamd.JPEG_420)
    need = sum(len(x) for x in want)
    cap = sum(len(x) for x in want[:3]) + len(want[3]) - 1          # frame 3 is one byte short
    buf = np.full(need + 64, 0xA5, np.uint8)
    rc, files, offsets, _ = ctx.rt_render_sequence_jpeg(cams, lights, 90, cgamd.JPEG_420, chunk=2, out=buf, cap=cap,
                                                        full=True)
    assert rc == cgamd.CG_E_CAPACITY and int(offsets[5]) == need
    assert files == want[:3]
    assert (buf[cap:] == 0xA5).all()
    rc, files, offsets, _ = ctx.rt_render_sequence_jpeg(cams, lights, 90, cgamd.JPEG_420, chunk=2, out=buf,
                                                        cap=int(offsets[5]), full=True)
    assert rc == cgamd.CG_OK and files == want and (buf[need:] == 0xA5).all()
    assert [int(o) for o in offsets] == [sum(len(x) for x in want[:k]) for k in range(6)]


def test_pinned_destination(rt):
    import torch
    ctx, cams, lights, raw = rt
    want = _want(raw, 75, cgamd.JPEG_420)
    pinned = torch.zeros(sum(len(x) for x in want), dtype=torch.uint8).pin_memory()
    assert ctx.rt_render_sequence_jpeg(cams, lights, 75, cgamd.JPEG_420, chunk=2, out=pinned) == want


def test_rasteriser_sequence_with_colour_modes(ctx):
    """tests/test_rast_sequence_gpu.py's script: modes 1 1 2 0 2 1 1 2, chunk 3."""
    ctx.rast_set_scene()
    ps = _params(W, H, 90.0, 0)
    raw, _, _, info, _ = ctx.rast_draw_sequence(ps, chunk=3)
    raw = raw.reshape(len(ps), H, W)
    for sub in (cgamd.JPEG_420, cgamd.JPEG_444):
        files, info_j = ctx.rast_draw_sequence_jpeg(ps, 75, sub, chunk=3)
        assert np.array_equal(info_j, info)
        assert files == _want(raw, 75, sub)


def test_rasteriser_files_longer_than_their_slot(ctx):
    """The random colours of modes 1-2 at Q = 100, 4:4:4: the first frame's file fits its W * H byte
    device slot, the others do not and are encoded again alone, in place among the others."""
    ctx.rast_set_scene()
    ps = _params(W, H, 90.0, 0)
    raw, _, _, info, _ = ctx.rast_draw_sequence(ps, chunk=3)
    want = _want(raw.reshape(len(ps), H, W), 100, cgamd.JPEG_444)
    lens = [len(x) for x in want]
    print("file lengths", lens, "slot", W * H)
    assert min(lens) < W * H < max(lens)
    files, info_j = ctx.rast_draw_sequence_jpeg(ps, 100, cgamd.JPEG_444, chunk=3)
    assert np.array_equal(info_j, info) and files == want


def test_rasteriser_flagged_frames_are_repaired(ctx):
    """A rand() stream of 20000 fragments flags frames 4-7 (tests/test_rast_draw_sequence_gpu.py); their
    files are those of the repaired frames, in place among the others."""
    ctx.rast_set_scene()
    ps = _params(W, H, 90.0, 0)
    raw, _, _, info, _ = ctx.rast_draw_sequence(ps, chunk=3)
    want = _want(raw.reshape(len(ps), H, W), 75, cgamd.JPEG_420)
    try:
        ctx.rast_set_rand_capacity(20000)
        files, info_j = ctx.rast_draw_sequence_jpeg(ps, 75, cgamd.JPEG_420, chunk=3)
    finally:
        ctx.rast_set_rand_capacity(0)
    assert np.array_equal(info_j, info) and files == want


def test_rasteriser_compact_route(ctx):
    f32 = lambda x: float(np.float32(x))   # noqa: E731
    ps = [cgamd.rast_params(157, 93, 70.0, cam=(0.0, 0.0, f32(-3.001 + 0.3 * k), 1.0),
                            indirect_first=f32(0.15 if k == 0 else 0.2)) for k in range(3)]
    ctx.rast_set_scene()
    try:
        ctx.rast_set_route_limit(1)
        raw, _, _, info, _ = ctx.rast_draw_sequence(ps, chunk=2)
        assert ctx.rast_scratch_info()["route"] == cgamd.RAST_ROUTE_COMPACT
        files, info_j = ctx.rast_draw_sequence_jpeg(ps, 90, cgamd.JPEG_420, chunk=2)
        assert ctx.rast_scratch_info()["route"] == cgamd.RAST_ROUTE_COMPACT
    finally:
        ctx.rast_set_route_limit(0)
    assert np.array_equal(info_j, info)
    assert files == _want(raw.reshape(3, 93, 157), 90, cgamd.JPEG_420)


def test_exposed_bloom_chunk_through_the_device_encoder(rt):
    """The exposed and bloom chains end in ARGB on the device, which the encoder takes as it is."""
    import torch
    ctx, cams, lights, _ = rt
    n, px = len(cams), W * H
    dev = torch.device("cuda", 0)
    d_argb = torch.zeros(n * px, dtype=torch.int32, device=dev)
    d_scales = torch.zeros(n, dtype=torch.float32, device=dev)
    slot = cgamd.image_jpeg_bound(W, H, cgamd.JPEG_420)
    d_out = torch.full((n * slot,), 0xA5, dtype=torch.uint8, device=dev)
    d_bytes = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.rt_render_exposed_bloom_device(cams, d_argb.data_ptr(), d_scales.data_ptr(), cgamd.hdr_params(),
                                       cgamd.hdr_bloom_params(threshold=0.5, intensity=0.5), lights=lights,
                                       per_frame_lights=True)
    ctx.image_encode_jpeg_device(d_argb.data_ptr(), W, H, n, d_out.data_ptr(), slot, d_bytes.data_ptr(), 75, cgamd.JPEG_420)
    torch.cuda.synchronize()
    argb = d_argb.cpu().numpy().view(np.uint32).reshape(n, H, W)
    out, lens = d_out.cpu().numpy(), d_bytes.cpu().numpy()
    assert len({f.tobytes() for f in argb}) == n
    for f in range(n):
        assert out[f * slot:f * slot + lens[f]].tobytes() == cgamd.image_encode_jpeg_host(argb[f], 75, cgamd.JPEG_420)


def test_argument_errors(rt):
    ctx, cams, lights, _ = rt
    lib = ctx.lib
    larr, n = cgamd.sequence_lights(lights)
    arr = (cgamd.RtCamera * len(cams))(*cams)
    buf = np.zeros(1 << 16, np.uint8)
    offs = np.zeros(len(cams) + 1, np.uint64)
    import ctypes as C
    op = C.cast(offs.ctypes.data, C.POINTER(C.c_size_t))
    call = lambda prm, out, offsets, chunk=0, nf=len(cams): lib.cg_rt_render_sequence_jpeg(   # noqa: E731
        ctx.h, larr, n, arr, nf, prm, out, buf.size, offsets, chunk, None)
    ok = cgamd.JpegParams(75, 2)
    out = cgamd.P(buf.ctypes.data)
    for bad in (cgamd.JpegParams(0, 2), cgamd.JpegParams(101, 2), cgamd.JpegParams(75, 1)):
        assert call(C.byref(bad), out, op) == cgamd.CG_E_INVALID
    assert call(None, out, op) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), None, op) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, None) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, chunk=-1) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, nf=-1) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, nf=0) == cgamd.CG_OK and not buf.any()
    rcall = lambda prm, out, offsets: lib.cg_rast_draw_sequence_jpeg(   # noqa: E731
        ctx.h, (cgamd.RastParams * 1)(cgamd.rast_params(W, H, 90.0)), 1, prm, out, buf.size, offsets, 0, None, None)
    ctx.rast_set_scene()
    assert rcall(None, out, op) == cgamd.CG_E_INVALID
    assert rcall(C.byref(ok), out, None) == cgamd.CG_E_INVALID
    assert rcall(C.byref(cgamd.JpegParams(75, 3)), out, op) == cgamd.CG_E_INVALID
    with cgamd.Context(0) as fresh:
        assert lib.cg_rast_draw_sequence_jpeg(fresh.h, (cgamd.RastParams * 1)(cgamd.rast_params(W, H, 90.0)), 1,
                                              C.byref(ok), out, buf.size, op, 0, None, None) == cgamd.CG_E_NOSCENE
