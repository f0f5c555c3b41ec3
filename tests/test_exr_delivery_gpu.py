"""GPU: key scripts of float pictures delivered as EXR files (cg_rt_render_sequence_exr,
cg_rast_draw_sequence_exr).  Every delivered file goes through the independent reader
(tests/exr_enc_ref.py part b: struct, zlib, numpy): FLOAT files must hold the floats of
cg_rt_render_sequence_device / cg_rast_draw_sequence_picture_device bit for bit, HALF files their
numpy halves; the rasteriser's records must equal cg_rast_draw_sequence's."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import exr_enc_ref as ref
import rt_seq_states as S
from test_rast_sequence_gpu import _params

pytestmark = pytest.mark.gpu

W, H = 160, 120
# the reference scene, five frames: the start, a yaw, a light move, two yaws back past 0, the light again
RT_SCRIPT = ["", "m", "d", "nn", "w"]
RT_ALPHA = 1.0 / 9.0
COMBOS = [(ref.RGBA, ref.FLOAT, ref.ZIP), (ref.RGBA, ref.HALF, ref.ZIP), (ref.RGB, ref.HALF, ref.NONE), (ref.RGB, ref.FLOAT, ref.NONE)]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def rt(ctx):
    torch, dev = _torch()
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)
    states = S.key_states(RT_SCRIPT, 96.0)
    cams = [S.camera(st, W, H) for st in states]
    lights = [S.light_array(st.lights()) for st in states]
    stride = W * cgamd.load().cg_rt_shard_rows(H, None)
    buf = torch.zeros(len(cams) * stride * 4, dtype=torch.float32, device=dev)
    ctx.rt_render_sequence_device(cams, lights, buf.data_ptr(), frame_stride=stride, pix_format=cgamd.PIX_RGBA_F32)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().reshape(len(cams), stride, 4)[:, :W * H].reshape(len(cams), H, W, 4).copy()
    raw.setflags(write=False)
    assert len({f.tobytes() for f in raw}) == len(cams)           # every key changed the picture
    return ctx, cams, lights, raw


@pytest.fixture(scope="module")
def rast(ctx):
    """tests/test_rast_sequence_gpu.py's script: colour modes 1 1 2 0 2 1 1 2, so the rand() chain runs."""
    torch, dev = _torch()
    ctx.rast_set_scene()
    ps = _params(W, H, 90.0, 0)
    assert {p.colour_mode for p in ps} >= {0, 1}
    _, _, _, info, _ = ctx.rast_draw_sequence(ps, chunk=3)
    buf = torch.zeros(len(ps) * W * H * 4, dtype=torch.float32, device=dev)
    d_info = torch.zeros((len(ps) + 1) * 6, dtype=torch.int32, device=dev)
    ctx.rast_set_scene()
    ctx.rast_draw_sequence_picture_device(ps, buf.data_ptr(), d_info=d_info.data_ptr())
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().reshape(len(ps), H, W, 4).copy()
    raw.setflags(write=False)
    return ctx, ps, raw, info


def _holds(files, raw, prm, alpha):
    assert len(files) == len(raw)
    for f, data in enumerate(files):
        got = ref.read(data)
        assert (got["width"], got["height"], got["type"], got["compression"]) == (W, H, prm[1], prm[2]), f"frame {f}"
        want = ref.expected_planes(raw[f], prm[0], prm[1], alpha)
        assert sorted(got["planes"]) == sorted(want)
        for k, v in want.items():
            assert np.array_equal(got["planes"][k], v), f"frame {f} channel {k}"


@pytest.mark.parametrize("prm", COMBOS, ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def test_raytracer_files_hold_the_pictures(rt, prm):
    ctx, cams, lights, raw = rt
    files = ctx.rt_render_sequence_exr(cams, lights, *prm, RT_ALPHA, chunk=2)      # two chunk boundaries and an odd tail
    _holds(files, raw, prm, RT_ALPHA)
    assert files == [cgamd.image_encode_exr_host(f, *prm, RT_ALPHA) for f in raw]


@pytest.mark.parametrize("chunk", [1, 3, 0, 64])
def test_raytracer_chunk_sizes(rt, chunk):
    """64 is clamped to the 8 frames of the float scratch."""
    ctx, cams, lights, raw = rt
    assert ctx.rt_render_sequence_exr(cams, lights, chunk=chunk) == [cgamd.image_encode_exr_host(f) for f in raw]


def test_nine_frames_cross_a_chunk(rt):
    ctx, cams, lights, raw = rt
    order = [0, 1, 2, 3, 4, 3, 2, 1, 0]
    files = ctx.rt_render_sequence_exr([cams[k] for k in order], [lights[k] for k in order])
    assert files == [cgamd.image_encode_exr_host(raw[k]) for k in order]


@pytest.mark.parametrize("prm", COMBOS, ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def test_rasteriser_files_hold_the_pictures(rast, prm):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    files, info_e = ctx.rast_draw_sequence_exr(ps, *prm, chunk=3)
    assert np.array_equal(info_e, info)
    _holds(files, raw, prm, 1.0)
    assert files == [cgamd.image_encode_exr_host(f, *prm) for f in raw]


@pytest.mark.parametrize("chunk", [1, 0, 8])
def test_rasteriser_chunk_sizes(rast, chunk):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    files, info_e = ctx.rast_draw_sequence_exr(ps, chunk=chunk)
    assert np.array_equal(info_e, info)
    assert files == [cgamd.image_encode_exr_host(f) for f in raw]


def test_rasteriser_nine_frames_cross_a_chunk(rast):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    ps9 = list(ps) + [ps[3]]                                       # a ninth frame in mode 0: it draws no random numbers
    assert len(ps9) == 9 and ps[3].colour_mode == 0
    files, info_e = ctx.rast_draw_sequence_exr(ps9)
    assert np.array_equal(info_e[:len(ps)], info[:len(ps)])
    assert info_e[len(ps9)]["rand_offset"] == info[len(ps)]["rand_offset"]
    assert files[:len(ps)] == [cgamd.image_encode_exr_host(f) for f in raw]
    assert files[8] == cgamd.image_encode_exr_host(raw[3])


def test_capacity_holds_three_of_five(rt):
    ctx, cams, lights, raw = rt
    want = [cgamd.image_encode_exr_host(f) for f in raw]
    need = sum(len(x) for x in want)
    cap = sum(len(x) for x in want[:3]) + len(want[3]) - 1          # frame 3 is one byte short
    buf = np.full(need + 64, 0xA5, np.uint8)
    rc, files, offsets, _ = ctx.rt_render_sequence_exr(cams, lights, chunk=2, out=buf, cap=cap, full=True)
    assert rc == cgamd.CG_E_CAPACITY and int(offsets[5]) == need
    assert files == want[:3]
    assert (buf[cap:] == 0xA5).all()
    rc, files, offsets, _ = ctx.rt_render_sequence_exr(cams, lights, chunk=2, out=buf, cap=int(offsets[5]), full=True)
    assert rc == cgamd.CG_OK and files == want and (buf[need:] == 0xA5).all()
    assert [int(o) for o in offsets] == [sum(len(x) for x in want[:k]) for k in range(6)]


def test_rasteriser_capacity(rast):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    want = [cgamd.image_encode_exr_host(f) for f in raw]
    need = sum(len(x) for x in want)
    cap = sum(len(x) for x in want[:4]) + 5
    buf = np.full(need + 64, 0xA5, np.uint8)
    rc, files, offsets, info_e, _ = ctx.rast_draw_sequence_exr(ps, chunk=3, out=buf, cap=cap, full=True)
    assert rc == cgamd.CG_E_CAPACITY and int(offsets[len(ps)]) == need and files == want[:4]
    assert (buf[cap:] == 0xA5).all() and np.array_equal(info_e, info)
    rc, files, offsets, info_e, _ = ctx.rast_draw_sequence_exr(ps, chunk=3, out=buf, cap=need, full=True)
    assert rc == cgamd.CG_OK and files == want and np.array_equal(info_e, info)


def test_argument_errors(rt):
    ctx, cams, lights, raw = rt
    lib = ctx.lib
    larr, n = cgamd.sequence_lights(lights)
    arr = (cgamd.RtCamera * len(cams))(*cams)
    buf = np.zeros(1 << 20, np.uint8)
    offs = np.zeros(len(cams) + 1, np.uint64)
    op = C.cast(offs.ctypes.data, C.POINTER(C.c_size_t))
    call = lambda prm, out, offsets, chunk=0, nf=len(cams): lib.cg_rt_render_sequence_exr(   # noqa: E731
        ctx.h, larr, n, arr, nf, prm, out, buf.size, offsets, chunk, None)
    ok = cgamd.ExrParams(ref.RGBA, ref.HALF, ref.ZIP, 1.0)
    out = cgamd.P(buf.ctypes.data)
    for bad in (cgamd.ExrParams(2, 1, 3, 1.0), cgamd.ExrParams(4, 0, 3, 1.0), cgamd.ExrParams(4, 1, 2, 1.0),
                cgamd.ExrParams(4, 1, 3, float("inf"))):
        assert call(C.byref(bad), out, op) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), None, op) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, None) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, chunk=-1) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, nf=0) == cgamd.CG_OK and not buf.any()
    assert call(None, out, op, nf=1) == cgamd.CG_OK                      # NULL: RGBA, HALF, ZIP, alpha scale 1
    assert bytes(buf[:int(offs[1])]) == cgamd.image_encode_exr_host(raw[0])
    rcall = lambda prm, out, offsets, chunk=0: lib.cg_rast_draw_sequence_exr(   # noqa: E731
        ctx.h, (cgamd.RastParams * 1)(cgamd.rast_params(W, H, 90.0)), 1, prm, out, buf.size, offsets, chunk, None, None)
    ctx.rast_set_scene()
    assert rcall(C.byref(ok), out, None) == cgamd.CG_E_INVALID
    assert rcall(C.byref(cgamd.ExrParams(5, 1, 3, 1.0)), out, op) == cgamd.CG_E_INVALID
    assert rcall(C.byref(ok), out, op, chunk=9) == cgamd.CG_E_INVALID
    with cgamd.Context(0) as fresh:
        assert lib.cg_rast_draw_sequence_exr(fresh.h, (cgamd.RastParams * 1)(cgamd.rast_params(W, H, 90.0)), 1,
                                             C.byref(ok), out, buf.size, op, 0, None, None) == cgamd.CG_E_NOSCENE
