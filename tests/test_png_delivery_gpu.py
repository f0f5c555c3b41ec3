"""GPU: frame sequences delivered exact (cg_rt_render_sequence_png, cg_rast_draw_sequence_png).
Every delivered file must decode -- by the test's own chunk walk, zlib and numpy un-filtering
(tests/png_enc_ref.py's decode, which shares nothing with the library) -- to exactly the frame the
uncompressed call delivers; the rasteriser's records must equal cg_rast_draw_sequence's."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import png_enc_ref as ref
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


@pytest.fixture(scope="module")
def rast(ctx):
    """tests/test_rast_sequence_gpu.py's script: colour modes 1 1 2 0 2 1 1 2, so the rand() chain runs."""
    ctx.rast_set_scene()
    ps = _params(W, H, 90.0, 0)
    assert {p.colour_mode for p in ps} >= {0, 1}
    raw, _, _, info, _ = ctx.rast_draw_sequence(ps, chunk=3)
    raw = raw.reshape(len(ps), H, W).copy()
    raw.setflags(write=False)
    return ctx, ps, raw, info


def _decodes_to(files, raw, colour):
    assert len(files) == len(raw)
    for f, data in enumerate(files):
        want = raw[f] if colour == cgamd.PNG_RGBA else raw[f] | np.uint32(0xFF000000)
        assert np.array_equal(ref.decode(data), want), f"frame {f}"


@pytest.mark.parametrize("colour", [cgamd.PNG_RGB, cgamd.PNG_RGBA])
def test_raytracer_files_decode_to_the_frames(rt, colour):
    ctx, cams, lights, raw = rt
    files = ctx.rt_render_sequence_png(cams, lights, colour, chunk=2)      # two chunk boundaries and an odd tail
    _decodes_to(files, raw, colour)
    assert files == [cgamd.image_encode_png_host(f, colour) for f in raw]


@pytest.mark.parametrize("chunk", [1, 3, 0])
def test_raytracer_chunk_sizes(rt, chunk):
    ctx, cams, lights, raw = rt
    assert ctx.rt_render_sequence_png(cams, lights, chunk=chunk) == [cgamd.image_encode_png_host(f) for f in raw]


@pytest.mark.parametrize("colour", [cgamd.PNG_RGB, cgamd.PNG_RGBA])
def test_rasteriser_files_decode_to_the_frames(rast, colour):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    files, info_p = ctx.rast_draw_sequence_png(ps, colour, chunk=3)
    assert np.array_equal(info_p, info)
    _decodes_to(files, raw, colour)
    assert files == [cgamd.image_encode_png_host(f, colour) for f in raw]


@pytest.mark.parametrize("chunk", [1, 3, 0])
def test_rasteriser_chunk_sizes_and_a_fixed_filter(rast, chunk):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    files, info_p = ctx.rast_draw_sequence_png(ps, cgamd.PNG_RGB, 4, chunk=chunk)
    assert np.array_equal(info_p, info)
    assert files == [cgamd.image_encode_png_host(f, cgamd.PNG_RGB, 4) for f in raw]


def test_capacity_holds_three_of_five(rt):
    ctx, cams, lights, raw = rt
    want = [cgamd.image_encode_png_host(f) for f in raw]
    need = sum(len(x) for x in want)
    cap = sum(len(x) for x in want[:3]) + len(want[3]) - 1          # frame 3 is one byte short
    buf = np.full(need + 64, 0xA5, np.uint8)
    rc, files, offsets, _ = ctx.rt_render_sequence_png(cams, lights, chunk=2, out=buf, cap=cap, full=True)
    assert rc == cgamd.CG_E_CAPACITY and int(offsets[5]) == need
    assert files == want[:3]
    assert (buf[cap:] == 0xA5).all()
    rc, files, offsets, _ = ctx.rt_render_sequence_png(cams, lights, chunk=2, out=buf, cap=int(offsets[5]), full=True)
    assert rc == cgamd.CG_OK and files == want and (buf[need:] == 0xA5).all()
    assert [int(o) for o in offsets] == [sum(len(x) for x in want[:k]) for k in range(6)]


def test_rasteriser_capacity(rast):
    ctx, ps, raw, info = rast
    ctx.rast_set_scene()
    want = [cgamd.image_encode_png_host(f) for f in raw]
    need = sum(len(x) for x in want)
    cap = sum(len(x) for x in want[:4]) + 5
    buf = np.full(need + 64, 0xA5, np.uint8)
    rc, files, offsets, info_p, _ = ctx.rast_draw_sequence_png(ps, chunk=3, out=buf, cap=cap, full=True)
    assert rc == cgamd.CG_E_CAPACITY and int(offsets[len(ps)]) == need and files == want[:4]
    assert (buf[cap:] == 0xA5).all() and np.array_equal(info_p, info)
    rc, files, offsets, info_p, _ = ctx.rast_draw_sequence_png(ps, chunk=3, out=buf, cap=need, full=True)
    assert rc == cgamd.CG_OK and files == want and np.array_equal(info_p, info)


def test_argument_errors(rt):
    ctx, cams, lights, _ = rt
    lib = ctx.lib
    larr, n = cgamd.sequence_lights(lights)
    arr = (cgamd.RtCamera * len(cams))(*cams)
    buf = np.zeros(1 << 16, np.uint8)
    offs = np.zeros(len(cams) + 1, np.uint64)
    op = C.cast(offs.ctypes.data, C.POINTER(C.c_size_t))
    call = lambda prm, out, offsets, chunk=0, nf=len(cams): lib.cg_rt_render_sequence_png(   # noqa: E731
        ctx.h, larr, n, arr, nf, prm, out, buf.size, offsets, chunk, None)
    ok = cgamd.PngParams(cgamd.PNG_RGB, cgamd.PNG_FILTER_ADAPTIVE)
    out = cgamd.P(buf.ctypes.data)
    for bad in (cgamd.PngParams(0, -1), cgamd.PngParams(3, -1), cgamd.PngParams(2, 5), cgamd.PngParams(6, -2)):
        assert call(C.byref(bad), out, op) == cgamd.CG_E_INVALID
    assert call(None, out, op) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), None, op) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, None) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, chunk=-1) == cgamd.CG_E_INVALID
    assert call(C.byref(ok), out, op, nf=0) == cgamd.CG_OK and not buf.any()
    rcall = lambda prm, out, offsets: lib.cg_rast_draw_sequence_png(   # noqa: E731
        ctx.h, (cgamd.RastParams * 1)(cgamd.rast_params(W, H, 90.0)), 1, prm, out, buf.size, offsets, 0, None, None)
    ctx.rast_set_scene()
    assert rcall(None, out, op) == cgamd.CG_E_INVALID
    assert rcall(C.byref(ok), out, None) == cgamd.CG_E_INVALID
    assert rcall(C.byref(cgamd.PngParams(4, -1)), out, op) == cgamd.CG_E_INVALID
    with cgamd.Context(0) as fresh:
        assert lib.cg_rast_draw_sequence_png(fresh.h, (cgamd.RastParams * 1)(cgamd.rast_params(W, H, 90.0)), 1,
                                             C.byref(ok), out, buf.size, op, 0, None, None) == cgamd.CG_E_NOSCENE
