"""GPU: the one-light lattice kernel's single pass per point (cg_rt.hip lattice_body).  A step of
a wave finds the closest hits of its chunks of 64 lattice points and shades them from the
registers that hold t, the table slot and the ray's X, Y; each live point is stored to LDS once,
as (DirectLight, slot).  The float operations are those of the two passes it replaces, so every
frame must equal the CPU oracle's, every pixel (integer ARGB: tolerance 0).  The shapes are the
smallest at which the step bookkeeping can go wrong: tiles cut by the right and bottom edge
(lanes of a chunk not live; a step's later chunks past the tile's points), a tile so small that
two of the four waves have no point, the same under a yaw (pitch 48, two points per lane,
several steps per wave), LoadTestModel with its sphere (several candidates per tile, per-object
shadow masks with and without CG_OBJ_MASKS, covered wall tiles), the blocks alone (misses
beside hits and shadowed hits beside lit ones inside a chunk), a frame sequence whose light
moves and a batched dolly.
Reference: raytracer/Source/skeleton.cpp:104-169, :366-415."""
import ctypes as C
import os

import numpy as np
import pytest

import cgamd
import oracle

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 4)
YAW = 0.1745
LIGHT_POS = (0.0, -0.5, -0.7, 1.0)
WHITE = (14.0, 14.0, 14.0)
BLACK_PIXEL = 0x80000000   # PutPixelSDL(0, 0, 0): none of the pixel's sub-rays hit

# name: (W, H, focal, cameraPos, yaw or None)
CAMERAS = {
    # right tile 8 pixels wide (cols = 17), bottom tile 7 rows tall (rows = 15, 495 points)
    "cut_40x37": (40, 37, 37.0, (0.0, 0.0, -3.0, 1.0), None),
    "cut_40x37_yaw": (40, 37, 37.0, (0.0, 0.0, -3.0, 1.0), YAW),
    # three lattice rows, 99 points: waves 2 and 3 have none
    "idle_16x1": (16, 1, 14.0, (0.0, 0.0, -3.0, 1.0), None),
    "idle_16x1_yaw": (16, 1, 14.0, (0.0, 0.0, -3.0, 1.0), YAW),
    "64x60": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None),
    "64x60_dolly": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.005)), 1.0), None),
    "64x60_dolly2": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.010)), 1.0), None),
    "48x45": (48, 45, 90.0, (0.1, 0.3, -3.0, 1.0), None),
}
# the light of each frame of the sequence
MOVING = (LIGHT_POS, (0.3, -0.5, -0.7, 1.0), (-0.3, -0.4, -0.9, 1.0))

_REF = {}


def _blocks():
    """Triangles 10..27 of LoadTestModel: the two blocks, no sphere."""
    tris, _, _ = cgamd.rt_scene()
    out = (cgamd.Tri * 18)()
    for k, i in enumerate(range(10, 28)):
        C.memmove(C.byref(out[k]), C.byref(tris[i]), C.sizeof(cgamd.Tri))
    return out, len(out), None


SCENES = {
    "test_model": lambda: cgamd.rt_scene(),   # with its sphere
    "blocks": _blocks,
}


def _lights(pos=LIGHT_POS, colour=WHITE):
    arr = cgamd.default_lights()
    arr[0].position = cgamd.Vec4(*pos)
    arr[0].colour = cgamd.Vec3(*colour)
    return arr


def _reference(scene, cam, pos=LIGHT_POS, colour=WHITE):
    """The CPU oracle's frame, computed once per (scene, camera, light) and never modified."""
    key = (scene, cam, pos, colour)
    if key not in _REF:
        W, H, f, cpos, yaw = CAMERAS[cam]
        tris, n, sph = SCENES[scene]()
        R = list(cgamd.yaw_matrix(yaw)) if yaw is not None else None
        otris = (oracle.RtTri * len(tris)).from_buffer_copy(tris)
        osph = C.pointer(oracle.Sphere.from_buffer_copy(sph)) if sph is not None else None
        p = oracle.rt_params(W, H, f, cpos, R, lights=[(pos, colour)])
        _REF[key] = oracle.rt_draw(p, threads=THREADS, scene=(otris, n, osph, 1 if sph is not None else 0))
        _REF[key].setflags(write=False)
    return _REF[key]


def _hit_and_missed(ref, what):
    """The case is not vacuous: the oracle's frame has pixels that hit and pixels that missed."""
    missed = int((ref == BLACK_PIXEL).sum())
    assert 0 < missed < ref.size, f"{what}: {missed} of {ref.size} pixels missed"


def _shadowed_and_lit(scene, cam):
    """The oracle's frame has pixels in shadow -- hit pixels whose value is the one a black light
    gives, every sub-ray's DirectLight zero -- beside lit ones."""
    ref, unlit = _reference(scene, cam), _reference(scene, cam, colour=(0.0, 0.0, 0.0))
    shadowed = int(((ref == unlit) & (ref != BLACK_PIXEL)).sum())
    lit = int((ref != unlit).sum())
    assert shadowed > 0 and lit > 0, f"{scene}/{cam}: {shadowed} pixels in shadow, {lit} lit"


def _camera(cam):
    W, H, f, pos, yaw = CAMERAS[cam]
    return cgamd.rt_camera(W, H, f, pos, cgamd.yaw_matrix(yaw) if yaw is not None else None)


@pytest.fixture
def scene_of(ctx):
    """Sets a scene; LoadTestModel is back afterwards (the session's context is shared)."""
    def set_scene(scene):
        tris, n, sph = SCENES[scene]()
        ctx.rt_set_scene(tris, n, sph, 1)
        return ctx
    yield set_scene
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)


def _assert_frame(ctx, scene, cam):
    tris, n, sph = SCENES[scene]()
    route = "lattice_yaw" if CAMERAS[cam][4] is not None else "lattice"
    assert cgamd.rt_route(_camera(cam), n, 1 if sph is not None else 0, 1) == route
    ref = _reference(scene, cam)
    _hit_and_missed(ref, f"{scene}/{cam}")
    argb, _ = ctx.rt_render(_camera(cam), lights=_lights())
    bad = np.flatnonzero(argb != ref)
    assert bad.size == 0, f"{scene}/{cam}: {bad.size} pixels differ, first {bad[:8]}"


@pytest.mark.parametrize("cam", ["cut_40x37", "idle_16x1", "cut_40x37_yaw", "idle_16x1_yaw"])
def test_fused_cut_tiles_and_idle_waves(scene_of, cam):
    """Tiles cut by the right and the bottom edge, and a tile of 99 points, with shared and with
    per-pixel columns."""
    _assert_frame(scene_of("test_model"), "test_model", cam)


@pytest.mark.parametrize("knob", ["on", "off"])
def test_fused_full_model(scene_of, monkeypatch, knob):
    """LoadTestModel with its sphere, the shadow masks per object and (CG_OBJ_MASKS=0) per tile.
    Pixels in shadow are present: hit pixels whose value is the one a black light gives."""
    if knob == "off":
        monkeypatch.setenv("CG_OBJ_MASKS", "0")
    else:
        monkeypatch.delenv("CG_OBJ_MASKS", raising=False)
    _shadowed_and_lit("test_model", "64x60")
    _assert_frame(scene_of("test_model"), "test_model", "64x60")


def test_fused_mixed_misses_and_shadows(scene_of):
    """The blocks alone: chunks hold misses beside hits, and shadowed hits beside lit ones."""
    _shadowed_and_lit("blocks", "48x45")
    _assert_frame(scene_of("blocks"), "blocks", "48x45")


def _device_frames(call, nframes, cam):
    import torch
    W, H = CAMERAS[cam][:2]
    stride = W * ((H + 7) // 8 * 8)   # device frames hold whole 8-row stripes
    out = torch.zeros(nframes * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    call(out.data_ptr(), s.cuda_stream, stride)
    s.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(nframes, stride)[:, :W * H]


def test_fused_sequence_light_moves(scene_of):
    """One cg_rt_render_sequence_device call of three frames, the light at another place in each."""
    ctx = scene_of("test_model")
    cams = [_camera("64x60")] * len(MOVING)
    frames = _device_frames(
        lambda ptr, stream, stride: ctx.rt_render_sequence_device(cams, [_lights(p) for p in MOVING], ptr, None,
                                                                  stream, frame_stride=stride),
        len(MOVING), "64x60")
    for k, pos in enumerate(MOVING):
        ref = _reference("test_model", "64x60", pos=pos)
        _hit_and_missed(ref, f"frame {k}")
        bad = np.flatnonzero(frames[k] != ref)
        assert bad.size == 0, f"frame {k} (light at {pos}): {bad.size} pixels differ, first {bad[:8]}"


def test_fused_batched_dolly(scene_of):
    """Three frames of a dolly in one cg_rt_render_frames_device call."""
    ctx = scene_of("test_model")
    names = ["64x60", "64x60_dolly", "64x60_dolly2"]
    frames = _device_frames(
        lambda ptr, stream, stride: ctx.rt_render_frames_device([_camera(c) for c in names], ptr, None, stream,
                                                                frame_stride=stride),
        len(names), "64x60")
    for k, c in enumerate(names):
        ref = _reference("test_model", c)
        _hit_and_missed(ref, f"frame {k}")
        bad = np.flatnonzero(frames[k] != ref)
        assert bad.size == 0, f"frame {k} ({c}): {bad.size} pixels differ, first {bad[:8]}"
