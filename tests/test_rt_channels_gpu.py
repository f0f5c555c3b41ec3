"""GPU: one divide per distinct channel in the one-light lattice kernels' lit quotient (cg_rt_dev.h
chan_share / div3_by_shared, used by lat_direct_light_tab; the light-set kernels, which measured
slower with it, keep their three quotients and are covered all the same).  :412's
(litColour * a) / area is three IEEE divides by one area; a channel whose litColour bits equal
another channel's in every active lane of the wave takes that channel's quotient instead of a
divide of its own.  The decision compares integer bits per wave, so it must hold for colours that
differ per triangle inside one 64-point chunk, for +0 against -0, for a light that makes equal
colours unequal (and unequal colours equal), per light of a light set and per frame of a sequence.
Every frame must equal the CPU oracle's, every pixel (integer ARGB: tolerance 0).
Reference: raytracer/Source/skeleton.cpp:366-415 (:412)."""
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

# name: (W, H, focal, cameraPos, yaw or None)
CAMERAS = {
    "64x60": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None),
    "cut_80x75": (80, 75, 75.0, (0.0, 0.0, -3.0, 1.0), None),        # right and bottom tiles cut
    "64x60_yaw": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), YAW),          # per-pixel columns (pitch 48)
    "64x60_dolly": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.005)), 1.0), None),
    "64x60_dolly2": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.010)), 1.0), None),
}
A, B, CC = 0.75, 0.15, 0.4
# (a,a,a), (a,a,b), (a,b,a), (b,a,a), (a,b,c): cycled per triangle, so the two triangles of a
# block face, which meet inside 64-point chunks, carry different patterns
MIXED = ((A, A, A), (A, A, B), (A, B, A), (B, A, A), (A, B, CC))
# bits, not values: +0 == -0 as floats, and under a light with a negative channel the zero
# products' signs differ between channels
ZEROS = ((0.0, -0.0, 0.0), (-0.0, -0.0, 0.5))
ZERO_LIGHT = (14.0, -7.0, 14.0)

_REF = {}


def _copy(tris, idx):
    out = (cgamd.Tri * len(idx))()
    for k, i in enumerate(idx):
        C.memmove(C.byref(out[k]), C.byref(tris[i]), C.sizeof(cgamd.Tri))
    return out


def _blocks(colours):
    """Triangles 10..27 of LoadTestModel: the two blocks, no sphere; colours cycled."""
    tris, _, _ = cgamd.rt_scene()
    out = _copy(tris, range(10, 28))
    for k in range(len(out)):
        out[k].color = cgamd.Vec3(*colours[k % len(colours)])
    return out, len(out), None


SCENES = {
    "mixed": lambda: _blocks(MIXED),
    "one_pattern": lambda: _blocks(((A, B, A),)),        # whole waves skip the z divide
    "zeros": lambda: _blocks(ZEROS),
    "grey": lambda: _blocks(((0.9, 0.9, 0.9),)),
    "products_equal": lambda: _blocks(((0.5, 0.25, 0.3),)),
    "test_model": lambda: cgamd.rt_scene(),               # with its sphere
}


def _lights(colour):
    arr = cgamd.default_lights()
    arr[0].position = cgamd.Vec4(*LIGHT_POS)
    arr[0].colour = cgamd.Vec3(*colour)
    return arr


def _tuples(lights):
    return [((l.position.x, l.position.y, l.position.z, l.position.w), (l.colour.x, l.colour.y, l.colour.z))
            for l in lights]


def _reference(scene, cam, lights):
    """The CPU oracle's frame, computed once per (scene, camera, lights) and never modified;
    lights: a tuple of (position, colour) tuples."""
    key = (scene, cam, lights)
    if key not in _REF:
        W, H, f, pos, yaw = CAMERAS[cam]
        tris, n, sph = SCENES[scene]()
        R = list(cgamd.yaw_matrix(yaw)) if yaw is not None else None
        otris = (oracle.RtTri * len(tris)).from_buffer_copy(tris)
        osph = C.pointer(oracle.Sphere.from_buffer_copy(sph)) if sph is not None else None
        p = oracle.rt_params(W, H, f, pos, R, lights=list(lights))
        _REF[key] = oracle.rt_draw(p, threads=THREADS, scene=(otris, n, osph, 1 if sph is not None else 0))
        _REF[key].setflags(write=False)
    return _REF[key]


def _camera(cam):
    W, H, f, pos, yaw = CAMERAS[cam]
    return cgamd.rt_camera(W, H, f, pos, cgamd.yaw_matrix(yaw) if yaw is not None else None)


@pytest.fixture
def scene_of(ctx):
    """Sets a scene; LoadTestModel is back afterwards (the session's context is shared)."""
    def set_scene(scene):
        tris, n, sph = SCENES[scene]()
        ctx.rt_set_scene(tris, n, sph, 1)
        return ctx, n, 1 if sph is not None else 0
    yield set_scene
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)


def _assert_frame(ctx, scene, cam, lights, route):
    tris, n, sph = SCENES[scene]()
    assert cgamd.rt_route(_camera(cam), n, 1 if sph is not None else 0, len(lights)) == route
    argb, _ = ctx.rt_render(_camera(cam), lights=lights)
    bad = np.flatnonzero(argb != _reference(scene, cam, tuple(_tuples(lights))))
    assert bad.size == 0, f"{scene}/{cam}: {bad.size} pixels differ, first {bad[:8]}"


def _route(cam, lights=False):
    yaw = CAMERAS[cam][4] is not None
    return ("lights" if lights else "lattice") + ("_yaw" if yaw else "")


@pytest.mark.parametrize("cam", ["64x60", "cut_80x75", "64x60_yaw"])
@pytest.mark.parametrize("scene", ["mixed", "one_pattern", "test_model"])
def test_channels_patterns(scene_of, scene, cam):
    """Every channel pattern beside every other inside one chunk; one pattern throughout (whole
    waves skip a divide); LoadTestModel with its sphere."""
    ctx, _, _ = scene_of(scene)
    _assert_frame(ctx, scene, cam, _lights(WHITE), _route(cam))


@pytest.mark.parametrize("cam", ["64x60", "64x60_yaw"])
def test_channels_signed_zeros(scene_of, cam):
    """(0, -0, 0) and (-0, -0, 0.5) under a light with a negative channel: equal as floats,
    different as bits, and the zero products' signs differ between channels."""
    ctx, _, _ = scene_of("zeros")
    _assert_frame(ctx, "zeros", cam, _lights(ZERO_LIGHT), _route(cam))


@pytest.mark.parametrize("scene,light", [("grey", (14.0, 7.0, 14.0)), ("products_equal", (2.0, 4.0, 1.0))])
def test_channels_light_decides(scene_of, scene, light):
    """Equal colours whose products differ (grey under (14, 7, 14)); different colours whose
    products are equal ((0.5, 0.25, 0.3) under (2, 4, 1): 1, 1 and 0.3 -- x == y only)."""
    ctx, _, _ = scene_of(scene)
    _assert_frame(ctx, scene, "64x60", _lights(light), _route("64x60"))


@pytest.mark.parametrize("cam", ["64x60", "64x60_yaw"])
def test_channels_light_set(scene_of, cam):
    """A 2 x 2 area light on the mixed-pattern scene: rt_lattice_lights_kernel, the quotients
    per (point, light)."""
    ctx, _, _ = scene_of("mixed")
    lights = cgamd.area_lights(_lights(WHITE)[0], 0.1, 2)
    _assert_frame(ctx, "mixed", cam, lights, _route(cam, lights=True))


def test_channels_sequence_light_per_frame(scene_of):
    """One cg_rt_render_sequence_device call of three frames whose lights are white, (14, 7, 14)
    and black: the decision is taken per frame."""
    import torch
    ctx, _, _ = scene_of("grey")
    W, H = CAMERAS["64x60"][:2]
    colours = [WHITE, (14.0, 7.0, 14.0), (0.0, 0.0, 0.0)]
    stride = W * ((H + 7) // 8 * 8)   # device frames hold whole 8-row stripes
    out = torch.zeros(len(colours) * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_sequence_device([_camera("64x60")] * len(colours), [_lights(c) for c in colours], out.data_ptr(),
                                  None, s.cuda_stream, frame_stride=stride)
    s.synchronize()
    frames = out.cpu().numpy().view(np.uint32).reshape(len(colours), stride)[:, :W * H]
    for k, c in enumerate(colours):
        bad = np.flatnonzero(frames[k] != _reference("grey", "64x60", tuple(_tuples(_lights(c)))))
        assert bad.size == 0, f"frame {k} (light {c}): {bad.size} pixels differ, first {bad[:8]}"


def test_channels_batched_device_call(scene_of):
    """Three frames of a dolly in one cg_rt_render_frames_device call, the mixed-pattern scene."""
    import torch
    ctx, _, _ = scene_of("mixed")
    names = ["64x60", "64x60_dolly", "64x60_dolly2"]
    W, H = CAMERAS["64x60"][:2]
    stride = W * ((H + 7) // 8 * 8)
    out = torch.zeros(len(names) * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_frames_device([_camera(c) for c in names], out.data_ptr(), None, s.cuda_stream, frame_stride=stride)
    s.synchronize()
    frames = out.cpu().numpy().view(np.uint32).reshape(len(names), stride)[:, :W * H]
    white = tuple(_tuples(_lights(WHITE)))
    for k, c in enumerate(names):
        bad = np.flatnonzero(frames[k] != _reference("mixed", c, white))
        assert bad.size == 0, f"frame {k} ({c}): {bad.size} pixels differ, first {bad[:8]}"
