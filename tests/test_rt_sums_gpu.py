"""GPU: the one-light lattice kernel's table of per-object products and its pixel sums without
tests (cg_rt.hip LatTab, lattice_body).  Every lattice point carries (DirectLight, table slot)
through LDS -- a miss the value (0, 0, 0) and the zero slot, whose ambient product is
(+0, +0, +0) -- and a pixel adds its nine points' values and ambient products in the
reference's order with no comparison, branch or `valid` flag.  Adding +0 for a sub-ray that
missed is an identity (the running sum starts at +0 and can never be -0), and the products
colour * lightColour and colour * indirect are the same float multiplies formed once per
object, so every frame must equal the CPU oracle's, every pixel (integer ARGB: tolerance 0).
Reference: raytracer/Source/skeleton.cpp:104-169 (:156 the ambient term), :366-415 (:412)."""
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
# red channel of a pixel k of whose nine sub-rays hit, every colour (0.9, 0.9, 0.9), the light
# black and indirect 0.5 (each hit adds 0.45; the pixel is the sum / 9)
RED_OF_HITS = (0, 12, 25, 38, 50, 63, 76, 89, 102, 114)

# name: (W, H, focal, cameraPos, yaw or None)
CAMERAS = {
    "64x60": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None),
    "cut_80x75": (80, 75, 75.0, (0.0, 0.0, -3.0, 1.0), None),        # right and bottom tiles cut
    "48x45": (48, 45, 90.0, (0.1, 0.3, -3.0, 1.0), None),
    "64x60_yaw": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), YAW),          # per-pixel columns, int8 slots
    "64x60_dolly": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.005)), 1.0), None),
}
SIGNED_COLOURS = ((-0.5, 0.0, 0.7), (0.3, -0.2, 0.0), (0.0, 0.0, 0.0))
SIGNED_LIGHT = (14.0, 0.0, -3.0)

_REF = {}


def _copy(tris, idx):
    out = (cgamd.Tri * len(idx))()
    for k, i in enumerate(idx):
        C.memmove(C.byref(out[k]), C.byref(tris[i]), C.sizeof(cgamd.Tri))
    return out


def _blocks(colours=None):
    """Triangles 10..27 of LoadTestModel: the two blocks, no sphere; colours cycled when given."""
    tris, _, _ = cgamd.rt_scene()
    out = _copy(tris, range(10, 28))
    if colours is not None:
        for k in range(len(out)):
            out[k].color = cgamd.Vec3(*colours[k % len(colours)])
    return out, len(out), None


def _padded(n_behind):
    """n_behind triangles wholly behind the camera (z < -3.5: no camera ray hits them, and no
    shadow ray towards the light at z = -0.7 reaches them), then LoadTestModel's 28 triangles;
    the sphere present."""
    tris, n, sph = cgamd.rt_scene()
    out = (cgamd.Tri * (n_behind + n))()
    for k in range(n_behind):
        x = -0.9 + 0.05 * k
        out[k].v0 = cgamd.Vec4(x, -0.5, -4.0, 1.0)
        out[k].v1 = cgamd.Vec4(x + 0.04, -0.5, -4.0, 1.0)
        out[k].v2 = cgamd.Vec4(x, -0.4, -4.2, 1.0)
        out[k].normal = cgamd.Vec4(0.0, 0.8944272, 0.4472136, 1.0)
        out[k].color = cgamd.Vec3(0.75, 0.15, 0.15)
    for i in range(n):
        C.memmove(C.byref(out[n_behind + i]), C.byref(tris[i]), C.sizeof(cgamd.Tri))
    return out, n_behind + n, sph


SCENES = {
    "blocks": lambda: _blocks(),
    "blocks_signed": lambda: _blocks(SIGNED_COLOURS),
    "blocks_grey": lambda: _blocks(((0.9, 0.9, 0.9),)),
    "padded64": lambda: _padded(36),
    # the lattice kernels take scenes of up to 62 triangles: the highest slot they can meet
    "padded62": lambda: _padded(34),
}


def _lights(colour):
    arr = cgamd.default_lights()
    arr[0].position = cgamd.Vec4(*LIGHT_POS)
    arr[0].colour = cgamd.Vec3(*colour)
    return arr


def _light_of(scene):
    return SIGNED_LIGHT if scene == "blocks_signed" else (14.0, 14.0, 14.0)


def _reference(scene, cam, light=None, indirect=0.5):
    """The CPU oracle's frame, computed once per (scene, camera, light)."""
    light = _light_of(scene) if light is None else light
    key = (scene, cam, light, indirect)
    if key not in _REF:
        W, H, f, pos, yaw = CAMERAS[cam]
        tris, n, sph = SCENES[scene]()
        R = list(cgamd.yaw_matrix(yaw)) if yaw is not None else None
        otris = (oracle.RtTri * len(tris)).from_buffer_copy(tris)
        osph = C.pointer(oracle.Sphere.from_buffer_copy(sph)) if sph is not None else None
        p = oracle.rt_params(W, H, f, pos, R, indirect=indirect, lights=[(LIGHT_POS, light)])
        _REF[key] = oracle.rt_draw(p, threads=THREADS, scene=(otris, n, osph, 1 if sph is not None else 0))
    return _REF[key]


def _camera(cam):
    W, H, f, pos, yaw = CAMERAS[cam]
    return cgamd.rt_camera(W, H, f, pos, cgamd.yaw_matrix(yaw) if yaw is not None else None)


def _hit_counts(cam):
    """How many of each pixel's nine sub-rays hit the blocks, from the oracle's frame of the grey
    scene under a black light."""
    red = (_reference("blocks_grey", cam, light=(0.0, 0.0, 0.0)) >> 16) & 0xff
    assert set(np.unique(red).tolist()) <= set(RED_OF_HITS), np.unique(red)
    return np.searchsorted(np.array(RED_OF_HITS), red)


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


def _assert_frame(ctx, scene, cam):
    argb, _ = ctx.rt_render(_camera(cam), lights=_lights(_light_of(scene)))
    bad = np.flatnonzero(argb != _reference(scene, cam))
    assert bad.size == 0, f"{scene}/{cam}: {bad.size} pixels differ, first {bad[:8]}"


@pytest.mark.parametrize("cam", ["64x60", "cut_80x75", "48x45", "64x60_yaw"])
def test_sums_partially_covered_pixels(scene_of, cam):
    """The blocks alone: pixels along their outlines have 1..8 of their nine sub-rays hit (checked
    on the oracle, so that the case is not vacuous) and add the zero slot for the others."""
    counts = _hit_counts(cam)
    seen = set(np.unique(counts).tolist())
    assert set(range(1, 9)) <= seen, f"{cam}: hit counts seen {sorted(seen)}"
    ctx, n, n_sph = scene_of("blocks")
    assert cgamd.rt_route(_camera(cam), n, n_sph, 1) == ("lattice_yaw" if CAMERAS[cam][4] else "lattice")
    _assert_frame(ctx, "blocks", cam)


def test_sums_signed_and_zero_products(scene_of):
    """Negative, -0 and all-zero entries in the table: colours with negative and zero channels
    under a light with a zero and a negative channel."""
    ctx, _, _ = scene_of("blocks_signed")
    _assert_frame(ctx, "blocks_signed", "64x60")


@pytest.mark.parametrize("cam", ["64x60", "64x60_yaw"])
@pytest.mark.parametrize("scene", ["padded64", "padded62"])
def test_sums_highest_slots(scene_of, scene, cam):
    """Hits on the last triangles of a 64-triangle scene and on the sphere beside misses (mask
    bits above 31).  The lattice kernels take scenes of up to 62 triangles (rt_use_lattice: the
    primary mask's two top bits are flags), so the 64-triangle frame is rendered by the pixel
    kernel; the same scene with 62 triangles is the one that reaches the lattice kernels'
    highest triangle slot (61), the sphere slot and the zero slot."""
    ctx, n, n_sph = scene_of(scene)
    if scene == "padded62":
        assert cgamd.rt_route(_camera(cam), n, n_sph, 1) == ("lattice_yaw" if CAMERAS[cam][4] else "lattice")
    _assert_frame(ctx, scene, cam)


def test_sums_batched_device_call(scene_of):
    """Three frames in one cg_rt_render_frames_device call: the first camera, that camera dollied
    by 0.005 in z, the first again; each == its oracle frame."""
    import torch
    ctx, _, _ = scene_of("blocks")
    names = ["64x60", "64x60_dolly", "64x60"]
    W, H = CAMERAS["64x60"][:2]
    stride = W * ((H + 7) // 8 * 8)   # device frames hold whole 8-row stripes
    out = torch.zeros(len(names) * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_frames_device([_camera(c) for c in names], out.data_ptr(), None, s.cuda_stream, frame_stride=stride)
    s.synchronize()
    frames = out.cpu().numpy().view(np.uint32).reshape(len(names), stride)[:, :W * H]
    for k, c in enumerate(names):
        bad = np.flatnonzero(frames[k] != _reference("blocks", c))
        assert bad.size == 0, f"frame {k} ({c}): {bad.size} pixels differ, first {bad[:8]}"
