"""GPU: the any-hit walk of the one-light lattice kernels' shadow rays (shadowed_wave, cg_rt_dev.h)
and their FP64 r_magnitude (light_rmag_inrange).  The walk keeps a per-lane `open` flag and runs
each candidate's t stage and u, v stage under one exec mask each, wave-uniform control around
them, instead of lanes returning from inside the loop; each lane's verdict, the (lane, candidate)
tests and their float operations are the other walk's, so every frame must equal the CPU oracle's,
every pixel (integer ARGB and float radiance: tolerance 0).

The light stands low behind the blocks, so that one frame -- and one 16 x 15 tile -- holds rays
whose first candidate blocks them, rays blocked by a later candidate after passing earlier ones,
and rays nothing blocks: _mix() shows that from the oracle's own DirectLight, called with the
first k triangles as blockers for growing k (the walk takes its candidates in ascending index
order).  Shapes: 64 x 45 (whole tiles), 70 x 31 (tiles cut at the right and the bottom) and 16 x 1
(two waves without a point), each with shared columns (pitch 33) and under a yaw (pitch 48);
LoadTestModel with its sphere and the blocks alone, with per-object masks and per-tile masks
(CG_OBJ_MASKS=0), a tile with more than seven triangle candidates among them (cg_rt_tile_masks);
the floor with the sphere as the only blocker; a sequence whose light moves; a batched dolly; the
RGB24 window; the F32 format.
Reference: raytracer/Source/skeleton.cpp:104-169, :289-335, :366-415."""
import ctypes as C
import os

import numpy as np
import pytest

import cgamd
import cgdist
import oracle
import rt_radiance_ref as rref

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 4)
YAW = 0.1745
LOW = (-0.9, 0.55, 0.9, 1.0)          # low, behind the tall block, seen from the camera
SIDE = (0.95, 0.2, -0.9, 1.0)         # in front, at the right wall: the short block shades the tall one
WHITE = (14.0, 14.0, 14.0)
BLACK_PIXEL = 0x80000000              # PutPixelSDL(0, 0, 0): none of the pixel's sub-rays hit
CAM0 = (0.0, 0.0, -3.0, 1.0)

# name: (W, H, focal, cameraPos, yaw or None)
CAMERAS = {
    "64x45": (64, 45, 45.0, CAM0, None),
    "64x45_yaw": (64, 45, 45.0, CAM0, YAW),
    "70x31": (70, 31, 31.0, CAM0, None),          # right tile 6 pixels wide, bottom tile 1 row tall
    "70x31_yaw": (70, 31, 31.0, CAM0, YAW),
    "16x1": (16, 1, 14.0, CAM0, None),            # 99 lattice points: waves 2 and 3 have none
    "16x1_yaw": (16, 1, 14.0, CAM0, YAW),
    "64x45_dolly": (64, 45, 45.0, (0.0, 0.0, float(np.float32(-3.0 + 0.005)), 1.0), None),
    "64x45_dolly2": (64, 45, 45.0, (0.0, 0.0, float(np.float32(-3.0 + 0.010)), 1.0), None),
    "160x45": (160, 45, 45.0, CAM0, None),        # ten tile columns, the room in the middle four
}
DOLLY = ["64x45", "64x45_dolly", "64x45_dolly2"]
# the light of each frame of the sequence: it moves along the back of the blocks and changes colour
MOVING = ((LOW, WHITE), ((-0.5, 0.55, 0.9, 1.0), (9.0, 14.0, 5.0)), ((0.4, 0.3, 0.9, 1.0), (14.0, 14.0, 14.0)))

_REF = {}


def _sub_scene(first, last, sphere):
    tris, _, sph = cgamd.rt_scene()
    out = (cgamd.Tri * (last - first))()
    for k, i in enumerate(range(first, last)):
        C.memmove(C.byref(out[k]), C.byref(tris[i]), C.sizeof(cgamd.Tri))
    return out, len(out), sph if sphere else None


SCENES = {
    "test_model": lambda: cgamd.rt_scene(),                 # the room, the two blocks, the sphere
    "blocks": lambda: _sub_scene(10, 28, False),            # the two blocks alone: misses beside hits
    "floor_sphere": lambda: _sub_scene(0, 2, True),         # the floor and the sphere: the only blocker
}


def _lights(pos=LOW, colour=WHITE):
    arr = cgamd.default_lights()
    arr[0].position = cgamd.Vec4(*pos)
    arr[0].colour = cgamd.Vec3(*colour)
    return arr


def _oracle_scene(scene):
    tris, n, sph = SCENES[scene]()
    otris = (oracle.RtTri * len(tris)).from_buffer_copy(tris)
    osph = C.pointer(oracle.Sphere.from_buffer_copy(sph)) if sph is not None else None
    return otris, n, osph, 1 if sph is not None else 0


def _reference(scene, cam, pos=LOW, colour=WHITE):
    """The CPU oracle's frame, computed once per (scene, camera, light) and never modified."""
    key = (scene, cam, pos, colour)
    if key not in _REF:
        W, H, f, cpos, yaw = CAMERAS[cam]
        R = list(cgamd.yaw_matrix(yaw)) if yaw is not None else None
        p = oracle.rt_params(W, H, f, cpos, R, lights=[(pos, colour)])
        _REF[key] = oracle.rt_draw(p, threads=THREADS, scene=_oracle_scene(scene))
        _REF[key].setflags(write=False)
    return _REF[key]


def _content(scene, cam, pos=LOW, colour=WHITE, missed=True):
    """Not vacuous, by the oracle: lit pixels, pixels in shadow (hit pixels whose value is the one a
    black light gives) and, unless the frame is filled, pixels that missed.  Returns the frame."""
    ref, unlit = _reference(scene, cam, pos, colour), _reference(scene, cam, pos, (0.0, 0.0, 0.0))
    n_missed = int((ref == BLACK_PIXEL).sum())
    n_shadow = int(((ref == unlit) & (ref != BLACK_PIXEL)).sum())
    n_lit = int((ref != unlit).sum())
    assert (n_missed > 0 or not missed) and n_shadow > 0 and n_lit > 0, \
        f"{scene}/{cam}: {n_missed} missed, {n_shadow} in shadow, {n_lit} lit"
    return ref


def _first_blockers(scene, cam, pos=LOW):
    """Per pixel's centre ray, from the oracle's DirectLight: -3 no hit, -2 the surface faces away
    from the light (zero with no blocker at all), -1 lit, k >= 0 the lowest k such that triangles
    0..k as the only blockers leave it in shadow, n_tris when only the sphere does.  Computed once."""
    key = ("first", scene, cam, pos)
    if key in _REF:
        return _REF[key]
    lib, glib = oracle.load(), cgamd.load()
    tris, n, sph, n_sph = _oracle_scene(scene)
    c = _camera(cam)
    light = oracle.Light(oracle.V4(*pos), oracle.V3(*WHITE))
    s, d, hit = cgamd.Vec4(), cgamd.Vec4(), oracle.Isect()
    out = np.full((c.height, c.width), -3, np.int32)

    def dark(k, ns):
        v = lib.cgo_rt_direct_light(C.byref(hit), tris, k, sph, ns, C.byref(light), None)
        return v.x == 0.0 and v.y == 0.0 and v.z == 0.0

    for v in range(c.height):
        for u in range(c.width):
            assert glib.cg_rt_pixel_ray(C.byref(c), u, v, 4, C.byref(s), C.byref(d)) == 0
            if not lib.cgo_rt_closest(oracle.V4(s.x, s.y, s.z, s.w), oracle.V4(d.x, d.y, d.z, d.w), tris, n, sph,
                                      n_sph, C.byref(hit), None):
                continue
            if dark(0, 0):
                out[v, u] = -2
            elif not dark(n, n_sph):
                out[v, u] = -1
            else:
                out[v, u] = next((k for k in range(n) if dark(k + 1, 0)), n)
    out.setflags(write=False)
    _REF[key] = out
    return out


def _mix(scene, cam, pos=LOW):
    """Some 16 x 15 tile holds, by the oracle, a lit ray, a ray whose first blocker is triangle a, and
    a ray whose first blocker is a later triangle b > a -- which a, a candidate of the same tile, was
    tested against first and did not block.  Returns (tile, a, b)."""
    first = _first_blockers(scene, cam, pos)
    n = SCENES[scene]()[1]
    H, W = first.shape
    for ty in range(0, H, 15):
        for tx in range(0, W, 16):
            t = first[ty:ty + 15, tx:tx + 16]
            tri = np.unique(t[(t >= 0) & (t < n)])
            if (t == -1).any() and len(tri) >= 2:
                return (tx // 16, ty // 15), int(tri[0]), int(tri[-1])
    raise AssertionError(f"{scene}/{cam}: no tile mixes lit rays with rays of two different first blockers")


def _camera(cam):
    W, H, f, pos, yaw = CAMERAS[cam]
    return cgamd.rt_camera(W, H, f, pos, cgamd.yaw_matrix(yaw) if yaw is not None else None)


def _on_lattice(scene, cam, shard=None):
    tris, n, sph = SCENES[scene]()
    route = "lattice_yaw" if CAMERAS[cam][4] is not None else "lattice"
    assert cgamd.rt_route(_camera(cam), n, 1 if sph is not None else 0, 1, shard) == route


@pytest.fixture
def scene_of(ctx):
    """Sets a scene; LoadTestModel is back afterwards (the session's context is shared)."""
    def set_scene(scene):
        tris, n, sph = SCENES[scene]()
        ctx.rt_set_scene(tris, n, sph, 1 if sph is not None else 0)
        return ctx
    yield set_scene
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)


def _same(got, ref, what):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(ref).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first {bad[:8]}"


def _frames(ctx, names, shard=None, fmt=None, lights=None, cols=None):
    """One cg_rt_render_frames_device call: per frame H x cols pixels (uint32) or wire bytes (RGB24)."""
    import torch
    W, H = CAMERAS[names[0]][:2]
    cols = cols or W
    fmt = cgamd.PIX_ARGB8888 if fmt is None else fmt
    bpp = 3 if fmt == cgamd.PIX_RGB24 else 4
    stride = W * ((H + 7) // 8 * 8)   # pixels: device frames hold whole 8-row stripes
    out = torch.zeros(len(names) * stride * 4 + 64, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_frames_device([_camera(c) for c in names], out.data_ptr(), shard, s.cuda_stream,
                                _lights() if lights is None else lights,
                                frame_stride=stride if bpp == 4 else 0, pix_format=fmt)
    s.synchronize()
    raw = out.cpu().numpy()
    if bpp == 4:
        return raw[:len(names) * stride * 4].view(np.uint32).reshape(len(names), stride)[:, :H * cols]
    return raw[:len(names) * H * cols * 3].reshape(len(names), H * cols * 3)


@pytest.mark.parametrize("cam", ["64x45", "64x45_yaw", "70x31", "70x31_yaw", "16x1", "16x1_yaw"])
def test_anyhit_low_light_frames(scene_of, cam):
    """Each frame size at both pitches under the low light; the larger frames have a tile that
    mixes lit rays, rays blocked by an early candidate and rays blocked by a later one."""
    ref = _content("test_model", cam, missed=False)
    if not cam.startswith("16x1"):
        _mix("test_model", cam)
    _on_lattice("test_model", cam)
    argb, _ = scene_of("test_model").rt_render(_camera(cam), lights=_lights())
    _same(argb, ref, cam)


@pytest.mark.parametrize("knob", ["on", "off"])
@pytest.mark.parametrize("scene,pos", [("test_model", LOW), ("blocks", SIDE)])
def test_anyhit_objects_and_many_candidates(scene_of, monkeypatch, scene, pos, knob):
    """LoadTestModel with its sphere and the blocks alone (misses beside hits inside a chunk), the
    shadow masks per object and (CG_OBJ_MASKS=0) per tile.  In LoadTestModel under the low light a
    walk has more than seven triangle candidates: some tile's mask, and with per-object masks some
    object's, holds that many."""
    if knob == "off":
        monkeypatch.setenv("CG_OBJ_MASKS", "0")
    else:
        monkeypatch.delenv("CG_OBJ_MASKS", raising=False)
    cam = "64x45"
    ref = _content(scene, cam, pos)
    _mix(scene, cam, pos)
    _on_lattice(scene, cam)
    ctx = scene_of(scene)
    argb, _ = ctx.rt_render(_camera(cam), lights=_lights(pos))
    _same(argb, ref, f"{scene}/{cam}, object masks {knob}")
    masks, obj = ctx.rt_tile_masks(0)
    assert (obj is not None) == (knob == "on")
    if scene == "test_model":
        tri_bits = (1 << 62) - 1
        most = lambda a: max(bin(int(m) & tri_bits).count("1") for m in np.asarray(a).reshape(-1))
        assert most(masks[..., 1]) > 7, "no tile with more than seven shadow candidates"
        assert obj is None or most(obj) > 7, "no object with more than seven shadow candidates"


def test_anyhit_sphere_is_the_only_blocker(scene_of):
    """The floor and the sphere: no triangle blocks any ray (the oracle's DirectLight with the
    triangles alone leaves no ray in shadow), the sphere's test alone decides."""
    scene, cam, pos = "floor_sphere", "64x45", (0.0, -0.5, -0.7, 1.0)
    ref = _content(scene, cam, pos)
    first = _first_blockers(scene, cam, pos)
    n = SCENES[scene]()[1]
    assert (first == n).sum() > 0 and ((first >= 0) & (first < n)).sum() == 0 and (first == -1).sum() > 0
    _on_lattice(scene, cam)
    argb, _ = scene_of(scene).rt_render(_camera(cam), lights=_lights(pos))
    _same(argb, ref, f"{scene}/{cam}")


def test_anyhit_sequence_light_moves(scene_of):
    """One cg_rt_render_sequence_device call of three frames, the light at another place behind the
    blocks in each: the candidates and which of them blocks change from frame to frame."""
    import torch
    ctx = scene_of("test_model")
    W, H = CAMERAS["64x45"][:2]
    stride = W * ((H + 7) // 8 * 8)
    out = torch.zeros(len(MOVING) * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_sequence_device([_camera("64x45")] * len(MOVING), [_lights(p, c) for p, c in MOVING], out.data_ptr(),
                                  None, s.cuda_stream, frame_stride=stride)
    s.synchronize()
    got = out.cpu().numpy().view(np.uint32).reshape(len(MOVING), stride)[:, :W * H]
    for k, (pos, colour) in enumerate(MOVING):
        _same(got[k], _content("test_model", "64x45", pos, colour, missed=False), f"frame {k} (light {pos}, {colour})")


def test_anyhit_batched_dolly(scene_of):
    """Three frames of a dolly in one call under the low light."""
    ctx = scene_of("test_model")
    got = _frames(ctx, DOLLY)
    for k, c in enumerate(DOLLY):
        _same(got[k], _content("test_model", c, missed=False), f"frame {k} ({c})")


def test_anyhit_rgb24_window(scene_of):
    """The RGB24 wire format over the output window of the columns anything can be seen in."""
    ctx = scene_of("test_model")
    cam = "160x45"
    W, H = CAMERAS[cam][:2]
    ref = _content("test_model", cam)
    tris, n, sph = cgamd.rt_scene()
    c0, c1 = cgamd.frame_columns(tris, n, sph, 1, _camera(cam))
    assert 0 < c0 and c1 < W
    sh = cgamd.RtShard(row0=0, rows=H, col0=c0, cols=c1 - c0)
    got = _frames(ctx, [cam], sh, cgamd.PIX_RGB24, cols=c1 - c0)
    _same(got[0], cgdist.pack_rgb24_np(cgdist.window_np(ref, W, c0, c1 - c0)), "RGB24 window")


@pytest.mark.parametrize("yaw", [None, YAW])
def test_anyhit_f32_format(scene_of, yaw):
    """CG_PIX_RGBA_F32 (the *_f32 kernels): float radiance and coverage against the pixel loop
    restated over the oracle's ClosestIntersection and DirectLight, bit for bit."""
    import torch
    R = list(cgamd.yaw_matrix(yaw)) if yaw is not None else None
    case = dict(scene="room", width=70, height=31, focal=31.0, cam=list(CAM0), R=R, lights=[[list(LOW), list(WHITE)]])
    key = ("f32", yaw)
    if key not in _REF:
        _REF[key] = rref.radiance(case)
        _REF[key].setflags(write=False)
    ref = _REF[key]
    ctx = scene_of("test_model")
    cam = rref.camera(case)
    W, H = cam.width, cam.height
    stride = W * ((H + 7) // 8 * 8)   # pixels: device frames hold whole 8-row stripes
    buf = torch.zeros(stride * 4, dtype=torch.float32, device="cuda")
    ctx.rt_render_frames_device([cam], buf.data_ptr(), lights=_lights(), frame_stride=stride,
                                pix_format=cgamd.PIX_RGBA_F32)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()[:H * W * 4]
    _same(got.view(np.uint32), np.ascontiguousarray(ref).reshape(-1).view(np.uint32), f"F32, yaw {yaw}")
