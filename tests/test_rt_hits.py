"""CPU: the host side of the hit-plane calls (cg_rt_pixel_ray, cg_rt_hits*, cg_rt_pick) -- record
layout, argument errors, and the ray cg_rt_pixel_ray forms: exact values where every product is
exact (identity R), and a float32 numpy restatement of GLM's column sum (type_mat4x4.inl:641-652:
(m0 v.x + m1 v.y) + (m2 v.z + m3 v.w)) for a yawed and a pitched camera.  Tolerance 0."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import make_golden as mg
from test_rt_big_gpu import PITCH, YAW

CG_E_INVALID = -1
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return cgamd.load()


def test_record_layout():
    assert C.sizeof(cgamd.Isect) == 28 and cgamd.ISECT_DTYPE.itemsize == 28
    assert [cgamd.ISECT_DTYPE.fields[k][1] for k in ("position", "distance", "triangleIndex", "sphereIndex")] == \
        [0, 16, 20, 24]
    assert C.sizeof(cgamd.Vec4) == 16 and C.sizeof(cgamd.RtShard) == 28
    assert cgamd.HIT_NONE == np.iinfo(np.int32).min


def test_pixel_ray_argument_errors(lib):
    cam = cgamd.rt_camera(64, 48, 48.0)
    s, d = cgamd.Vec4(), cgamd.Vec4()
    ok = lambda *a: lib.cg_rt_pixel_ray(*a)   # noqa: E731
    assert ok(C.byref(cam), 0, 0, 0, C.byref(s), C.byref(d)) == 0
    assert ok(C.byref(cam), 63, 47, 8, C.byref(s), C.byref(d)) == 0
    for x, y, sub in [(-1, 0, 4), (64, 0, 4), (0, -1, 4), (0, 48, 4), (0, 0, -1), (0, 0, 9)]:
        assert ok(C.byref(cam), x, y, sub, C.byref(s), C.byref(d)) == CG_E_INVALID, (x, y, sub)
    assert ok(None, 0, 0, 4, C.byref(s), C.byref(d)) == CG_E_INVALID
    assert ok(C.byref(cam), 0, 0, 4, None, C.byref(d)) == CG_E_INVALID
    assert ok(C.byref(cam), 0, 0, 4, C.byref(s), None) == CG_E_INVALID
    with pytest.raises(ValueError):
        cgamd.rt_pixel_ray(cam, 0, 0, 9)


def test_hit_calls_reject_a_null_context(lib):
    """Without a context nothing can be checked further: CG_E_INVALID, no device touched."""
    cam = cgamd.rt_camera(64, 48, 48.0)
    buf = np.zeros(64 * 48, cgamd.ISECT_DTYPE)
    hit = C.c_int()
    assert lib.cg_rt_hits_device(None, C.byref(cam), 4, None, buf.ctypes.data, None, None, None) == CG_E_INVALID
    assert lib.cg_rt_hits(None, C.byref(cam), 4, buf.ctypes.data, None, None) == CG_E_INVALID
    assert lib.cg_rt_pick(None, C.byref(cam), 0, 0, 4, C.cast(buf.ctypes.data, C.POINTER(cgamd.Isect)),
                          C.byref(hit)) == CG_E_INVALID


@pytest.mark.parametrize("W,H,focal", [(64, 48, 48.0), (320, 256, 256.0), (33, 17, 20.5)])
def test_pixel_ray_identity_is_exact(W, H, focal):
    """Identity R: every product of the column sum is x * 1 or x * 0, so d = (x - W/2, y - H/2, focal, 1)
    (integer division, skeleton.cpp:126) and dir = (d.x + 0.5 i, d.y + 0.5 j, focal, 1) exactly."""
    campos = (0.25, -0.5, -3.0, 1.0)
    cam = cgamd.rt_camera(W, H, focal, campos)
    for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]:
        for s in range(9):
            i, j = s // 3 - 1, s % 3 - 1
            start, d = cgamd.rt_pixel_ray(cam, x, y, s)
            assert start.tolist() == [f32(c) for c in campos]
            assert d.tolist() == [float(x - W // 2) + 0.5 * i, float(y - H // 2) + 0.5 * j, float(f32(focal)), 1.0]
    c, d4 = cgamd.rt_pixel_ray(cam, W // 2, H // 2)      # the default sub-ray is the pixel centre
    assert d4.tolist() == [0.0, 0.0, float(f32(focal)), 1.0]


def _glm_ray(R, W, H, focal, x, y, s):
    """The float32 restatement: R column-major (m[4 c + r]), products first, then the two pair sums."""
    m = np.array(R, f32)
    v = np.array([x - W // 2, y - H // 2, focal, 1.0], f32)
    d = [(m[0 * 4 + k] * v[0] + m[1 * 4 + k] * v[1]) + (m[2 * 4 + k] * v[2] + m[3 * 4 + k] * v[3]) for k in range(4)]
    i, j = s // 3 - 1, s % 3 - 1
    return np.array([d[0] + f32(0.5) * f32(i), d[1] + f32(0.5) * f32(j), f32(focal), f32(1.0)], f32)


@pytest.mark.parametrize("name,R", [("yaw", YAW), ("pitch", PITCH)])
@pytest.mark.parametrize("W,H,focal", [(64, 48, 48.0), (320, 256, 256.0)])
def test_pixel_ray_matches_the_glm_column_sum(name, R, W, H, focal):
    cam = cgamd.rt_camera(W, H, focal, (0.0, 0.0, -3.0, 1.0), (C.c_float * 16)(*R))
    seen = set()
    for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]:
        for s in range(9):
            _, d = cgamd.rt_pixel_ray(cam, x, y, s)
            want = _glm_ray(R, W, H, focal, x, y, s)
            assert d.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (name, x, y, s, d, want)
            seen.add(d.tobytes())
    assert len(seen) == 45                               # every pixel's every sub-ray is its own ray
    # the rotation is felt: a rotated corner ray differs from the unrotated one
    _, d = cgamd.rt_pixel_ray(cam, 0, 0, 4)
    assert d[:2].tolist() != [float(-(W // 2)), float(-(H // 2))]


def test_pixel_rays_batch_equals_single_calls():
    cam = cgamd.rt_camera(16, 12, 12.0, R=(C.c_float * 16)(*mg.yaw_R(f32(0.3))))
    starts, dirs = cgamd.rt_pixel_rays(cam, 7)
    assert starts.shape == dirs.shape == (16 * 12, 4)
    for p in (0, 17, 16 * 12 - 1):
        s, d = cgamd.rt_pixel_ray(cam, p % 16, p // 16, 7)
        assert np.array_equal(starts[p], s) and np.array_equal(dirs[p], d)
    s2, d2 = cgamd.rt_pixel_rays(cam, 7, pixels=[17, 0])
    assert np.array_equal(d2, dirs[[17, 0]])
