"""Reference for CG_PIX_RGBA_F32 frames: the pixel loop of oracle/cg_oracle_rt.c:327-356 (raytracer
skeleton.cpp:120-166) restated over the oracle's own primitives, shared by test_rt_radiance.py
(which pins it to oracle.rt_draw without a GPU) and test_rt_radiance_gpu.py.

Per pixel: the nine sub-rays in the order i outer, j inner (cg_rt_pixel_ray's sub_ray 0..8);
cgo_rt_closest for each; for a hit, cgo_rt_direct_light per light in order, then
objectColor * indirect; every add and multiply a numpy float32 scalar operation (one rounding each);
at the end float32 / float32(9), or +0 when no sub-ray hit.  w counts the cgo_rt_closest results.

A case is a dict: scene (a key of scene()), width, height, focal, cam, R (16 floats, column-major,
or None), lights (a list of (position, colour)) and optionally area=dict(side, n) around lights[0].
"""
import ctypes as C

import numpy as np

import cgamd
import oracle
from test_rt_big_gpu import CASES as BIG_CASES, PITCH, YAW

F32 = np.float32
L0 = [[0.0, -0.5, -0.7, 1.0], [14.0, 14.0, 14.0]]
INDIRECT = 0.5


class Scene:
    """A scene for the library (cgamd.Tri, cgamd.Sphere) and the same bytes for the oracle."""

    def __init__(self, tris, n, sph=None):
        self.tris, self.n, self.sph = tris, n, sph
        self.otris = (oracle.RtTri * max(n, 1)).from_buffer_copy(bytes(tris)[:max(n, 1) * 76])
        self.osph = oracle.Sphere.from_buffer_copy(bytes(sph)) if sph is not None else None
        self.n_sph = 1 if sph is not None else 0

    def set(self, ctx):
        ctx.rt_set_scene(self.tris, self.n, self.sph, self.n_sph)

    def oracle_scene(self):
        """As oracle.rt_draw's `scene` argument."""
        return self.otris, self.n, C.pointer(self.osph) if self.osph is not None else None, self.n_sph


_SCENES = {}


def scene(name):
    """'room': LoadTestModel (28 triangles and the sphere); 'room+<k>': the same followed by the
    first k triangles of random_scene(64, 0x5EED); 'rand<n>': random_scene(n, 0x5EED);
    'rand<n>+sphere': the same with the room's sphere."""
    if name not in _SCENES:
        room = cgamd.rt_scene()
        if name == "room":
            _SCENES[name] = Scene(*room)
        elif name.startswith("room+"):
            k = int(name[5:])
            raw = bytes(room[0])[:room[1] * 76] + bytes(cgamd.random_scene(64, 0x5EED))[:k * 76]
            _SCENES[name] = Scene((cgamd.Tri * (room[1] + k)).from_buffer_copy(raw), room[1] + k, room[2])
        else:
            n = int(name[4:].split("+")[0])
            _SCENES[name] = Scene(cgamd.random_scene(n, 0x5EED), n, room[2] if name.endswith("+sphere") else None)
    return _SCENES[name]


def _small(width=70, height=50, focal=50.0, R=None, lights=(L0,), **kw):
    return dict(dict(scene="room", width=width, height=height, focal=focal, cam=[0, 0, -3.0, 1], R=R,
                     lights=list(lights)), **kw)


def _big(case, **kw):
    return dict(dict(scene="rand500", width=64, height=48, focal=48.0, cam=[0, 0, -3.0, 1]), **dict(BIG_CASES[case], **kw))


AREA4 = dict(side=0.1, n=2)
# name -> (case, the CG_RT_ROUTE_* name the frame must take)
CASES = {
    # the room: 70 x 50 cuts the right and bottom 16 x 15 tiles
    "id_1": (_small(), "lattice"),
    "yaw_1": (_small(R=YAW), "lattice_yaw"),
    "pitch_1": (_small(R=PITCH), "pixel"),
    "id_4": (_small(area=AREA4), "lights"),
    "yaw_4": (_small(R=YAW, area=AREA4), "lights_yaw"),
    "pitch_4": (_small(R=PITCH, area=AREA4), "pixel"),
    "id_0": (_small(lights=()), "pixel"),
    # more lights than a lattice word holds: off the lattice (32 x 24 keeps the restatement short)
    "id_65": (_small(32, 24, 24.0, lights=[[[-0.32 + 0.01 * k, -0.5, -0.7, 1.0], [0.25, 0.2, 0.3]] for k in range(65)]),
              "pixel"),
    # 160 x 45, focal 45: tile columns outside cg_rt_frame_columns' bound, and certified-black tiles
    "wide_1": (_small(160, 45, 45.0), "lattice"),
    "wide_4": (_small(160, 45, 45.0, area=AREA4), "lights"),
    # the route boundary
    "tris_64": (_small(64, 48, 48.0, scene="room+36"), "pixel"),
    "tris_65": (_small(64, 48, 48.0, scene="room+37"), "big_lattice"),
    # random_scene(500): the large-scene modes of test_rt_big_gpu.py
    "big_lat_1": (_big("lat_1"), "big_lattice"),
    "big_lat_area16": (_big("lat_area16"), "big_lattice"),
    "big_yawlat_1": (_big("yawlat_1"), "big_lattice_yaw"),
    "big_yawlat_area16": (_big("yawlat_area16"), "big_lattice_yaw"),
    "big_pix_pitch_1": (_big("pix_pitch_1"), "big_pixel"),
    "big_pix_pitch_area16": (_big("pix_pitch_area16"), "big_pixel"),
    "big_pix_area81": (_big("pix_area81", width=32, height=24, focal=24.0), "big_pixel"),
    "big_inside_lat_1": (_big("inside_lat_1"), "big_lattice"),
    "big_sphere_lat_1": (_big("lat_1", scene="rand500+sphere"), "big_lattice"),
}


def lights_of(case):
    """[(position, colour)] of a case: explicit, or the area light around lights[0] (float32 values)."""
    if "area" in case:
        (p, c), a = case["lights"][0], case["area"]
        return oracle.rt_area_lights(tuple(p), tuple(c), a["side"], a["n"])
    return [(tuple(p), tuple(c)) for p, c in case["lights"]]


def camera(case):
    R = (C.c_float * 16)(*case["R"]) if case["R"] is not None else None
    return cgamd.rt_camera(case["width"], case["height"], case["focal"], tuple(case["cam"]), R, INDIRECT)


def light_array(lights):
    arr = (cgamd.Light * len(lights))()
    for i, (p, c) in enumerate(lights):
        arr[i].position = cgamd.Vec4(*p)
        arr[i].colour = cgamd.Vec3(*c)
    return arr


def oracle_params(case):
    return oracle.rt_params(case["width"], case["height"], case["focal"], tuple(case["cam"]), case["R"], INDIRECT,
                            lights_of(case))


def radiance(case):
    """float32[H, W, 4] of the case by the restated pixel loop."""
    lib, glib = oracle.load(), cgamd.load()
    sc = scene(case["scene"])
    tris, n, sph, n_sph = sc.oracle_scene()
    cam = camera(case)
    W, H = cam.width, cam.height
    olights = (oracle.Light * max(len(lights_of(case)), 1))()
    for k, (p, c) in enumerate(lights_of(case)):
        olights[k] = oracle.Light(oracle.V4(*p), oracle.V3(*c))
    lrefs = [C.byref(olights[k]) for k in range(len(lights_of(case)))]
    ind = F32(cam.indirect)
    zero, nine = F32(0.0), F32(9.0)
    out = np.zeros((H, W, 4), np.float32)
    s, d, hit = cgamd.Vec4(), cgamd.Vec4(), oracle.Isect()
    ps, pd, ph, pc = C.byref(s), C.byref(d), C.byref(hit), C.byref(cam)
    ray, closest, direct = glib.cg_rt_pixel_ray, lib.cgo_rt_closest, lib.cgo_rt_direct_light
    for v in range(H):
        for u in range(W):
            x, y, z, w = zero, zero, zero, 0
            for k in range(9):                                   # i outer, j inner (:336-337)
                if ray(pc, u, v, k, ps, pd) != 0:
                    raise ValueError("cg_rt_pixel_ray")
                if not closest(oracle.V4(s.x, s.y, s.z, s.w), oracle.V4(d.x, d.y, d.z, d.w), tris, n, sph, n_sph, ph,
                               None):
                    continue
                w += 1
                col = tris[hit.triangleIndex].color if hit.triangleIndex != -1 else sph[hit.sphereIndex].color
                for lr in lrefs:                                 # :346-349
                    dl = direct(ph, tris, n, sph, n_sph, lr, None)
                    x, y, z = x + F32(dl.x), y + F32(dl.y), z + F32(dl.z)
                x, y, z = x + F32(col.x) * ind, y + F32(col.y) * ind, z + F32(col.z) * ind   # :350
            if w:
                out[v, u] = (x / nine, y / nine, z / nine, w)   # :354
    return out


_REF = {}


def reference(name):
    """radiance(CASES[name]), computed once; treat it as read-only."""
    if name not in _REF:
        r = radiance(CASES[name][0])
        r.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def put_pixels(xyz):
    """cgo_put_pixel of every pixel of a float32[..., 3 or 4] array, as uint32[...]."""
    lib = oracle.load()
    flat = np.ascontiguousarray(xyz, np.float32).reshape(-1, xyz.shape[-1])
    out = np.empty(len(flat), np.uint32)
    for k, p in enumerate(flat):
        out[k] = lib.cgo_put_pixel(oracle.V3(float(p[0]), float(p[1]), float(p[2])))
    return out.reshape(xyz.shape[:-1])
