"""Caller-supplied scenes for the reference programs' scene-loading builds: every scene of
tests/golden/ref_scene_sessions.json, built deterministically from the library's host-only
generators or numpy.  No scene file is committed: the recording script
(tests/golden/make_ref_scene_sessions.py) and the tests both call scene(name) and compare the
SHA-256 of scene_bytes(...), the file the reference binary was given.

Normals: the reference's constructor computes every normal itself (ComputeNormal), so a scene
only pins anything if its records hold those very bits.  The generators' normals are the
reference's; triangles edited here get reference_normals(), numpy's float32 restatement of
ComputeNormal.  The recording script compares every normal with the ones the reference binary
dumped, as bits, NaN payloads included.

Keys as the reference's Update() reads them: U D L R camera z / x, n m yaw, w s a d q e light;
raytracer i o focal length; rasteriser f g focal length, z x camera y, 1 2 indirect term, SPACE
colour mode; '.' a frame without a key."""
import ctypes as C
import functools

import numpy as np

import cgamd

f32 = np.float32
TRI = np.dtype([("v", "<f4", (3, 4)), ("normal", "<f4", 4), ("color", "<f4", 3)])
RTRI = np.dtype([("v", "<f4", (3, 4)), ("normal", "<f4", 4), ("color", "<f4", 3), ("texture", "<i4"), ("index", "<i4")])
assert TRI.itemsize == 76 and RTRI.itemsize == 84


def reference_normals(v):
    """ComputeNormal (TestModelH.h) for vertices v (n, 3, 4) float32 -> (n, 4): e1 = v1 - v0,
    e2 = v2 - v0, glm::cross(e2, e1), glm::normalize = v * (1 / sqrt(dot)), w = 1.  Every
    operation a float32 one in glm's order; a zero-area triangle gives NaN as the hardware does."""
    v = np.asarray(v, f32)
    e1, e2 = v[:, 1, :3] - v[:, 0, :3], v[:, 2, :3] - v[:, 0, :3]
    x, y = e2, e1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2],
                      x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0],
                      x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], 1).astype(f32)
        d = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        inv = f32(1.0) / np.sqrt(d, dtype=f32)
        n = np.ones((len(v), 4), f32)
        n[:, :3] = c * inv[:, None]
    return n


def _np(arr, n, dtype):
    return np.frombuffer(C.string_at(C.addressof(arr), n * dtype.itemsize), dtype).copy() if n else np.zeros(0, dtype)


# ---- raytracer ---------------------------------------------------------------------------------
SPHERE = np.dtype([("centre", "<f4", 3), ("radius", "<f4"), ("color", "<f4", 3)])


def _room_sphere():
    _, _, s = cgamd.rt_scene()
    return np.array([((s.centre.x, s.centre.y, s.centre.z), s.radius, (s.color.x, s.color.y, s.color.z))], SPHERE)


def _cloud(n):
    return _np(cgamd.random_scene(n, 0x5EED), n, TRI)


def _degenerate(n, around_eye):
    """test_rt_big_gpu._degenerate_scene's edits, with the normals of the edited triangles as the
    reference computes them."""
    from test_rt_big_gpu import _degenerate_scene
    t = _np(_degenerate_scene(n, around_eye)[0], n, TRI)
    t["normal"][1:9] = reference_normals(t["v"][1:9])
    return t


def _three_spheres():
    from test_rt_gpu import _three_spheres as three
    return np.array([((s.centre.x, s.centre.y, s.centre.z), s.radius, (s.color.x, s.color.y, s.color.z))
                     for s in three()], SPHERE)


def _room():
    tris, n, _ = cgamd.rt_scene()
    return _np(tris, n, TRI)


def _one_triangle():
    t = np.zeros(1, TRI)
    t["v"][0] = [[-0.6, 0.5, 0.2, 1.0], [0.7, 0.4, -0.1, 1.0], [0.1, -0.7, 0.4, 1.0]]
    t["color"][0] = (0.75, 0.45, 0.15)
    t["normal"] = reference_normals(t["v"])
    return t


NO_SPHERES = np.zeros(0, SPHERE)


def _eyes():
    from test_rt_big_gpu import EYE_IN, EYE_V0
    return EYE_IN[:3], EYE_V0[:3]


# name: (scene builder, spheres builder, session spec).  route: what cg_rt_route must report for
# the session's unrotated / yawed frames.  Sessions of the 300-triangle scenes cost the reference
# about 2 s a frame: at most 8 frames each.
RT_CASES = {
    # the large-scene path: unrotated, yawed (m), light moved (w, a), focal length (i), back to
    # the tiny yaw (n) and on to the other side (n)
    "rt_cloud300": dict(tris=lambda: _cloud(300), keys="Umwinnao", routes=("big_lattice", "big_lattice_yaw")),
    # the eye inside the first triangle's span / the eye plane exactly through its vertex v0
    "rt_cloud300_eye_in": dict(tris=lambda: _cloud(300), keys=".mnd", cam=lambda: _eyes()[0],
                               routes=("big_lattice", "big_lattice_yaw")),
    "rt_cloud300_eye_v0": dict(tris=lambda: _cloud(300), keys=".mnq", cam=lambda: _eyes()[1],
                               routes=("big_lattice", "big_lattice_yaw")),
    "rt_cloud300_sphere": dict(tris=lambda: _cloud(300), spheres=_room_sphere, keys="Lmei",
                               routes=("big_lattice", "big_lattice_yaw")),
    "rt_degenerate40": dict(tris=lambda: _degenerate(40, False), keys=".mnUio", routes=("lattice", "lattice_yaw")),
    "rt_degenerate40_around_eye": dict(tris=lambda: _degenerate(40, True), keys=".mnUsi",
                                       routes=("lattice", "lattice_yaw")),
    "rt_degenerate300": dict(tris=lambda: _degenerate(300, False), keys=".mUa",
                             routes=("big_lattice", "big_lattice_yaw")),
    "rt_degenerate300_around_eye": dict(tris=lambda: _degenerate(300, True), keys=".mUw",
                                        routes=("big_lattice", "big_lattice_yaw")),
    "rt_room_three_spheres": dict(tris=_room, spheres=_three_spheres, keys="Umwion",
                                  routes=("lattice", "lattice_yaw")),
    "rt_empty": dict(tris=lambda: np.zeros(0, TRI), keys=".m", routes=("pixel", "pixel")),     # nothing to tile
    # start values for the light and the focal length too
    "rt_one_triangle": dict(tris=_one_triangle, keys=".mUw", light=(0.2, -0.6, -0.9), focal=200.0,
                            routes=("lattice", "lattice_yaw")),
}


# ---- rasteriser --------------------------------------------------------------------------------
def _mesh(n, extent, seed):
    return _np(cgamd.rast_random_scene(n, extent, seed), n, RTRI)


NO_TRIS = np.zeros(0, RTRI)
DEGENERATE_FOCAL = 512.0          # the rasteriser's start value: the side-plane vertex is exact for it


def _rast_degenerate():
    """A mesh in front of a camera at the origin (so camera space is scene space in the first
    frames, and after 'm' 'n' for a vertex with x = 0): 120 ordinary triangles around z = 2 and
    seven edge cases written over the first ones."""
    t = _mesh(120, 0.25, 0xDE6E)
    t["v"][:, :, 2] += f32(2.0)
    v = t["v"]
    v[1, 1], v[1, 2] = v[1, 0], v[1, 0]                                         # a point
    v[2, 2, :3] = v[2, 0, :3] + f32(2) * (v[2, 1, :3] - v[2, 0, :3])           # collinear
    v[3, 1] = v[3, 0]                                                          # a repeated vertex
    v[4, 2, :3] = v[4, 1, :3] + f32(1e-6)                                      # a sliver
    v[5, :, :3] = [[0.0, 0.0, 0.01], [0.3, 0.1, 0.8], [-0.2, 0.25, 0.9]]       # v0 at z = 0.01f exactly
    # v0 exactly on the left plane: x = (z / f) * -W / 2 with z = 2, f = 512, W = 900, all exact
    v[6, :, :3] = [[-1.7578125, 0.2, 2.0], [-0.9, 0.1, 2.0], [-1.2, 0.6, 2.2]]
    v[7, :, :3] = [[-1.0, -1.0, -1.0], [1.0, -1.0, -1.5], [0.0, 1.0, -2.0]]   # wholly behind the camera
    t["normal"] = reference_normals(v)
    return t


def _indexed(t, first=0):
    """Every record's index names an object of the reference's (0-4), so no field is arbitrary."""
    t["index"] = (np.arange(len(t)) + first) % 5
    return t


RAST_CASES = {
    "rast_mesh3000": dict(room=lambda: _indexed(_mesh(3000, 0.15, 0x5EED)), boxes=lambda: _mesh(60, 0.1, 0xB0C5),
                          keys="Umn Rx  d"),
    "rast_subpixel20000": dict(room=lambda: _mesh(20000, 0.004, 0x51B), boxes=lambda: NO_TRIS, keys="mUn  zL "),
    # triangles as large as the frustum around a camera inside the mesh: every clip case on every
    # plane (the shadow volumes reach beyond the far plane, w = 5 / focal)
    "rast_clip400": dict(room=lambda: _mesh(400, 1.5, 0xC11B), boxes=lambda: _mesh(20, 0.5, 0xC11C),
                         keys="DDmn gDx  R", cam=(0.0, 0.0, -1.0)),
    "rast_boxes700": dict(room=lambda: NO_TRIS, boxes=lambda: _mesh(700, 0.1, 0xB0C5), keys="Um nz  a"),
    "rast_degenerate": dict(room=_rast_degenerate, boxes=lambda: NO_TRIS, keys=".mn U x  ", cam=(0.0, 0.0, 0.0)),
    "rast_empty_room_boxes": dict(room=lambda: NO_TRIS, boxes=lambda: _mesh(30, 0.2, 0xE0B), keys="mn U  x",
                                  light=(0.3, -0.4, 0.2), focal=400.0),
    "rast_empty": dict(room=lambda: NO_TRIS, boxes=lambda: NO_TRIS, keys="m n U "),
}
EMPTY = ("rt_empty", "rast_empty")

CASES = {**{k: dict(v, program="raytracer") for k, v in RT_CASES.items()},
         **{k: dict(v, program="rasteriser") for k, v in RAST_CASES.items()}}


def spec(name):
    """The JSON-able part of a case: program, keys and start values."""
    c = CASES[name]
    out = dict(program=c["program"], keys=c["keys"])
    for key in ("cam", "light"):
        if key in c:
            v = c[key]() if callable(c[key]) else c[key]
            out[key] = [float(f32(x)) for x in v]
    if "focal" in c:
        out["focal"] = float(f32(c["focal"]))
    return out


@functools.lru_cache(maxsize=None)
def scene(name):
    """Raytracer: (TRI records, SPHERE records); rasteriser: (room RTRI records, boxes RTRI records)."""
    c = CASES[name]
    if c["program"] == "raytracer":
        out = c["tris"](), c.get("spheres", lambda: NO_SPHERES)()
    else:
        out = c["room"](), c["boxes"]()
    for a in out:
        a.setflags(write=False)
    return out


def scene_bytes(name):
    """The file CG_REF_SCENE names: two int32 counts, then the records."""
    a, b = scene(name)
    return np.array([len(a), len(b)], "<i4").tobytes() + a.tobytes() + b.tobytes()


# ---- the scenes as library / oracle arguments --------------------------------------------------
def _ctypes(records, ctype):
    arr = (ctype * max(len(records), 1))()
    if len(records):
        C.memmove(arr, np.ascontiguousarray(records).ctypes.data, records.nbytes)
    return arr


def _spheres(records, ctype, v3):
    arr = (ctype * max(len(records), 1))()
    for k, s in enumerate(records):
        r = f32(s["radius"])
        arr[k].radius, arr[k].radiusSquared = float(r), float(r * r)      # Sphere's constructor: r * r
        arr[k].centre = v3(*[float(x) for x in s["centre"]])
        arr[k].color = v3(*[float(x) for x in s["color"]])
    return arr


def rt_library_scene(name):
    """(tris, n, spheres or None, n_spheres) for Context.rt_set_scene."""
    t, s = scene(name)
    return _ctypes(t, cgamd.Tri), len(t), (_spheres(s, cgamd.Sphere, cgamd.Vec3) if len(s) else None), len(s)


def rt_oracle_scene(name):
    """(tris, n, spheres or None, n_spheres) for oracle.rt_draw."""
    import oracle
    t, s = scene(name)
    return _ctypes(t, oracle.RtTri), len(t), (_spheres(s, oracle.Sphere, oracle.V3) if len(s) else None), len(s)


def rast_library_scene(name):
    """(room, n_room, boxes, n_boxes) for Context.rast_set_scene and cgamd.rast_prepare."""
    r, b = scene(name)
    return _ctypes(r, cgamd.RTri), len(r), _ctypes(b, cgamd.RTri), len(b)


def rast_oracle_scene(name):
    """(room, n_room, boxes, n_boxes) for oracle.rast_draw(scene=...)."""
    import oracle
    r, b = scene(name)
    return _ctypes(r, oracle.RastTri), len(r), _ctypes(b, oracle.RastTri), len(b)
