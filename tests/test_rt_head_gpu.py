"""GPU: the head of a one-light lattice workgroup (cg_rt.hip lattice_body).  The shading table
is loaded and its barrier taken after the first closest-hit step (pitch 33: the wave's only
step; pitch 48: the first step peeled), a tile whose primary mask is empty leaves as soon as its
masks are in registers, and a single rank's tile rows come without shard_row's division.  No
float operation of any ray changes, so every frame must equal the CPU oracle's, every pixel
(integer ARGB: tolerance 0).  The shapes are the smallest at which the head can go wrong: tiles
cut by the right and bottom edge; a 16 x 1 frame, two of whose four waves have no point and
must still reach the barrier; the same under a yaw; a frame several tile columns wider than the
scene's box (windowed launches: black tiles, the edge workgroups' black columns, the RGB24
window); two and three ranks with tile rows at stripe boundaries (shard_row's general form) and
a band with row0 > 0 (the single-rank form); changes of frame size, shard and format on one
context and the same geometry on two; the measured dispatch orders; a batched dolly; a sequence
whose light moves and changes colour; LoadTestModel and the blocks alone with and without
per-object masks; published certificates and the uncertified path, which builds its own table.
Every frame has hit, missed and shadowed pixels by the oracle.
Reference: raytracer/Source/skeleton.cpp:104-169, :366-415."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cgamd
import cgdist
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, os.cpu_count() or 4)
YAW = 0.1745
LIGHT_POS = (0.0, -0.5, -0.7, 1.0)
LOW_LIGHT = (-0.9, 0.0, 0.8, 1.0)   # behind the tall block: the central row of the room has shadows
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
    # ten tile columns, the scene's box in the middle four: black tiles on both sides
    "wide_160x45": (160, 45, 45.0, (0.0, 0.0, -3.0, 1.0), None),
    "wide_160x45_dolly": (160, 45, 45.0, (0.0, 0.0, float(np.float32(-3.0 + 0.005)), 1.0), None),
    "64x60": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None),
    "64x60_dolly": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.005)), 1.0), None),
    "64x60_dolly2": (64, 60, 60.0, (0.0, 0.0, float(np.float32(-3.0 + 0.010)), 1.0), None),
    "48x45": (48, 45, 90.0, (0.1, 0.3, -3.0, 1.0), None),
}
DOLLY = ["64x60", "64x60_dolly", "64x60_dolly2"]
# the light of each frame of the sequence: a plain one, one with a negative channel, one whose
# zero channels make the unequal red and blue of every object's colour * lc equal
MOVING = ((LIGHT_POS, WHITE), ((0.3, -0.5, -0.7, 1.0), (-3.0, 14.0, 5.0)), ((-0.3, -0.4, -0.9, 1.0), (0.0, 14.0, 0.0)))

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


def _content(scene, cam, pos=LIGHT_POS, colour=WHITE):
    """The case is not vacuous: by the oracle the frame has pixels that missed, lit pixels, and
    pixels in shadow -- hit pixels whose value is the one a black light gives, every sub-ray's
    DirectLight zero.  Returns the oracle's frame."""
    ref, unlit = _reference(scene, cam, pos, colour), _reference(scene, cam, pos, (0.0, 0.0, 0.0))
    missed = int((ref == BLACK_PIXEL).sum())
    shadowed = int(((ref == unlit) & (ref != BLACK_PIXEL)).sum())
    lit = int((ref != unlit).sum())
    assert missed > 0 and shadowed > 0 and lit > 0, f"{scene}/{cam}: {missed} missed, {shadowed} in shadow, {lit} lit"
    return ref


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
        ctx.rt_set_scene(tris, n, sph, 1)
        return ctx
    yield set_scene
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)


def _same(got, ref, what):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(ref).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first {bad[:8]}"


def _frames(ctx, names, shard=None, fmt=None, lights=None, rows=None, cols=None):
    """One cg_rt_render_frames_device call: per frame the shard's rows x cols pixels (uint32) or
    wire bytes (RGB24)."""
    import torch
    W, H = CAMERAS[names[0]][:2]
    rows, cols = rows or H, cols or W
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
        return raw[:len(names) * stride * 4].view(np.uint32).reshape(len(names), stride)[:, :rows * cols]
    return raw[:len(names) * rows * cols * 3].reshape(len(names), rows * cols * 3)


@pytest.mark.parametrize("cam", ["cut_40x37", "idle_16x1", "cut_40x37_yaw", "idle_16x1_yaw"])
def test_head_cut_tiles_and_empty_waves(scene_of, cam):
    """Tiles cut by the right and the bottom edge, and a tile of 99 points two of whose waves
    only reach the barrier, with shared and with per-pixel columns."""
    pos = LOW_LIGHT if cam.startswith("idle") else LIGHT_POS
    ref = _content("test_model", cam, pos)
    _on_lattice("test_model", cam)
    argb, _ = scene_of("test_model").rt_render(_camera(cam), lights=_lights(pos))
    _same(argb, ref, cam)


@pytest.mark.parametrize("fmt", ["argb", "rgb24_window"])
def test_head_windowed_launch(scene_of, fmt):
    """A frame of ten tile columns with the scene's box in the middle: the batch's launch covers
    the window's tile columns only, tiles beside the box inside it are black by their masks, and
    the edge workgroups store the columns outside; RGB24 over the output window of the columns
    anything can be seen in."""
    ctx = scene_of("test_model")
    names = ["wide_160x45", "wide_160x45_dolly"]
    W, H = CAMERAS[names[0]][:2]
    refs = [_content("test_model", c) for c in names]
    tris, n, sph = cgamd.rt_scene()
    c0, c1 = cgamd.frame_columns(tris, n, sph, 1, _camera(names[0]))
    assert 0 < c0 and c1 < W and (c1 - c0) <= W - 4 * 16, (c0, c1)   # black tile columns on both sides
    for ref in refs:
        outside = np.concatenate([ref.reshape(H, W)[:, :c0].ravel(), ref.reshape(H, W)[:, c1:].ravel()])
        assert (outside == BLACK_PIXEL).all()
    if fmt == "argb":
        got = _frames(ctx, names)
        for k, ref in enumerate(refs):
            _same(got[k], ref, f"frame {k}")
        return
    sh = cgamd.RtShard(row0=0, rows=H, col0=c0, cols=c1 - c0)
    got = _frames(ctx, names, sh, cgamd.PIX_RGB24, cols=c1 - c0)
    for k, ref in enumerate(refs):
        _same(got[k], cgdist.pack_rgb24_np(cgdist.window_np(ref, W, c0, c1 - c0)), f"frame {k}")


@pytest.mark.parametrize("nranks", [2, 3])
def test_head_stripes_on_tile_rows(scene_of, nranks):
    """Stripes of the tile height over 60 rows: every tile row starts a stripe, a rank's local
    rows map through shard_row's general form, and three ranks leave the last rank a stripe short."""
    ctx = scene_of("test_model")
    W, H = CAMERAS["64x60"][:2]
    S = cgdist.LATTICE_STRIPE
    refs = [_content("test_model", c) for c in DOLLY]
    rows = cgdist.shard_rows(H, nranks, S)
    parts = []
    for r in range(nranks):
        sh = cgamd.RtShard(r, nranks, S)
        _on_lattice("test_model", "64x60", sh)
        parts.append(_frames(ctx, DOLLY, sh, rows=rows))
    for k, ref in enumerate(refs):
        frame = cgdist.unstripe_np(np.stack([p[k] for p in parts]).reshape(nranks, rows, W), H, nranks, S)
        _same(frame, ref, f"{nranks} ranks, frame {k}")


def test_head_band_from_row_15(scene_of):
    """A band with row0 > 0 (one rank: rows row0 + L, no division), ARGB and RGB24."""
    ctx = scene_of("test_model")
    W = CAMERAS["64x60"][0]
    refs = [_content("test_model", c) for c in DOLLY]
    band = cgamd.RtShard(row0=15, rows=30)
    got = _frames(ctx, DOLLY, band, rows=30)
    wire = _frames(ctx, DOLLY, band, cgamd.PIX_RGB24, rows=30)
    for k, ref in enumerate(refs):
        _same(got[k], ref[15 * W:45 * W], f"frame {k}")
        _same(wire[k], cgdist.pack_rgb24_np(ref[15 * W:45 * W]), f"frame {k} RGB24")


def test_head_geometry_changes_on_one_context(scene_of):
    """Frame size, shard and output format change from call to call on one context and change
    back; the same geometry on a second context.  Nothing a call reads may be left over from
    another geometry."""
    ctx = scene_of("test_model")
    W = CAMERAS["64x60"][0]
    ref = _content("test_model", "64x60")
    small = _content("test_model", "cut_40x37")
    for _ in range(2):
        _same(_frames(ctx, ["64x60"])[0], ref, "64x60")
        _same(_frames(ctx, ["cut_40x37"])[0], small, "40x37")
        _same(_frames(ctx, ["64x60"], cgamd.RtShard(row0=30, rows=30), rows=30)[0], ref[30 * W:], "band")
        _same(_frames(ctx, ["64x60"], cgamd.RtShard(row0=0, rows=60), cgamd.PIX_RGB24)[0],
              cgdist.pack_rgb24_np(ref), "RGB24")
        _same(_frames(ctx, ["64x60"], cgamd.RtShard(1, 2, cgdist.LATTICE_STRIPE), rows=30)[0],
              np.concatenate([ref[15 * W:30 * W], ref[45 * W:]]), "rank 1 of 2")
    with cgamd.Context(0) as other:
        tris, n, sph = cgamd.rt_scene()
        other.rt_set_scene(tris, n, sph, 1)
        _same(_frames(other, ["64x60"])[0], ref, "second context")
        _same(_frames(ctx, ["64x60"])[0], ref, "first context again")


_ORDER_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path[:0] = [os.path.join(os.environ["CG_ROOT"], "computer-graphics_amd")]
import cgamd
W, H, F = 64, 60, 60.0
ctx = cgamd.Context(0)
tris, n, sph = cgamd.rt_scene()
ctx.rt_set_scene(tris, n, sph, 1)
cams = [cgamd.rt_camera(W, H, F, (0.0, 0.0, float(np.float32(-3.0 + 0.005 * k)), 1.0)) for k in range(3)]
sh = cgamd.RtShard(row0=15, rows=30)
out = []
buf = torch.zeros(3 * W * 64, dtype=torch.int32, device="cuda")
for call in range(3):   # call 1 records, later calls take the sorted order
    buf.zero_()
    ctx.rt_render_frames_device(cams, buf.data_ptr(), sh, None, frame_stride=W * 64)
    torch.cuda.synchronize()
    out.append(buf.cpu().numpy().view(np.uint32).reshape(3, W * 64)[:, :30 * W].tolist())
print("RESULT " + json.dumps({"frames": out, "order": ctx.rt_lattice_path()[0]}))
"""


@pytest.mark.parametrize("mode", ["2", "1", "0"])
def test_head_measured_order_band(mode):
    """A band-sized call repeated on one context under each dispatch order (CG_LAT_ORDER is read
    once per process: a child process per mode): the workgroup's tile is the one its dispatch
    slot names, whatever the order."""
    W = CAMERAS["64x60"][0]
    refs = [_content("test_model", c) for c in DOLLY]
    env = dict(os.environ, CG_ROOT=ROOT, CG_LAT_ORDER=mode)
    r = subprocess.run([sys.executable, "-c", _ORDER_CHILD], capture_output=True, text=True, timeout=100, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and lines, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    res = json.loads(lines[-1][7:])
    assert res["order"] == int(mode)
    for c, frames in enumerate(res["frames"]):
        for k, ref in enumerate(refs):
            _same(np.array(frames[k], np.uint32), ref[15 * W:45 * W], f"order {mode}, call {c}, frame {k}")


def test_head_batched_dolly(scene_of):
    """Three frames of a dolly in one call: the geometry is shared, the masks are per frame."""
    ctx = scene_of("test_model")
    got = _frames(ctx, DOLLY)
    for k, c in enumerate(DOLLY):
        _same(got[k], _content("test_model", c), f"frame {k} ({c})")


def test_head_sequence_light_moves_and_changes_colour(scene_of):
    """One cg_rt_render_sequence_device call of three frames, each with its own light: position
    and colour, one colour with a negative channel, one that makes unequal products equal."""
    import torch
    ctx = scene_of("test_model")
    W, H = CAMERAS["64x60"][:2]
    stride = W * ((H + 7) // 8 * 8)
    out = torch.zeros(len(MOVING) * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_sequence_device([_camera("64x60")] * len(MOVING), [_lights(p, c) for p, c in MOVING], out.data_ptr(),
                                  None, s.cuda_stream, frame_stride=stride)
    s.synchronize()
    got = out.cpu().numpy().view(np.uint32).reshape(len(MOVING), stride)[:, :W * H]
    for k, (pos, colour) in enumerate(MOVING):
        _same(got[k], _content("test_model", "64x60", pos, colour), f"frame {k} (light {pos}, {colour})")


@pytest.mark.parametrize("knob", ["on", "off"])
@pytest.mark.parametrize("scene,cam", [("test_model", "64x60"), ("blocks", "48x45")])
def test_head_objects(scene_of, monkeypatch, scene, cam, knob):
    """LoadTestModel with its sphere and the blocks alone (misses beside hits inside a chunk),
    the shadow masks per object and (CG_OBJ_MASKS=0) per tile."""
    if knob == "off":
        monkeypatch.setenv("CG_OBJ_MASKS", "0")
    else:
        monkeypatch.delenv("CG_OBJ_MASKS", raising=False)
    ref = _content(scene, cam)
    _on_lattice(scene, cam)
    argb, _ = scene_of(scene).rt_render(_camera(cam), lights=_lights())
    _same(argb, ref, f"{scene}/{cam}, object masks {knob}")


_CERT_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path[:0] = [os.path.join(os.environ["CG_ROOT"], "computer-graphics_amd")]
import cgamd
W, H, F = 64, 60, 60.0
ctx = cgamd.Context(0)
tris, n, sph = cgamd.rt_scene()
ctx.rt_set_scene(tris, n, sph, 1)
cams = [cgamd.rt_camera(W, H, F, (0.0, 0.0, float(np.float32(-3.0 + 0.005 * k)), 1.0)) for k in range(3)]
out, paths = [], []
buf = torch.zeros(3 * W * 64, dtype=torch.int32, device="cuda")
for call in range(2):   # both certificate slots
    buf.zero_()
    ctx.rt_render_frames_device(cams, buf.data_ptr(), None, None, frame_stride=W * 64)
    torch.cuda.synchronize()
    paths.append(list(ctx.rt_lattice_path()))
    out.append(buf.cpu().numpy().view(np.uint32).reshape(3, W * 64)[:, :H * W].tolist())
print("RESULT " + json.dumps({"paths": paths, "frames": out}))
"""


@pytest.mark.parametrize("mode", ["published", "uncertified"])
def test_head_published_certificates(mode):
    """CG_CERT_CONC=1 on whole-frame calls in the default order (CG_LAT_ORDER=0, read once per
    process: a child process per mode -- a call small enough for a measured order keeps its
    certificates first): the lattice workgroups wait for their super-tile's certificates or, with
    CG_LAT_FORCE_UNCERT=1, take the uncertified path, whose workgroups store the frame's RtTri and
    load the table themselves, with two more barriers ahead of the table's.  cg_rt_lattice_path
    says that the call was launched that way."""
    refs = [_content("test_model", c) for c in DOLLY]
    env = dict(os.environ, CG_ROOT=ROOT, CG_LAT_ORDER="0", CG_CERT_CONC="1")
    env.pop("CG_LAT_FORCE_UNCERT", None)
    env.pop("CG_LAT_SPIN", None)
    if mode == "uncertified":
        env["CG_LAT_FORCE_UNCERT"] = "1"
    r = subprocess.run([sys.executable, "-c", _CERT_CHILD], capture_output=True, text=True, timeout=100, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and lines, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    res = json.loads(lines[-1][7:])
    tiles = 4 * 5 * len(DOLLY)   # four tile columns; the device frame's 64 rows (whole 8-row stripes) are five tile rows
    for call, frames in enumerate(res["frames"]):
        order, published, forced, wgs = res["paths"][call]
        assert (order, published, forced) == (0, 1, int(mode == "uncertified")), f"{mode}, call {call}: {res['paths'][call]}"
        assert 0 < wgs <= tiles
        for k, ref in enumerate(refs):
            _same(np.array(frames[k], np.uint32), ref, f"{mode}, call {call}, frame {k}")
