"""GPU: shadow masks per object of the one-light lattice kernel (cg_internal.h kObjSlots;
rt_tile_cert_kernel's phase 3, lattice_body's pass 2).  A tile with several primary
candidates gets one shadow mask per candidate, certified over that candidate's own box of hit
positions, and each 64-point chunk of the lattice kernel walks the masks of the objects its
points hit instead of the tile's union mask.  The shadow test is an any-hit search and every
mask is a certificate for all the hits on its object, so the frame must stay the reference's
bit for bit (integer ARGB: the tolerance is 0) with the masks on and with CG_OBJ_MASKS=0 (the
union mask, as before).  The diagnostic export (cg_rt_tile_masks) gives the masks' structure.
Reference: raytracer/Source/skeleton.cpp:104-169, :366-415."""
import ctypes as C
import os

import numpy as np
import pytest

import cgamd
import oracle

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 4)


def _moved_sphere():
    """The scene's sphere set down just above the floor (y = 1), under the light: the tiles
    around its foot hold sphere hits and floor hits the sphere shadows."""
    _, _, s = cgamd.rt_scene()
    r = 0.15
    s.radius, s.radiusSquared = r, np.float32(r) * np.float32(r)
    s.centre = cgamd.Vec3(0.3, 0.84, -0.6)
    return s


# name: (W, H, focal, cameraPos, yaw or None, scene); scene None = LoadTestModel, "sphere" = the
# sphere moved, (n, seed) = n seeded random triangles (no sphere)
CASES = {
    # one super-tile (4 x 4 tiles): the box, both blocks and the sphere in few tiles -- more
    # primary candidates than slots, so the candidates past the last slot take the union mask
    "one_super_tile": (64, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None, None),
    # right and bottom tiles cut, partial super-tiles
    "cut_80x75": (80, 75, 75.0, (0.0, 0.0, -3.0, 1.0), None, None),
    "cut_70x50": (70, 50, 50.0, (0.0, 0.0, -3.0, 1.0), None, None),
    # zoomed (focal 8 x the height) at the short block's foot over the floor: tiles of two or
    # three objects with a shadow boundary
    "zoom": (64, 60, 480.0, (0.3, 0.9, -3.0, 1.0), None, None),
    "zoom_yaw": (64, 60, 480.0, (-0.2, 0.9, -3.0, 1.0), 0.1745, None),
    "zoom_dolly": (64, 60, 480.0, (0.3, 0.9, float(np.float32(-3.0 + 0.005)), 1.0), None, None),
    # the sphere both hit and blocking within one tile
    "sphere": (64, 60, 240.0, (0.3, 0.85, -3.0, 1.0), None, "sphere"),
    "random20": (96, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None, (20, 0x5EED)),
    "random41": (96, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None, (41, 7)),
    "random60": (96, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None, (60, 12345)),
    # masks with bit 31 set and nothing above it (a mask's halves travel as two 32-bit words)
    "random33": (96, 60, 60.0, (0.0, 0.0, -3.0, 1.0), None, (33, 99)),
}

_REF = {}


def _scene(case):
    """(tris, n, sphere or None) of a case, product-side."""
    sc = CASES[case][5]
    if isinstance(sc, tuple):
        return cgamd.random_scene(*sc), sc[0], None
    tris, n, sph = cgamd.rt_scene()
    return tris, n, (_moved_sphere() if sc == "sphere" else sph)


def _reference(case):
    """The CPU oracle's frame of a case, computed once."""
    if case not in _REF:
        W, H, f, pos, yaw, _ = CASES[case]
        tris, n, sph = _scene(case)
        R = list(cgamd.yaw_matrix(yaw)) if yaw is not None else None
        otris = (oracle.RtTri * len(tris)).from_buffer_copy(tris)
        osph = C.pointer(oracle.Sphere.from_buffer_copy(sph)) if sph is not None else None
        _REF[case] = oracle.rt_draw(oracle.rt_params(W, H, f, pos, R), threads=THREADS,
                                    scene=(otris, n, osph, 1 if sph is not None else 0))
    return _REF[case]


def _camera(case):
    W, H, f, pos, yaw, _ = CASES[case]
    return cgamd.rt_camera(W, H, f, pos, cgamd.yaw_matrix(yaw) if yaw is not None else None)


@pytest.fixture
def scene_of(ctx):
    """Sets a case's scene; LoadTestModel is back afterwards (the session's context is shared)."""
    def set_scene(case):
        tris, n, sph = _scene(case)
        ctx.rt_set_scene(tris, n, sph, 1)
        return ctx
    yield set_scene
    tris, n, sph = cgamd.rt_scene()
    ctx.rt_set_scene(tris, n, sph, 1)


@pytest.mark.parametrize("knob", ["on", "off"])
@pytest.mark.parametrize("case", list(CASES))
def test_objmask_frame_matches_oracle(scene_of, monkeypatch, case, knob):
    """The frame == the CPU oracle's, every pixel, with the masks per object and with the union
    mask; with them, the masks' structure through the diagnostic export."""
    if knob == "off":
        monkeypatch.setenv("CG_OBJ_MASKS", "0")
    else:
        monkeypatch.delenv("CG_OBJ_MASKS", raising=False)
    ctx = scene_of(case)
    argb, _ = ctx.rt_render(_camera(case))
    ref = _reference(case)
    bad = np.flatnonzero(argb != ref)
    assert bad.size == 0, f"{case}/{knob}: {bad.size} pixels differ, first {bad[:8]}"
    masks, obj = ctx.rt_tile_masks(0)
    W, H = CASES[case][:2]
    # (the frame's rows are rounded up to whole stripes: the last tile row may lie below the frame)
    assert masks.shape[1] == (W + 15) // 16 and masks.shape[0] >= (H + 14) // 15
    if knob == "off":
        assert obj is None
        return
    _check_structure(case, masks, obj)


def _check_structure(case, masks, obj):
    slots = obj.shape[2]
    ntri = slots - 1
    pm, um = masks[..., 0], masks[..., 1]
    multi = 0
    narrowed = 0
    for (ty, tx), p in np.ndenumerate(pm):
        p, u = int(p), int(um[ty, tx])
        o = [int(v) for v in obj[ty, tx]]
        cand = bin(p & ~(3 << 62)).count("1")
        sphere = (p >> 63) & 1
        where = f"{case}: tile ({tx}, {ty}) primary {p:#x} shadow {u:#x} slots {[hex(v) for v in o]}"
        # every mask a subset of the tile's union mask
        assert all(v & ~u == 0 for v in o), where
        # slots of objects outside the primary mask are zero
        assert all(o[j] == 0 for j in range(min(cand, ntri), ntri)), where
        assert sphere or o[ntri] == 0, where
        # a tile of one candidate carries the union mask
        if cand + sphere == 1:
            assert (o[ntri] if sphere else o[0]) == u, where
        if cand + sphere > 1:
            multi += 1
            narrowed += any(v != u for v in o[:min(cand, ntri)] + ([o[ntri]] if sphere else []))
    print(f"{case}: {pm.size} tiles, {multi} with several candidates, {narrowed} with a mask narrower than the union; "
          f"candidates per tile (histogram) {np.bincount([bin(int(p) & ~(1 << 62)).count('1') for p in pm.ravel()]).tolist()}")
    assert multi > 0, f"{case}: no tile has several primary candidates"


def test_objmask_more_candidates_than_slots(scene_of):
    """The one-super-tile frame has tiles with more triangle candidates than slots: those past
    the last slot have no mask of their own (the lattice kernel gives them the union mask)."""
    ctx = scene_of("one_super_tile")
    ctx.rt_render(_camera("one_super_tile"))
    masks, obj = ctx.rt_tile_masks(0)
    cand = [bin(int(p) & ~(3 << 62)).count("1") for p in masks[..., 0].ravel()]
    assert max(cand) > obj.shape[2] - 1, cand


@pytest.mark.parametrize("knob", ["on", "off"])
def test_objmask_batched_call(scene_of, monkeypatch, knob):
    """The batched call (the pipelined certificate slots): the zoomed frame and its dolly step
    in one call, each == the oracle's frame; the export gives each frame's masks."""
    if knob == "off":
        monkeypatch.setenv("CG_OBJ_MASKS", "0")
    else:
        monkeypatch.delenv("CG_OBJ_MASKS", raising=False)
    ctx = scene_of("zoom")
    names = ["zoom", "zoom_dolly", "zoom"]
    import torch
    W, H = CASES["zoom"][:2]
    stride = W * ((H + 7) // 8 * 8)   # device frames hold whole 8-row stripes
    out = torch.zeros(len(names) * stride, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ctx.rt_render_frames_device([_camera(c) for c in names], out.data_ptr(), None, s.cuda_stream, frame_stride=stride)
    s.synchronize()
    frames = out.cpu().numpy().view(np.uint32).reshape(len(names), stride)[:, :W * H]
    for k, c in enumerate(names):
        assert np.array_equal(frames[k], _reference(c)), f"{knob}: frame {k} ({c})"
    if knob == "on":
        for k, c in enumerate(names):
            masks, obj = ctx.rt_tile_masks(k)
            _check_structure(c, masks, obj)
