"""CPU: the ABI of the rasteriser's buffers calls (cg_rast_draw_buffers*, cg_rast_render_buffers*,
cg_rast_pick) and the checker the GPU tests lean on -- tests/rast_owner_ref.py's restatement of the
ordered z-buffer's owner rule, proved here against cgo_rast_draw on every pixel."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import oracle
import rast_owner_ref as ro
from test_rast_big_gpu import CAMERAS

CASES = [(96, 64, "unrotated"), (67, 45, "in_short_box"), (96, 64, "yawed")]


def case_params(W, H, camera, ind=0.2, colour_mode=0, rand_offset=0, setting=0, boxes=0):
    """(cgamd params, oracle params) of one camera of CAMERAS, as test_rast_big_gpu frames them."""
    cfg = CAMERAS[camera]
    F = 0.8 * W
    R = cgamd.yaw_matrix(cfg["yaw"]) if cfg["yaw"] else None
    p = cgamd.rast_params(W, H, F, cfg["cam"], R, indirect_first=ind, yaw=cfg["yaw"], colour_mode=colour_mode,
                          rand_offset=rand_offset)
    po = oracle.rast_params(W, H, F, cfg["cam"], list(R) if R is not None else None, indirect_first=ind,
                            colour_mode=colour_mode, rand_offset=rand_offset, setting=setting, setting_boxes=boxes,
                            yaw=cfg["yaw"])
    return p, po


def test_abi_and_layout():
    lib = cgamd.load()
    for name in ("cg_rast_draw_buffers_device", "cg_rast_draw_buffers", "cg_rast_render_buffers_device",
                 "cg_rast_render_buffers", "cg_rast_pick"):
        assert name in cgamd.EXPORTS and getattr(lib, name).restype is C.c_int
    B = cgamd.RastBuffers
    assert [f[0] for f in B._fields_] == ["argb", "depth", "shadow", "screen", "low", "high", "clip", "tri", "pos"]
    assert C.sizeof(B) == 9 * C.sizeof(C.c_void_p)
    assert [getattr(B, n).offset for n, _, _ in cgamd.RAST_PLANES] == [8 * k for k in range(9)]
    assert cgamd.RAST_OWNER_NONE == -1
    for fn in ("rast_draw_buffers", "rast_render_buffers", "rast_draw_buffers_device", "rast_render_buffers_device",
               "rast_pick"):
        assert callable(getattr(cgamd.Context, fn))
    # every pointer NULL, or no context: refused before any device work
    p = cgamd.rast_params(64, 48)
    assert lib.cg_rast_draw_buffers(None, C.byref(p), C.byref(B()), None) == cgamd.CG_E_INVALID
    assert lib.cg_rast_pick(None, C.byref(p), 0, 0, None, None, None, None) == cgamd.CG_E_INVALID


def test_plane_shapes():
    p = cgamd.rast_params(10, 7)
    b, out = cgamd.rast_buffers_planes(p, ("screen", "clip", "pos"))
    assert out["screen"].shape == (70, 3) and out["screen"].dtype == np.float32
    assert out["clip"].shape == (70,) and out["clip"].dtype == np.int32
    assert out["pos"].shape == (70, 4)
    assert b.screen == out["screen"].ctypes.data and b.pos == out["pos"].ctypes.data
    assert not b.argb and not b.low and not b.tri
    with pytest.raises(ValueError):
        cgamd.rast_buffers_planes(p, ("colour",))


@pytest.mark.parametrize("W,H,camera", CASES)
def test_restatement_equals_the_oracle(W, H, camera):
    """owner_planes' depth and shadow are cgo_rast_draw's on every pixel, bit for bit: the walk
    that names the owner is the oracle's own."""
    p, po = case_params(W, H, camera)
    tris, n, _ = oracle.rast_geometry(po)
    assert n > 150
    _, rd, rs = oracle.rast_draw(po)
    depth, shadow, clip, pos = ro.owner_planes(po, tris, n, W, H)
    assert np.array_equal(depth.view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(shadow, rs)
    owned = clip >= 0
    assert owned.any() and (clip < n).all()
    # an untextured owner is the depth's writer: pos.z = 1 / zinv, and no owner leaves pos at 0
    assert np.array_equal((np.float32(1) / depth[owned]).view(np.uint32), pos[owned, 2].view(np.uint32))
    assert not pos[~owned].any() and (pos[owned, 3] == 1).all()
    # the GPU's clipped list is the oracle's (cg_rast_prepare's order)
    ct, cn, _ = cgamd.rast_prepare(p)
    assert cn == n and C.string_at(ct, n * 84) == C.string_at(tris, n * 84)


@pytest.mark.parametrize("W,H,camera", CASES)
def test_input_counts_sum_to_the_clipped_total(W, H, camera):
    p, _ = case_params(W, H, camera)
    room, nr, boxes, nb = cgamd.rast_scene()
    _, n, _ = cgamd.rast_prepare(p, room, nr, boxes, nb)
    counts = ro.input_counts(p, room, nr, boxes, nb)
    assert counts.size == nr + nb and counts.sum() == n
    src = ro.input_of_clip(p, room, nr, boxes, nb)
    assert src.size == n and (np.diff(src) >= 0).all() and src.max() < nr + nb
