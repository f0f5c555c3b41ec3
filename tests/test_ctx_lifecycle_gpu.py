"""What a context holds is freed by cg_destroy: cg_debug_live's four counts (device allocations,
pinned allocations, events, streams) return to where they were once a context, whatever it ran,
is closed.  The session's shared context is alive throughout, so every test compares against
the counts it found at its start."""
import ctypes as C
import os

import numpy as np
import pytest

import cgamd

pytestmark = pytest.mark.gpu

TEX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textures")
W, H, F = 64, 48, 48.0          # the small frames of test_dist_gpu / test_rt_hits_gpu
IDLE = (0, 0, 2, 1)             # cg_create: the stream and the two timing events, nothing else
N_BIG = 500                     # random_scene(500): the large-scene route (> 64 triangles)


def _live():
    return cgamd.debug_live()


def _above(base):
    return tuple(a - b for a, b in zip(_live(), base))


def _jpeg(name):
    with open(os.path.join(TEX, name), "rb") as f:
        return f.read()


def _small_scene(c):
    tris, n, sph = cgamd.rt_scene()
    c.rt_set_scene(tris, n, sph, 1)
    return n


def _lattice_calls(c, torch):
    """Single lattice frames with one light and with a light set, then two batched calls."""
    n = _small_scene(c)
    cam = cgamd.rt_camera(W, H, F)
    area = cgamd.area_lights()
    assert cgamd.rt_route(cam, n, 1, 1) == "lattice" and cgamd.rt_route(cam, n, 1, len(area)) == "lights"
    c.rt_render(cam)            # latmask, supmask
    c.rt_render(cam, area)      # umask
    out = torch.zeros(2 * W * H, dtype=torch.int32, device="cuda")
    for _ in range(2):          # the second call finds the first one's recording
        c.rt_render_frames_device([cam, cam], out.data_ptr())
    assert c.rt_lattice_path()[0] != 0, "the batched call did not take the measured order"   # lcost, lflat
    torch.cuda.synchronize()
    return cam


def test_idle_contexts_leave_nothing():
    base = _live()
    for _ in range(50):
        c = cgamd.Context(0)
        assert _above(base) == IDLE
        c.close()
        assert _live() == base


def test_everything_touched_is_freed():
    import torch
    base = _live()
    c = cgamd.Context(0)
    try:
        # raytracer, small scene: lattice frames, a sequence, host output
        cam = _lattice_calls(c, torch)
        out = torch.zeros(2 * W * H, dtype=torch.int32, device="cuda")
        c.rt_render_sequence_device([cam, cam], [cgamd.default_lights()] * 2, out.data_ptr())
        c.rt_render_frames([cam] * 3, chunk=1)
        # large scene: two frames in flight, hit planes, a pick, the device grid builder
        big = cgamd.random_scene(N_BIG, 0x5EED)
        c.rt_set_scene(big, N_BIG, None, 0)
        assert cgamd.rt_route(cam, N_BIG, 0, 1).startswith("big")
        c.rt_render_frames_device([cam, cam], out.data_ptr())
        torch.cuda.synchronize()
        assert c.rt_scratch_info()["bytes"] > 0
        index = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        c.rt_hits_device(cam, d_index=index.data_ptr())
        c.rt_pick(cam, W // 2, H // 2)
        d_tris = torch.frombuffer(bytearray(bytes(big)), dtype=torch.uint8)[:N_BIG * C.sizeof(cgamd.Tri)].cuda()
        c.rt_set_scene_device(d_tris.data_ptr(), N_BIG)
        assert c.rt_grid_info()["candidates"] > 0, "the grid was not built on the device"
        # JPEG decode, textures, rasteriser: lanes, host sequence, a buffers call
        grill = {k: c.decode_jpeg(_jpeg(cgamd.TEXTURE_FILES[k])) for k in ("grill", "grill_opacity", "grill_normal")}
        c.rast_set_textures(grill)
        c.rast_set_scene(*cgamd.rast_scene(2, 0))
        p = cgamd.rast_params(W, H, 64.0)
        argb = torch.zeros(3 * W * H, dtype=torch.int32, device="cuda")
        c.rast_draw_device(p, argb.data_ptr())
        torch.cuda.synchronize()
        alone = c.rast_scratch_info()
        c.rast_draw_frames_device([p] * 3, argb.data_ptr())
        torch.cuda.synchronize()
        lanes = c.rast_scratch_info()
        assert lanes["route"] == cgamd.RAST_ROUTE_DENSE and lanes["bytes"] > alone["bytes"], "no lane rendered"
        c.rast_draw_sequence([p] * 3, chunk=1)
        c.rast_draw_buffers(p)
        # starfield: resident stars, frames into host memory
        c.starfield_set(cgamd.starfield_init(100))
        c.starfield_run([16.0] * 3, 3, W, H, chunk=1)
        torch.cuda.synchronize()
        held = _above(base)
        assert all(h > i for h, i in zip(held, IDLE)), held
    finally:
        c.close()
    assert _live() == base


def test_lattice_masks_order_maps_and_jpeg_scratch_are_freed():
    """Before the context's members owned their resources, cg_destroy forgot six device buffers:
    latmask, supmask, umask, lcost[2], lflat[2] and iscratch.  Each context of this loop would have
    left them behind, the device-allocation count growing with every iteration."""
    import torch
    base = _live()
    jpeg = _jpeg(cgamd.TEXTURE_FILES["grill"])
    for k in range(10):
        c = cgamd.Context(0)
        try:
            _lattice_calls(c, torch)
            c.decode_jpeg(jpeg)
            assert _above(base)[0] >= 8     # the six names above: eight allocations, among others
        finally:
            c.close()
        assert _live()[0] == base[0], f"context {k}"
    assert _live() == base


def test_dist_handles_and_their_contexts_are_freed():
    import torch
    base = _live()
    ctxs = [cgamd.Context(0) for _ in range(2)]
    ds = []
    try:
        for c in ctxs:
            _small_scene(c)
        ds = cgamd.Dist.local(ctxs)
        cams = [cgamd.rt_camera(W, H, F, (0.01 * k, 0.0, -3.0, 1.0)) for k in range(2)]
        frames = torch.zeros(2 * W * H, dtype=torch.int32, device="cuda")
        for d in reversed(ds):      # ranks > 0 enqueue first (local transport)
            d.render_frames(cams, frames.data_ptr() if d.rank == 0 else None)
        torch.cuda.synchronize()
        assert _above(base)[3] > 2 * IDLE[3]   # the handles' transfer streams
    finally:
        for d in ds:
            d.close()
        for c in ctxs:
            c.close()
    assert _live() == base
