"""GPU: cg_rast_draw_sequence -- a rasteriser key script into host memory in one call.  The frames
render chunk by chunk through the device sequence while the previous chunk downloads; the rand()
call index passes from chunk to chunk on the device, and a frame the rand() stream's capacity
could not hold is repaired through the single-frame path.  Every plane of every frame and the
chain are checked against the oracle's (the frames, configurations and pinned chain of
tests/test_rast_sequence_gpu.py)."""
import numpy as np
import pytest

import cgamd
from test_rast_sequence_gpu import (CLOSING_160, MODES, OFFSETS_160, SHADED_160, Planes, _check_all, _expected,
                                    _params)

pytestmark = pytest.mark.gpu

SENT_A, SENT_D, SENT_S = np.uint32(0xDEADBEEF), np.float32(-7.5), np.int32(77)


def _check_frames(W, H, F, start, argb, depth, shadow, stride=None, frames=range(8), first=0):
    """frame k of the oracle's sequence at slot k - first of the planes"""
    ref = _expected(W, H, F, start)[0]
    npx = W * H
    stride = stride or npx
    for k in frames:
        o = (k - first) * stride
        if shadow is not None:
            assert np.array_equal(shadow[o:o + npx], ref[k][2]), f"frame {k} shadow"
        if depth is not None:
            assert np.array_equal(depth.view(np.uint32)[o:o + npx], ref[k][1]), f"frame {k} depth"
        assert np.array_equal(argb[o:o + npx], ref[k][0]), f"frame {k} colour"


def _check_info(info, offs, shaded, closing):
    assert [int(x) for x in info["rand_offset"]] == offs + [closing]
    assert [int(x) for x in info["n_shaded"]] == shaded + [-1]
    assert not info["status"].any()


@pytest.mark.parametrize("chunk", [1, 3, 4, 8, 0])
def test_every_chunk_boundary(ctx, chunk):
    """chunk 3: a boundary before the mode 0 frame and one between two mode 1 frames; chunk 4: one
    right after the mode 0 frame (the index passes through a record that frame did not advance);
    chunk 1: every frame its own chunk; 8 and 0 (= 8): one chunk."""
    W, H, F = 160, 120, 90.0
    ctx.rast_set_scene()
    a, d, s, info, st = ctx.rast_draw_sequence(_params(W, H, F, 0), want_depth=True, want_shadow=True, chunk=chunk)
    _check_info(info, OFFSETS_160, SHADED_160, CLOSING_160)
    _check_frames(W, H, F, 0, a, d, s)
    assert st.n_shaded == sum(x for x in SHADED_160 if x > 0)
    assert st.n_tris == cgamd.rast_prepare(_params(W, H, F, 0)[7])[1] == ctx.rast_scratch_info()["tris"]


def test_ragged_size_and_high_start(ctx):
    W, H, F, start = 67, 45, 40.0, 12_000_000
    _, offs, shaded, closing = _expected(W, H, F, start)
    assert closing == start + 69_864
    ctx.rast_set_scene()
    a, d, s, info, _ = ctx.rast_draw_sequence(_params(W, H, F, start), want_depth=True, want_shadow=True, chunk=3)
    _check_info(info, offs, shaded, closing)
    _check_frames(W, H, F, start, a, d, s)


@pytest.mark.parametrize("planes", [1, 3])
def test_gaps_and_unasked_planes_untouched(ctx, planes):
    W, H, F = 160, 120, 90.0
    npx, stride = W * H, W * H + 256
    A, D, S = np.full(8 * stride, SENT_A), np.full(8 * stride, SENT_D), np.full(8 * stride, SENT_S)
    ctx.rast_set_scene()
    a, d, s, info, _ = ctx.rast_draw_sequence(_params(W, H, F, 0), out=A, want_depth=D if planes == 3 else False,
                                              want_shadow=S if planes == 3 else False, chunk=3, frame_stride=stride)
    assert a is A
    _check_info(info, OFFSETS_160, SHADED_160, CLOSING_160)
    if planes == 3:
        assert d is D and s is S
        _check_frames(W, H, F, 0, A, D, S, stride)
    else:
        assert d is None and s is None
        _check_frames(W, H, F, 0, A, None, None, stride)
        assert np.all(D.view(np.uint32) == SENT_D.view(np.uint32)) and np.all(S == SENT_S)
    for k in range(8):
        lo, hi = k * stride + npx, (k + 1) * stride
        assert np.all(A[lo:hi] == SENT_A), f"gap after frame {k}: colour written"
        assert np.all(D.view(np.uint32)[lo:hi] == SENT_D.view(np.uint32)), f"gap after frame {k}: depth written"
        assert np.all(S[lo:hi] == SENT_S), f"gap after frame {k}: shadow written"


def test_pinned_and_pageable_agree(ctx):
    import torch
    W, H, F = 160, 120, 90.0
    ctx.rast_set_scene()
    a, _, _, info, _ = ctx.rast_draw_sequence(_params(W, H, F, 0), chunk=3)
    pinned = torch.zeros(8 * W * H, dtype=torch.int32).pin_memory()
    assert pinned.is_pinned()
    b, _, _, info2, _ = ctx.rast_draw_sequence(_params(W, H, F, 0), out=pinned, chunk=3)
    assert b is pinned
    assert np.array_equal(pinned.numpy().view(np.uint32), a) and np.array_equal(info, info2)
    _check_frames(W, H, F, 0, a, None, None)


def test_capacity_frames_are_repaired(ctx):
    """A stream of 20000 fragments: the device form flags frames 4-7 (22861 .. 26994 shaded;
    tests/test_rast_sequence_gpu.py); the host form delivers them all the same."""
    W, H, F = 160, 120, 90.0
    ctx.rast_set_scene()
    try:
        ctx.rast_set_rand_capacity(20000)
        a, d, s, info, st = ctx.rast_draw_sequence(_params(W, H, F, 0), want_depth=True, want_shadow=True, chunk=3)
        tris = ctx.rast_scratch_info()["tris"]
        # frames 4-6 repaired, the last frame (mode 0) not, every frame through the context's own
        # scratch (chunk 1): the scratch still reports the last frame
        b = ctx.rast_draw_sequence(_params(W, H, F, 0)[:7] + [cgamd.rast_params(W, H, F)], chunk=1)
        tris_b = ctx.rast_scratch_info()["tris"]
    finally:
        ctx.rast_set_rand_capacity(0)
    _check_info(info, OFFSETS_160, SHADED_160, CLOSING_160)
    _check_frames(W, H, F, 0, a, d, s)
    assert st.n_shaded == sum(x for x in SHADED_160 if x > 0)
    assert st.n_tris == tris == cgamd.rast_prepare(_params(W, H, F, 0)[7])[1]
    assert not b[3]["status"].any()
    _check_frames(W, H, F, 0, b[0], None, None, frames=range(7))
    assert b[4].n_tris == tris_b == cgamd.rast_prepare(cgamd.rast_params(W, H, F))[1]
    assert tris_b != cgamd.rast_prepare(_params(W, H, F, 0)[6])[1]   # the check has teeth


def test_second_call_continues_from_info(ctx):
    W, H, F = 160, 120, 90.0
    ctx.rast_set_scene()
    ps = _params(W, H, F, 0)
    a1, d1, s1, info1, _ = ctx.rast_draw_sequence(ps[:4], want_depth=True, want_shadow=True, chunk=3)
    assert int(info1["rand_offset"][4]) == OFFSETS_160[4]
    ps[4].rand_offset = int(info1["rand_offset"][4])
    a2, d2, s2, info2, _ = ctx.rast_draw_sequence(ps[4:], want_depth=True, want_shadow=True, chunk=3)
    _check_info(np.concatenate([info1[:4], info2]), OFFSETS_160, SHADED_160, CLOSING_160)
    _check_frames(W, H, F, 0, a1, d1, s1, frames=range(4))
    _check_frames(W, H, F, 0, a2, d2, s2, frames=range(4, 8), first=4)


def test_compact_route(ctx):
    W, H, F = 157, 93, 70.0
    f32 = lambda x: float(np.float32(x))   # noqa: E731
    ps = [cgamd.rast_params(W, H, F, cam=(0.0, 0.0, f32(-3.001 + 0.3 * k), 1.0), indirect_first=f32(0.15 if k == 0 else 0.2))
          for k in range(3)]
    ctx.rast_set_scene()
    try:
        ctx.rast_set_route(cgamd.RAST_ROUTE_COMPACT)
        a, d, s, info, st = ctx.rast_draw_sequence(ps, want_depth=True, want_shadow=True, chunk=2)
        assert ctx.rast_scratch_info()["route"] == cgamd.RAST_ROUTE_COMPACT
        singles = [ctx.rast_draw(p) for p in ps]
        colour = ps[:2] + [cgamd.rast_params(W, H, F, colour_mode=1)]
        with pytest.raises(RuntimeError) as e:   # modes 1-2 stay refused there, the message as it is
            ctx.rast_draw_sequence(colour, chunk=2)
        assert f"({cgamd.CG_E_INVALID})" in str(e.value) and "compact route" in str(e.value)
    finally:
        ctx.rast_set_route(-1)
    npx = W * H
    assert not info["status"].any() and list(info["n_shaded"]) == [-1] * 4 and st.n_shaded == -1
    assert len({a[k * npx:(k + 1) * npx].tobytes() for k in range(3)}) == 3
    for k, (ra, rd, rs, _) in enumerate(singles):
        o = slice(k * npx, (k + 1) * npx)
        assert np.array_equal(a[o], ra) and np.array_equal(s[o], rs), f"frame {k}"
        assert np.array_equal(d[o].view(np.uint32), rd.view(np.uint32)), f"frame {k} depth"


def _rc(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


def test_argument_errors(ctx):
    W, H, F = 160, 120, 90.0
    lib = ctx.lib
    A = np.full(2 * W * H, SENT_A)
    ok = cgamd.rast_params(W, H, F, colour_mode=1)
    with cgamd.Context(0) as fresh:
        assert f"({cgamd.CG_E_NOSCENE})" in _rc(lambda: fresh.rast_draw_sequence([ok], out=A))
    ctx.rast_set_scene()
    two = (cgamd.RastParams * 2)(ok, ok)
    mixed = (cgamd.RastParams * 2)(ok, cgamd.rast_params(W, H - 1, F))
    mode3 = (cgamd.RastParams * 2)(ok, cgamd.rast_params(W, H, F, colour_mode=3))
    P = cgamd.P
    call = lambda ps, n, argb, stride, chunk: lib.cg_rast_draw_sequence(   # noqa: E731
        ctx.h, ps, n, argb, None, None, stride, chunk, None, None)
    # through the C entry: the binding refuses some of these before the library sees them
    assert call(two, 2, P(A.ctypes.data), 0, 65) == cgamd.CG_E_INVALID
    assert call(two, 2, P(A.ctypes.data), 0, -1) == cgamd.CG_E_INVALID
    assert call(two, 2, P(A.ctypes.data), W * H - 1, 0) == cgamd.CG_E_INVALID
    assert call(mixed, 2, P(A.ctypes.data), 0, 0) == cgamd.CG_E_INVALID
    assert call(mode3, 2, P(A.ctypes.data), 0, 0) == cgamd.CG_E_INVALID
    assert call(None, 2, P(A.ctypes.data), 0, 0) == cgamd.CG_E_INVALID
    assert call(two, 2, None, 0, 0) == cgamd.CG_E_INVALID
    assert call(two, -1, P(A.ctypes.data), 0, 0) == cgamd.CG_E_INVALID
    assert call(two, 0, P(A.ctypes.data), 0, 0) == cgamd.CG_OK
    a, d, s, info, _ = ctx.rast_draw_sequence([], out=A)
    assert len(info) == 1 and np.all(A == SENT_A)


def test_device_form_unchanged(ctx):
    """The public device form goes through the entry the chunks use: one call still gives the
    records and planes it gave, and a second call still starts at its own ps[0].rand_offset
    whatever the records hold."""
    W, H, F = 160, 120, 90.0
    ctx.rast_set_scene()
    pl = Planes(8, W * H + 256)
    pl.draw(ctx, _params(W, H, F, 0))
    _check_all(pl, W, H, F, 0)
    pl.draw(ctx, _params(W, H, F, 0))   # the records now hold the first call's: they are not read
    _check_all(pl, W, H, F, 0)
    assert MODES[3] == 0
