"""GPU: resident stars and frame runs on the device (cg_starfield_set / _get / _run_device /
_advance_device / _run) against the oracle's main loop, Draw and Update frame by frame:
every pixel of every frame and every z of the final state bit for bit."""
import functools

import numpy as np
import pytest

import cgamd
import oracle
from star_seq_ref import SCRIPT, SPECIAL_DTS, SPECIAL_STARS, oracle_run, same_stars

pytestmark = pytest.mark.gpu

SENT = 0x5EA7BEEF            # never a starfield pixel (those are 0 or 0x80FFFFFF)
WHITE = 0x80FFFFFF
NOSCENE, CAPACITY = cgamd.CG_E_NOSCENE, cgamd.CG_E_CAPACITY


@functools.lru_cache(maxsize=None)
def _init(n):
    s = oracle.starfield_init(n)
    s.setflags(write=False)
    return s


class Frames:
    """n frames of device memory at `stride` pixels, pre-filled with the sentinel"""

    def __init__(self, n, W, H, stride=0):
        import torch
        self.n, self.px, self.stride = n, W * H, stride or W * H
        self.W, self.H = W, H
        self.t = torch.full((max(n * self.stride, 1),), SENT - (1 << 32) if SENT >= 1 << 31 else SENT,
                            dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # the runs go to the context's own stream

    def run(self, ctx, dts, n_frames=None, n_updates=None, first=0, stride_arg=None):
        n_frames = self.n - first if n_frames is None else n_frames
        ctx.starfield_run_device(dts, n_frames, self.W, self.H, self.t.data_ptr() + 4 * first * self.stride,
                                 n_updates, self.stride if stride_arg is None else stride_arg)

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint32)[:self.n * self.stride].reshape(self.n, self.stride)


def _check(got, final, ref_frames, ref_final, what=""):
    px = ref_frames.shape[1]
    for f in range(len(ref_frames)):
        assert np.array_equal(got[f, :px], ref_frames[f]), f"{what} frame {f}"
    assert (got[:, px:] == SENT).all(), f"{what}: pixels between frames written"
    assert same_stars(final, ref_final), f"{what} final state"


def _device_run(ctx, stars, dts, n_frames, W, H, n_updates=None, stride=0):
    ctx.starfield_set(stars)
    fr = Frames(n_frames, W, H, stride)
    fr.run(ctx, dts, n_frames, n_updates)
    final = ctx.starfield_get()
    return fr.host(), final


# ---- 1. the scripted session ---------------------------------------------------------------

def test_scripted_session(ctx):
    W, H, n = 320, 256, len(SCRIPT)
    ref, ref_final, (low, high) = oracle_run(_init(1000), SCRIPT, n, n, W, H)
    assert low >= 1000 and high == 370, "the script must take both wraps"
    white = (ref == WHITE).sum(axis=1)
    assert (white[:12] >= 100).all() and white[:12].min() == 106 and white[12] == 4
    assert (ref_final[:, 2] < -4.9e5).all()
    got, final = _device_run(ctx, _init(1000), SCRIPT, n, W, H)
    _check(got, final, ref, ref_final)
    assert np.array_equal(final.view(np.uint32), ref_final.view(np.uint32))


# ---- 2. launch and block boundaries --------------------------------------------------------

BW, BH, BDT = 64, 48, 16.0
_, L_, B_ = cgamd.starfield_plan(1000, 1)
BOUNDARY = sorted({min(x, 300) for x in (1, 2, B_ - 1, B_, B_ + 1, 2 * B_ + 1, L_ - 1, L_, L_ + 1, 2 * L_ + 3) if x > 0})


@functools.lru_cache(maxsize=None)
def _boundary_ref():
    """the oracle's frames 0 .. 299 at dt 16 and its stars after 0 .. 300 updates"""
    n = max(BOUNDARY)
    s = _init(1000).copy()
    frames, states, low = np.zeros((n, BW * BH), np.uint32), np.zeros((n + 1, 1000, 3), np.float32), []
    for f in range(n):
        states[f] = s
        frames[f] = oracle.starfield_draw(s, BW, BH)
        low.append(int((s[:, 2] <= 0).sum()))
        oracle.starfield_update(s, BDT)
    states[n] = s
    frames.setflags(write=False)
    states.setflags(write=False)
    return frames, states, low


def test_boundary_reference_is_not_trivial():
    frames, _, low = _boundary_ref()
    white = (frames == WHITE).sum(axis=1)
    assert sum(low[:130]) == 1015 and white[:130].min() == 301
    assert white.min() >= 100 and sum(low) > 1015


@pytest.mark.parametrize("last_update", [1, 0])
@pytest.mark.parametrize("n_frames", BOUNDARY)
def test_boundaries(ctx, n_frames, last_update):
    frames, states, _ = _boundary_ref()
    n_updates = n_frames - 1 + last_update
    launches, L, B = cgamd.starfield_plan(1000, n_frames)
    assert launches == -(-n_frames // L)
    got, final = _device_run(ctx, _init(1000), [BDT] * n_updates, n_frames, BW, BH, n_updates)
    _check(got, final, frames[:n_frames], states[n_updates], f"{n_frames} frames, {n_updates} updates")


# ---- 3. split invariance -------------------------------------------------------------------

def test_split_invariance(ctx):
    W, H, n = 64, 48, 70
    dts = [16.0 + 7.0 * (k % 5) for k in range(n)]
    ref, ref_final, _ = oracle_run(_init(1000), dts, n, n, W, H)
    got, final = _device_run(ctx, _init(1000), dts, n, W, H)
    _check(got, final, ref, ref_final, "one run")
    # 33 + 37, queued back to back with no synchronise in between
    ctx.starfield_set(_init(1000))
    fr = Frames(n, W, H)
    fr.run(ctx, dts[:33], 33, 33, first=0)
    fr.run(ctx, dts[33:], 37, 37, first=33)
    final2 = ctx.starfield_get()
    _check(fr.host(), final2, ref, ref_final, "33 + 37")
    # 70 runs of one frame
    ctx.starfield_set(_init(1000))
    fr = Frames(n, W, H)
    for f in range(n):
        fr.run(ctx, dts[f:f + 1], 1, 1, first=f)
    final3 = ctx.starfield_get()
    _check(fr.host(), final3, ref, ref_final, "70 x 1")


# ---- 4. star counts -------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(64, 48), (7, 5)])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000, 100003])
def test_star_counts(ctx, n, W, H):
    dts = [16.0, 400.0, 33.0]
    ref, ref_final, _ = oracle_run(_init(n), dts, 3, 3, W, H)
    if n >= 63:
        assert (ref == WHITE).any()
    got, final = _device_run(ctx, _init(n), dts, 3, W, H)
    assert final.shape == (n, 3)
    _check(got, final, ref, ref_final, f"{n} stars {W}x{H}")


# ---- 5. sizes --------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1921, 1081), (1920, 1080)])
def test_sizes(ctx, W, H):
    dts = [16.0, 400.0, 33.0]
    ref, ref_final, _ = oracle_run(_init(5000), dts, 3, 3, W, H)
    assert ((ref == WHITE).sum(axis=1) >= 100).all()
    got, final = _device_run(ctx, _init(5000), dts, 3, W, H)
    _check(got, final, ref, ref_final, f"{W}x{H}")


# ---- 6. special values -----------------------------------------------------------------------

# the whole list (every z ends NaN), the list up to its inf (ends -inf or NaN) and its finite start
@pytest.mark.parametrize("n,last_update", [(len(SPECIAL_DTS), 1), (len(SPECIAL_DTS), 0), (4, 1), (3, 1)])
def test_special_values(ctx, n, last_update):
    W, H = 64, 48
    nu = n - 1 + last_update
    ref, ref_final, _ = oracle_run(SPECIAL_STARS, SPECIAL_DTS, nu, n, W, H)
    assert (ref == WHITE).any() and np.isnan(ref_final[:, 2]).any()
    assert n == len(SPECIAL_DTS) or not np.isnan(ref_final[:, 2]).all()
    with np.errstate(invalid="ignore"):
        got, final = _device_run(ctx, SPECIAL_STARS, SPECIAL_DTS, n, W, H, nu)
    _check(got, final, ref, ref_final, "special values")
    # and one frame at a time, so that every special state is also a launch's input
    ctx.starfield_set(SPECIAL_STARS)
    fr = Frames(n, W, H)
    for f in range(n):
        fr.run(ctx, SPECIAL_DTS[f:f + 1], 1, 1 if f < nu else 0, first=f)
    _check(fr.host(), ctx.starfield_get(), ref, ref_final, "special values, frame by frame")


# ---- 7. frame stride ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames", [5, 11])
def test_frame_stride_leaves_gaps_alone(ctx, n_frames):
    W, H = 64, 48
    dts = [16.0 + k for k in range(n_frames)]
    ref, ref_final, _ = oracle_run(_init(1000), dts, n_frames, n_frames, W, H)
    got, final = _device_run(ctx, _init(1000), dts, n_frames, W, H, stride=W * H + 37)
    assert got.shape == (n_frames, W * H + 37)
    _check(got, final, ref, ref_final, "stride W*H + 37")      # _check also asserts the gaps' sentinel


# ---- 8. advance_device -------------------------------------------------------------------------

@pytest.mark.parametrize("n_updates", [1, 13, L_ + 5])
def test_advance_then_draw(ctx, n_updates):
    W, H = 64, 48
    dts = [SCRIPT[k % len(SCRIPT)] if k % len(SCRIPT) != 11 else 20.0 for k in range(n_updates)]
    s = _init(1000).copy()
    for dt in dts:
        oracle.starfield_update(s, float(np.float32(dt)))
    ref = oracle.starfield_draw(s, W, H)
    assert (ref == WHITE).sum() >= 100
    ctx.starfield_set(_init(1000))
    ctx.starfield_advance_device(dts)
    fr = Frames(1, W, H)
    fr.run(ctx, [], 1, 0)
    final = ctx.starfield_get()
    _check(fr.host(), final, ref[None, :], s, f"advance x {n_updates}")


# ---- 9. the host form --------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [0, 1, 3, 40])
def test_host_form_equals_device_form(ctx, chunk):
    W, H, n = 64, 48, 19
    dts = [16.0 + 3.0 * (k % 7) for k in range(n)]
    ref, ref_final, _ = oracle_run(_init(1000), dts, n, n, W, H)
    dev, dev_final = _device_run(ctx, _init(1000), dts, n, W, H)
    ctx.starfield_set(_init(1000))
    out, st = ctx.starfield_run(dts, n, W, H, chunk=chunk)
    final = ctx.starfield_get()
    assert np.array_equal(out.reshape(n, W * H), dev) and np.array_equal(final.view(np.uint32), dev_final.view(np.uint32))
    _check(out.reshape(n, W * H), final, ref, ref_final, f"chunk {chunk}")
    assert st.total_ms > 0


def test_host_form_pinned_strided_and_last_frame_only_drawn(ctx):
    import torch
    W, H, n = 64, 48, 10
    stride = W * H + 37
    dts = [16.0] * (n - 1)
    ref, ref_final, _ = oracle_run(_init(1000), dts, n - 1, n, W, H)
    pinned = torch.full((n * stride,), 7, dtype=torch.int32).pin_memory()
    ctx.starfield_set(_init(1000))
    out, _ = ctx.starfield_run(dts, n, W, H, n_updates=n - 1, out=pinned, chunk=4, frame_stride=stride)
    got = pinned.numpy().view(np.uint32).reshape(n, stride)
    for f in range(n):
        assert np.array_equal(got[f, :W * H], ref[f]), f
    assert (got[:, W * H:] == 7).all()
    assert same_stars(ctx.starfield_get(), ref_final)


def test_old_draw_interleaved_with_resident_runs(ctx):
    """cg_starfield_draw (its own upload and buffers) between queued resident runs: neither
    disturbs the other."""
    W, H, n = 64, 48, 12
    dts = [16.0 + k for k in range(n)]
    ref, ref_final, _ = oracle_run(_init(1000), dts, n, n, W, H)
    other = _init(5000)[1000:].copy()
    other_ref = oracle.starfield_draw(other.copy(), W, H)
    ctx.starfield_set(_init(1000))
    fr = Frames(n, W, H)
    fr.run(ctx, dts[:5], 5, 5, first=0)
    assert np.array_equal(ctx.starfield_draw(other, W, H), other_ref)
    host, _ = ctx.starfield_run(dts[5:8], 3, W, H, chunk=2)
    assert np.array_equal(ctx.starfield_draw(other, W, H), other_ref)
    fr.run(ctx, dts[8:], 4, 4, first=8)
    final = ctx.starfield_get()
    got = fr.host().copy()
    got[5:8] = host.reshape(3, W * H)
    _check(got, final, ref, ref_final, "interleaved")
    assert np.array_equal(ctx.starfield_draw(other, W, H), other_ref)


# ---- 10. errors --------------------------------------------------------------------------------

def test_errors():
    import ctypes as C
    with cgamd.Context(0) as c:
        fr = Frames(1, 8, 8)
        dts = (C.c_float * 2)(16, 16)
        P = C.c_void_p
        assert c.lib.cg_starfield_run_device(c.h, C.cast(dts, P), 1, 1, 8, 8, P(fr.t.data_ptr()), 0, None) == NOSCENE
        assert c.lib.cg_starfield_advance_device(c.h, C.cast(dts, P), 1, None) == NOSCENE
        host = np.zeros(64, np.uint32)
        assert c.lib.cg_starfield_run(c.h, C.cast(dts, P), 1, 1, 8, 8, host.ctypes.data_as(P), 0, 0, None) == NOSCENE
        out = np.zeros((8, 3), np.float32)
        assert c.lib.cg_starfield_get(c.h, out.ctypes.data_as(P), 8) == NOSCENE
        assert (fr.host() == SENT).all()
        c.starfield_set(_init(5))
        assert c.lib.cg_starfield_get(c.h, out.ctypes.data_as(P), 4) == CAPACITY
        assert c.lib.cg_starfield_get(c.h, out.ctypes.data_as(P), 8) == 5
        assert np.array_equal(out[:5], _init(5))
        with pytest.raises(RuntimeError):
            c.starfield_get(cap=2)
        c.starfield_set(_init(0))                       # an empty field is a scene
        fr.run(c, [16.0], 1, 1)
        assert (fr.host() == 0).all() and c.starfield_get().shape == (0, 3)
        c.starfield_set(_init(70))                      # replaces the set, growing the buffers
        assert np.array_equal(c.starfield_get(), _init(70))
