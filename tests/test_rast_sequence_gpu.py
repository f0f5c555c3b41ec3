"""GPU: cg_rast_draw_sequence_device -- a frame sequence in any mix of colour
modes with the rand() call index chained on the device -- against the oracle
(all three planes of every frame bit-exact, the chain exact), and the device
seek + generator (cg_glibc_rand_device) against the host restatement."""
import functools

import numpy as np
import pytest

import cgamd
import oracle

pytestmark = pytest.mark.gpu

f32 = lambda x: float(np.float32(x))   # noqa: E731
MODES = [1, 1, 2, 0, 2, 1, 1, 2]
INFO = np.dtype([("rand_offset", "<u8"), ("n_shaded", "<i8"), ("status", "<i4"), ("pad", "<i4")])
SENT_A, SENT_D, SENT_S = -559038737, -7.5, 77   # 0xDEADBEEF as int32
# the CPU oracle's chain at 160 x 120, focal 90, from call index 0
OFFSETS_160 = [0, 28593, 66129, 115911, 115911, 184494, 255714, 331158]
CLOSING_160 = 412140
SHADED_160 = [9531, 12512, 16594, -1, 22861, 23740, 25148, 26994]


def _cfg(k):
    return dict(cam=(0.0, 0.0, f32(-3.001 + 0.25 * k), 1.0), light=(f32(0.1 * (k % 3) - 0.1), -0.5, 0.0, 1.0),
                indirect_first=f32(0.2))


def _params(W, H, F, start=0):
    return [cgamd.rast_params(W, H, F, _cfg(k)["cam"], None, _cfg(k)["light"], _cfg(k)["indirect_first"], MODES[k],
                              start if k == 0 else 0) for k in range(8)]


@functools.lru_cache(maxsize=None)
def _expected(W, H, F, start):
    """The oracle's 8 frames (argb, depth bits, shadow), the index each started at, its
    shaded fragments (-1 in mode 0), and the index after the last."""
    frames, offs, shaded, off = [], [], [], start
    for k in range(8):
        c = _cfg(k)
        p = oracle.rast_params(W, H, F, c["cam"], light=c["light"], indirect_first=c["indirect_first"],
                               colour_mode=MODES[k], rand_offset=off)
        a, d, s, cnt = oracle.rast_draw(p, counters=True)
        for x in (a, d, s):
            x.setflags(write=False)
        frames.append((a, d.view(np.uint32), s))
        offs.append(off)
        shaded.append(int(cnt.n_shaded) if MODES[k] else -1)
        if MODES[k]:
            off += 3 * int(cnt.n_shaded)
    return frames, offs, shaded, off


class Planes:
    def __init__(self, n, stride):
        import torch
        self.n, self.stride = n, stride
        self.a = torch.full((n * stride,), SENT_A, dtype=torch.int32, device="cuda")
        self.d = torch.full((n * stride,), SENT_D, dtype=torch.float32, device="cuda")
        self.s = torch.full((n * stride,), SENT_S, dtype=torch.int32, device="cuda")
        self.info = torch.full((3 * (n + 1),), -1, dtype=torch.int64, device="cuda")

    def draw(self, ctx, ps, first=0, info_first=None):
        """frames first .. first + len(ps) - 1 of the planes; records from info_first on"""
        import torch
        st = torch.cuda.current_stream()
        o = first * self.stride
        ctx.rast_draw_sequence_device(ps, self.a.data_ptr() + 4 * o, self.d.data_ptr() + 4 * o,
                                      self.s.data_ptr() + 4 * o, self.stride,
                                      self.info.data_ptr() + 24 * (first if info_first is None else info_first),
                                      st.cuda_stream)
        torch.cuda.synchronize()   # every stream: a null stream argument means the context's own

    def host(self):
        return (self.a.cpu().numpy().view(np.uint32), self.d.cpu().numpy().view(np.uint32), self.s.cpu().numpy(),
                self.info.cpu().numpy().view(INFO))


def _check_frame(A, D, S, k, stride, npx, ref):
    o = k * stride
    assert np.array_equal(S[o:o + npx], ref[2]), f"frame {k} shadow"
    assert np.array_equal(D[o:o + npx], ref[1]), f"frame {k} depth"
    assert np.array_equal(A[o:o + npx], ref[0]), f"frame {k} colour"


def _check_sentinel(A, D, S, lo, hi, what):
    assert np.all(A[lo:hi] == np.uint32(0xDEADBEEF)), f"{what}: colour written"
    assert np.all(D[lo:hi] == np.float32(SENT_D).view(np.uint32)), f"{what}: depth written"
    assert np.all(S[lo:hi] == SENT_S), f"{what}: shadow written"


def _check_all(pl, W, H, F, start):
    frames, offs, shaded, closing = _expected(W, H, F, start)
    A, D, S, info = pl.host()
    npx = W * H
    assert [int(x) for x in info["rand_offset"]] == offs + [closing]
    assert [int(x) for x in info["n_shaded"]] == shaded + [-1]
    assert not info["status"].any()
    for k in range(8):
        _check_frame(A, D, S, k, pl.stride, npx, frames[k])
        _check_sentinel(A, D, S, k * pl.stride + npx, (k + 1) * pl.stride, f"gap after frame {k}")


def test_sequence_chain_160x120(ctx):
    """8 frames, modes 1 1 2 0 2 1 1 2, from call index 0: planes, gaps and the chain."""
    W, H, F = 160, 120, 90.0
    _, offs, shaded, closing = _expected(W, H, F, 0)
    assert offs == OFFSETS_160 and closing == CLOSING_160 and shaded == SHADED_160   # the oracle, cross-checked
    ctx.rast_set_scene()
    pl = Planes(8, W * H + 256)
    pl.draw(ctx, _params(W, H, F, 0))
    _check_all(pl, W, H, F, 0)


def test_sequence_ragged_67x45(ctx):
    """Row tails in the 64-pixel walk, an odd height, a start index past 2^23."""
    W, H, F, start = 67, 45, 40.0, 12_000_000
    assert _expected(W, H, F, start)[3] == start + 69_864
    ctx.rast_set_scene()
    pl = Planes(8, W * H + 256)
    pl.draw(ctx, _params(W, H, F, start))
    _check_all(pl, W, H, F, start)


def test_sequence_second_call_continues(ctx):
    """Frames 0-3 in one call, 4-7 in a second that starts at the first's closing record."""
    W, H, F = 160, 120, 90.0
    ctx.rast_set_scene()
    pl = Planes(8, W * H + 256)
    ps = _params(W, H, F, 0)
    pl.draw(ctx, ps[:4])
    closing = int(pl.host()[3]["rand_offset"][4])
    assert closing == OFFSETS_160[4]
    ps[4].rand_offset = closing
    pl.draw(ctx, ps[4:], first=4)
    _check_all(pl, W, H, F, 0)


def test_sequence_capacity_is_exact(ctx):
    """A stream capacity of 20000 fragments: frames 4-7 (22861 .. 26994 shaded) are flagged and
    left undrawn, the chain stays exact, a flagged frame renders alone from its record, and
    the automatic capacity draws everything."""
    W, H, F = 160, 120, 90.0
    frames, offs, shaded, closing = _expected(W, H, F, 0)
    ctx.rast_set_scene()
    npx, stride = W * H, W * H + 256
    try:
        ctx.rast_set_rand_capacity(20000)
        pl = Planes(8, stride)
        pl.draw(ctx, _params(W, H, F, 0))
        A, D, S, info = pl.host()
        assert [int(x) for x in info["rand_offset"]] == OFFSETS_160 + [CLOSING_160]
        assert [int(x) for x in info["n_shaded"]] == SHADED_160 + [-1]
        assert [int(x) for x in info["status"]] == [0, 0, 0, 0] + [cgamd.CG_E_CAPACITY] * 4 + [0]
        for k in range(4):
            _check_frame(A, D, S, k, stride, npx, frames[k])
        _check_sentinel(A, D, S, 4 * stride, 8 * stride, "flagged frames")
        p5 = _params(W, H, F, 0)[5]
        p5.rand_offset = int(info["rand_offset"][5])
        a, d, s, st = ctx.rast_draw(p5)
        assert st.n_shaded == SHADED_160[5]
        assert np.array_equal(a, frames[5][0]) and np.array_equal(d.view(np.uint32), frames[5][1])
        assert np.array_equal(s, frames[5][2])
    finally:
        ctx.rast_set_rand_capacity(0)
    pl = Planes(8, stride)
    pl.draw(ctx, _params(W, H, F, 0))
    _check_all(pl, W, H, F, 0)


@pytest.mark.parametrize("n", [100, 2000])
def test_device_seek_and_generator_match_host(ctx, n):
    """cg_glibc_rand_device == cg_glibc_rand (pinned to glibc by the CPU suite), n = 2000
    crossing two 992-value chunks; call indices around the 31- and 344-word boundaries of
    the state, past 2^32, and a high bit set far above the low ones."""
    import torch
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    for off in (0, 1, 30, 31, 343, 344, 12_000_000, 2**32 - 1, 2**32, 2**40 + 7):
        d_off = torch.tensor([off], dtype=torch.int64, device="cuda")
        out.fill_(-1)
        st = torch.cuda.current_stream()
        ctx.glibc_rand_device(d_off.data_ptr(), n, out.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()   # every stream: a null stream argument means the context's own
        got, ref = out.cpu().numpy(), cgamd.glibc_rand(off, n)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, f"offset {off}: {bad.size} differ, first {bad[:4]} gpu {got[bad[:4]]} host {ref[bad[:4]]}"


def _rc(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


def test_sequence_argument_errors(ctx):
    W, H, F = 160, 120, 90.0
    pl = Planes(2, W * H)
    args = (pl.a.data_ptr(), pl.d.data_ptr(), pl.s.data_ptr())
    with cgamd.Context(0) as fresh:
        assert f"({cgamd.CG_E_NOSCENE})" in _rc(lambda: fresh.rast_draw_sequence_device(
            [cgamd.rast_params(W, H, F)], *args, 0, pl.info.data_ptr()))
    ctx.rast_set_scene()
    ok = cgamd.rast_params(W, H, F, colour_mode=1)
    inv = f"({cgamd.CG_E_INVALID})"
    assert inv in _rc(lambda: ctx.rast_draw_sequence_device([ok, cgamd.rast_params(W, H - 1, F)], *args, 0,
                                                            pl.info.data_ptr()))
    assert inv in _rc(lambda: ctx.rast_draw_sequence_device([ok, ok], *args, W * H - 1, pl.info.data_ptr()))
    assert inv in _rc(lambda: ctx.rast_draw_sequence_device([ok, ok], *args, 0, None))
    assert inv in _rc(lambda: ctx.rast_draw_sequence_device([ok, cgamd.rast_params(W, H, F, colour_mode=3)], *args, 0,
                                                            pl.info.data_ptr()))
    ctx.rast_draw_sequence_device([], *args, 0, pl.info.data_ptr())   # no frames: OK, nothing written
    import torch
    torch.cuda.synchronize()
    A, D, S, info = pl.host()
    _check_sentinel(A, D, S, 0, 2 * W * H, "no frames")
    assert np.all(pl.info.cpu().numpy() == -1)
