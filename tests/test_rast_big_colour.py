"""CPU: the host-only parts of colour modes 1-2 on the rasteriser's compact route -- the segment
rule that sizes the fragment-count entries (cg_rast_span_segments, shared by the kernels) against a
numpy restatement, and the two new entries of the C ABI."""
import ctypes as C

import numpy as np

import cgamd

SEG = 64   # kFillPx: pixels per fill wave


def _segments(lx, rx, W):
    """The 64-pixel segments that hold a pixel of [max(lx, 0), min(rx, W)), by enumeration."""
    x = np.arange(max(lx, 0), min(rx, W))
    s = np.unique(x // SEG)
    return (len(s), int(s[0])) if len(s) else (0, None)


def test_span_segments_matches_enumeration():
    cases = 0
    for W in (64, 65, 157):
        edges = sorted({-70, -64, -1, 0, 1, 62, 63, 64, 65, 66, 127, 128, 129, W - 1, W, W + 1, W + 70})
        for lx in edges:
            for rx in edges:
                n, first = cgamd.rast_span_segments(lx, rx, W)
                want_n, want_first = _segments(lx, rx, W)
                assert n == want_n, (W, lx, rx, n, want_n)
                if want_n:
                    assert first == want_first, (W, lx, rx, first, want_first)
                    assert 0 <= first and first + n <= -(-W // SEG)      # entries stay inside the row's segments
                cases += 1
    assert cases > 600


def test_span_segments_named_cases():
    f = cgamd.rast_span_segments
    assert f(-5, 10, 157) == (1, 0)               # lx < 0: the extent starts at pixel 0
    assert f(100, 400, 157) == (2, 1)             # rx > W: it ends at W (pixels 100 .. 156)
    assert f(10, 10, 157)[0] == 0 and f(12, 3, 157)[0] == 0      # rx <= lx: no fragment
    assert f(-9, 0, 157)[0] == 0 and f(157, 200, 157)[0] == 0    # wholly off screen
    assert f(0, 63, 157) == (1, 0)                # last pixel 62
    assert f(0, 64, 157) == (1, 0)                # last pixel 63: still one segment
    assert f(0, 65, 157) == (2, 0)                # last pixel 64: the second segment
    assert f(63, 65, 157) == (2, 0) and f(64, 65, 157) == (1, 1)
    assert f(0, 64, 64) == (1, 0) and f(0, 65, 65) == (2, 0) and f(-3, 999, 157) == (3, 0)
    # a random sweep: the count is the closed form of the enumeration
    rng = np.random.default_rng(11)
    for lx, rx, W in zip(rng.integers(-200, 400, 300), rng.integers(-200, 400, 300), rng.choice([64, 65, 157], 300)):
        n, first = f(int(lx), int(rx), int(W))
        assert (n, first if n else None) == _segments(int(lx), int(rx), int(W))


def test_abi_of_the_new_entries():
    lib = cgamd.load()
    for name in ("cg_rast_set_route_limit", "cg_rast_span_segments"):
        assert hasattr(lib, name), name
    assert lib.cg_rast_set_route_limit.argtypes == [C.c_void_p, C.c_longlong]
    assert lib.cg_rast_set_route_limit.restype is C.c_int
    assert lib.cg_rast_span_segments.argtypes == [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    assert lib.cg_rast_span_segments.restype is C.c_int
    assert lib.cg_rast_span_segments(0, 65, 157, None) == 2          # *first is optional
    assert lib.cg_rast_set_route_limit(None, 1) == cgamd.CG_E_INVALID
    assert callable(cgamd.Context.rast_set_route_limit)
