"""CPU: the starfield frame-sequence C-ABI without a device -- cg_starfield_plan's
properties, every argument check that comes before any HIP call, and the host
cg_starfield_update (what the sequence kernel is compared with) against the oracle
over the scripted session and the special values of the GPU tests."""
import ctypes as C

import numpy as np

import cgamd
import oracle
from star_seq_ref import SCRIPT, SPECIAL_DTS, SPECIAL_STARS, oracle_run, same_stars

INVALID = cgamd.CG_E_INVALID


def test_plan_properties():
    lib = cgamd.load()
    for n_stars in (0, 1, 1000, 100003):
        n0, L, B = cgamd.starfield_plan(n_stars, 0)
        assert n0 == 0 and 1 <= B <= L
        prev = 0
        for nf in list(range(0, 3 * L + 5)) + [10 * L, 10 * L + 1]:
            n, L2, B2 = cgamd.starfield_plan(n_stars, nf)
            assert (L2, B2) == (L, B)
            assert n == -(-nf // L)
            assert n >= prev
            prev = n
    assert lib.cg_starfield_plan(1000, 7, None, None) == 1          # the outputs are optional
    Lc, Bc = C.c_int(), C.c_int()
    assert lib.cg_starfield_plan(-1, 4, C.byref(Lc), C.byref(Bc)) == INVALID
    assert lib.cg_starfield_plan(4, -1, C.byref(Lc), C.byref(Bc)) == INVALID
    try:
        cgamd.starfield_plan(1000, -3)
    except ValueError:
        pass
    else:
        raise AssertionError("starfield_plan must reject a negative frame count")


def test_argument_checks_need_no_device():
    lib = cgamd.load()
    dts = (C.c_float * 4)(16, 16, 16, 16)
    stars = (C.c_float * 6)()
    buf = (C.c_uint32 * 64)()
    P = C.c_void_p
    d, s, b = C.cast(dts, P), C.cast(stars, P), C.cast(buf, P)
    # no context
    assert lib.cg_starfield_set(None, s, 2) == INVALID
    assert lib.cg_starfield_get(None, s, 2) == INVALID
    assert lib.cg_starfield_run_device(None, d, 2, 2, 4, 4, b, 0, None) == INVALID
    assert lib.cg_starfield_advance_device(None, d, 2, None) == INVALID
    assert lib.cg_starfield_run(None, d, 2, 2, 4, 4, b, 0, 0, None) == INVALID
    # bad counts and sizes are refused before the context is looked at: a non-null handle that
    # is never dereferenced stands in for one
    fake = P(C.addressof(buf))
    for nu, nf, W, H, dd in ((-1, 0, 4, 4, d), (2, -1, 4, 4, d), (0, 2, 4, 4, d), (3, 2, 4, 4, d), (2, 2, 0, 4, d),
                             (2, 2, 4, -1, d), (2, 2, 4, 4, None), (1, 2, 4, 4, None)):
        assert lib.cg_starfield_run_device(fake, dd, nu, nf, W, H, b, 0, None) == INVALID, (nu, nf, W, H)
        assert lib.cg_starfield_run(fake, dd, nu, nf, W, H, b, 0, 0, None) == INVALID, (nu, nf, W, H)
    assert lib.cg_starfield_run_device(fake, d, 2, 2, 4, 4, b, 15, None) == INVALID      # frame_stride < W * H
    assert lib.cg_starfield_run(fake, d, 2, 2, 4, 4, b, 15, 0, None) == INVALID
    assert lib.cg_starfield_run(fake, d, 2, 2, 4, 4, b, 0, -1, None) == INVALID          # chunk < 0
    assert lib.cg_starfield_run_device(fake, d, 2, 2, 4, 4, None, 0, None) == INVALID    # no frames buffer
    assert lib.cg_starfield_advance_device(fake, d, -1, None) == INVALID
    assert lib.cg_starfield_advance_device(fake, None, 1, None) == INVALID
    assert lib.cg_starfield_set(fake, s, -1) == INVALID
    assert lib.cg_starfield_set(fake, None, 2) == INVALID
    assert lib.cg_starfield_get(fake, s, -1) == INVALID


def test_binding_and_header():
    for name in ("cg_starfield_set", "cg_starfield_get", "cg_starfield_run_device", "cg_starfield_advance_device",
                 "cg_starfield_run", "cg_starfield_plan"):
        assert name in cgamd.EXPORTS
    for meth in ("starfield_set", "starfield_get", "starfield_run_device", "starfield_advance_device", "starfield_run"):
        assert callable(getattr(cgamd.Context, meth))


def test_host_update_matches_oracle_scripted_session():
    """cg_starfield_update, the per-frame API the sequence kernel must equal, over the script
    of the GPU tests; the script takes both wraps (checked on the oracle's own state)."""
    a = cgamd.starfield_init(1000)
    _, ref, (low, high) = oracle_run(oracle.starfield_init(1000), SCRIPT, len(SCRIPT), 0, 1, 1)
    assert low >= 1000 and high == 370
    for dt in SCRIPT:
        cgamd.starfield_update(a, dt)
    assert np.array_equal(a.view(np.uint32), ref.view(np.uint32))
    assert (ref[:, 2] < -4.9e5).all()


def test_host_update_matches_oracle_special_values():
    a = SPECIAL_STARS.copy()
    _, ref, _ = oracle_run(SPECIAL_STARS, SPECIAL_DTS, len(SPECIAL_DTS), 0, 1, 1)
    with np.errstate(invalid="ignore"):
        for k, dt in enumerate(SPECIAL_DTS):
            cgamd.starfield_update(a, dt)
            _, part, _ = oracle_run(SPECIAL_STARS, SPECIAL_DTS, k + 1, 0, 1, 1)
            assert same_stars(a, part), k
    assert same_stars(a, ref)
