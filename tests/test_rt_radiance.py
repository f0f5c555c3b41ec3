"""CPU: the reference of the CG_PIX_RGBA_F32 tests (tests/rt_radiance_ref.py) pinned to the oracle,
and the host-only parts of the format.  No GPU.

For every scene and camera the GPU test compares against, cgo_put_pixel of the restated pixel loop's
x, y, z equals oracle.rt_draw's ARGB on every pixel: the restatement performs the oracle's operations
in the oracle's order, so the float values it hands the GPU test are the ones the oracle packs."""
import os

import numpy as np
import pytest

import cgamd
import oracle
import rt_radiance_ref as ref

CG_E_INVALID = -1


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_packs_to_the_oracle_frame(name):
    case, _ = ref.CASES[name]
    rad = ref.reference(name)
    want = oracle.rt_draw(ref.oracle_params(case), scene=ref.scene(case["scene"]).oracle_scene(),
                          threads=min(16, os.cpu_count() or 8))
    got = ref.put_pixels(rad[..., :3]).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[:6]}"
    w = rad[..., 3]
    assert w.min() >= 0 and w.max() <= 9 and np.array_equal(w, np.round(w))
    # a pixel no sub-ray of which hit is +0 in all three, and packs to PutPixelSDL(0, 0, 0)
    miss = w.reshape(-1) == 0
    assert not rad.reshape(-1, 4)[miss].view(np.uint32).any()
    assert (want[miss] == 0x80000000).all()
    assert (~miss).sum() > 50                      # the frame does see the scene


@pytest.mark.parametrize("name", list(ref.CASES))
def test_cases_take_the_routes_they_are_meant_for(name):
    case, route = ref.CASES[name]
    sc = ref.scene(case["scene"])
    assert cgamd.rt_route(ref.camera(case), sc.n, sc.n_sph, len(ref.lights_of(case))) == route


def test_pix_bytes():
    lib = cgamd.load()
    assert cgamd.PIX_RGBA_F32 == 2
    assert [lib.cg_pix_bytes(f) for f in (cgamd.PIX_ARGB8888, cgamd.PIX_RGB24, cgamd.PIX_RGBA_F32)] == [4, 3, 16]
    for f in (-1, 3, 4, 1 << 20):
        assert lib.cg_pix_bytes(f) == CG_E_INVALID
    assert cgamd.pix_bytes(cgamd.PIX_RGBA_F32) == 16
    with pytest.raises(ValueError):
        cgamd.pix_bytes(3)
