"""CPU: the host-only entry points of the rasteriser's compact route -- the route rule, the
row-list block sizes and the random scene generator (PCG32, restated here) -- and the
condition the GPU test beyond the old scene limit relies on."""
import ctypes as C

import numpy as np

import cgamd
import rast_big_scenes as sc


def test_route_rule():
    assert cgamd.rast_route(0) == cgamd.RAST_ROUTE_DENSE == 0
    assert cgamd.rast_route(131072) == cgamd.RAST_ROUTE_DENSE
    assert cgamd.rast_route(131073) == cgamd.RAST_ROUTE_COMPACT == 1


def test_row_blocks():
    batch, chunk = cgamd.rast_row_blocks()
    assert batch == 64 and chunk > batch and chunk % batch == 0
    assert cgamd.load().cg_rast_row_blocks(None, None) == cgamd.CG_E_INVALID


class Pcg32:
    """pcg32_random_r seeded as pcg32_srandom_r(seed, seq)."""
    M = (1 << 64) - 1

    def __init__(self, seed, seq):
        self.state, self.inc = 0, ((seq << 1) | 1) & self.M
        self.next()
        self.state = (self.state + seed) & self.M
        self.next()

    def next(self):
        old = self.state
        self.state = (old * 6364136223846793005 + self.inc) & self.M
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF

    def uniform(self, a, b):
        f = np.float32
        u = f(self.next() >> 8) * f(5.9604644775390625e-8)
        return f(f(a) + f(f(f(b) - f(a)) * u))


def test_random_scene_layout_and_draws():
    assert C.sizeof(cgamd.RTri) == 84 and cgamd.RTri.color.offset == 64 and cgamd.RTri.texture.offset == 76
    n, extent = 7, 0.3
    t = sc.as_numpy(cgamd.rast_random_scene(n, extent, seed=99), n)
    g = Pcg32(99, 54)
    for k in range(n):
        c = [g.uniform(-1.0, 1.0) for _ in range(3)]
        for v in range(3):
            d = [g.uniform(-extent, extent) for _ in range(3)]
            want = np.array([c[0] + d[0], c[1] + d[1], c[2] + d[2], 1.0], np.float32)
            assert np.array_equal(t["v"][k, v], want), (k, v)
        col = np.array([g.uniform(0.15, 0.75) for _ in range(3)], np.float32)
        assert np.array_equal(t["color"][k], col)
        # ComputeNormal (TestModelH.h:32-41): normalize(cross(v2 - v0, v1 - v0)), w = 1
        e1, e2 = t["v"][k, 1, :3] - t["v"][k, 0, :3], t["v"][k, 2, :3] - t["v"][k, 0, :3]
        nrm = np.cross(e2.astype(np.float64), e1.astype(np.float64))
        nrm /= np.linalg.norm(nrm)
        assert np.allclose(t["normal"][k, :3], nrm, atol=1e-5) and t["normal"][k, 3] == 1.0
    assert not t["texture"].any() and not t["index"].any()


def test_random_scene_seeds_and_extent():
    n, extent = 1000, 0.02
    a = sc.as_numpy(cgamd.rast_random_scene(n, extent), n)
    b = sc.as_numpy(cgamd.rast_random_scene(n, extent), n)
    c = sc.as_numpy(cgamd.rast_random_scene(n, extent, seed=0x5EED + 1), n)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    # every vertex within `extent` of the triangle's centroid draw, per axis: the three vertices
    # lie in one box of side 2 * extent (one float32 rounding of a coordinate <= 1.02 allowed)
    xyz = a["v"][:, :, :3].astype(np.float64)
    assert (xyz.max(1) - xyz.min(1)).max() <= 2 * extent + 2.0 ** -22
    assert np.abs(xyz).max() <= 1.0 + extent + 2.0 ** -22
    assert (a["v"][:, :, 3] == 1.0).all()
    assert (a["color"] >= 0.15).all() and (a["color"] <= 0.75).all()


def test_random_scene_argument_errors():
    lib = cgamd.load()
    buf = (cgamd.RTri * 4)()
    assert lib.cg_rast_random_scene(1, -1, 0.02, buf) == cgamd.CG_E_INVALID
    assert lib.cg_rast_random_scene(1, 4, 0.02, None) == cgamd.CG_E_INVALID
    assert lib.cg_rast_random_scene(1, 4, -0.5, buf) == cgamd.CG_E_INVALID
    assert lib.cg_rast_random_scene(1, 4, float("nan"), buf) == cgamd.CG_E_INVALID
    assert lib.cg_rast_random_scene(1, 0, 0.02, None) == 0
    assert lib.cg_rast_random_scene(1, 4, 0.02, buf) == 4


def test_beyond_scene_clips_past_the_old_limit():
    """The GPU test's scene: more than 4,096 input triangles and more than 4,096 clipped ones."""
    B = sc.BEYOND
    room = cgamd.rast_random_scene(B["n"], B["extent"], B["seed"])
    p = cgamd.rast_params(B["W"], B["H"], B["focal"])
    _, n, _ = cgamd.rast_prepare(p, room, B["n"], (cgamd.RTri * 1)(), 0)
    assert B["n"] > 4096 and n > 4096
    assert cgamd.rast_route(32 * B["n"]) == cgamd.RAST_ROUTE_COMPACT
