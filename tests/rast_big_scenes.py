"""Scenes and bounds shared by tests/test_rast_big.py (CPU) and tests/test_rast_big_gpu.py."""
import ctypes as C

import numpy as np

import cgamd

# case 2 of the GPU tests: a room beyond the old 4,096-input limit
BEYOND = dict(n=6000, extent=0.3, seed=0x5EED, W=96, H=48, focal=48.0)

RTRI = np.dtype([("v", "<f4", (3, 4)), ("normal", "<f4", 4), ("color", "<f4", 3), ("texture", "<i4"), ("index", "<i4")])
assert RTRI.itemsize == 84


def as_rtri(arr):
    """numpy RTRI records -> ctypes RTri array (a copy)."""
    arr = np.ascontiguousarray(arr, RTRI)
    out = (cgamd.RTri * max(len(arr), 1))()
    C.memmove(out, arr.ctypes.data, arr.nbytes)
    return out


def as_numpy(tris, n):
    return np.frombuffer(C.string_at(C.addressof(tris), n * 84), RTRI).copy()


def camera_list(n, W, H, focal, rows, rng):
    """n already-clipped camera-space triangles for cg_rast_render, in pairs: each triangle is
    listed twice in a row with two colours (an exact depth tie: the later one must win).  Every
    triangle covers screen rows rows[0] .. rows[1] (one row when equal); depths repeat among the
    pairs, so ties also occur between triangles that are far apart in the list."""
    t = np.zeros(n, RTRI)
    half = (n + 1) // 2
    z = rng.choice(np.array([1.0, 1.25, 1.5, 2.0, 3.0], np.float32), half)
    xa = rng.integers(-4, W // 2, half).astype(np.float32)
    xb = xa + rng.integers(3, W, half).astype(np.float32)
    col = rng.uniform(0.15, 0.75, (half, 2, 3)).astype(np.float32)
    f = np.float32(focal)
    # x_pix = f * X / Z + W / 2 and y_pix likewise: choose X, Y so the pixel coordinates are
    # these integers plus a half (far from a rounding boundary)
    X = lambda px: ((px + np.float32(0.5) - np.float32(W // 2)) * z / f).astype(np.float32)   # noqa: E731
    Y = lambda py: ((np.float32(py) + np.float32(0.5) - np.float32(H // 2)) * z / f).astype(np.float32)   # noqa: E731
    p, c = np.arange(n) // 2, np.arange(n) % 2
    one = np.ones(half, np.float32)
    y0, y1 = rows
    t["v"][:, 0] = np.stack([X(xa), Y(y0), z, one], 1)[p]
    t["v"][:, 1] = np.stack([X(xb), Y(y0), z, one], 1)[p]
    t["v"][:, 2] = np.stack([X((xa + xb) / 2), Y(y1), z, one], 1)[p]
    t["color"] = col[p, c]
    t["normal"] = (0.0, 0.0, -1.0, 1.0)
    return t


def oracle_params(p):
    """The oracle's parameter record of the frame a cgamd.RastParams describes."""
    import oracle
    v4 = lambda v: (v.x, v.y, v.z, v.w)   # noqa: E731
    return oracle.rast_params(p.width, p.height, p.focal, v4(p.camera), list(p.R), v4(p.light_scene),
                              p.indirect_first, p.colour_mode, p.rand_offset, yaw=p.yaw)


def oracle_scene_frame(p, room, nr, boxes, nb):
    """(argb, depth, shadow, counters): the oracle's Draw of a caller's room and boxes -- its own
    clip, its own fill; nothing of the library's."""
    import oracle
    return oracle.rast_draw(oracle_params(p), counters=True, scene=(room, nr, boxes, nb))


def oracle_list_frame(p, tris, n, light):
    """(argb, depth, shadow, counters): the oracle's Draw of an already clipped list (what
    cg_rast_render takes)."""
    import oracle
    return oracle.rast_draw_list(oracle_params(p), tris, n, light, counters=True)


def scratch_need(n_in, info, W, H, chunk):
    """Device bytes per buffer that one compact-route cg_rast_draw frame needs: a formula of the
    frame's own counts (cg_rast_scratch_info out[2..4]) and the struct sizes.  Triangle 84 B,
    span 32 B + its 8 B (triangle, row) key, header 32 B, row record 48 B, offsets 8 B."""
    n, S, R = max(info["tris"], 1), max(info["spans"], 1), max(info["recs"], 1)
    ni = max(n_in, 1)
    blocks = lambda N: -(-N // 4096) * 8   # noqa: E731  the scans' block sums
    return {
        "stage": ni * 32 * 84, "geo": 64 + 4 * ni, "count": (H + 16) * 4, "pre": (ni + 1) * 8,
        "scan": max(blocks(n_in), blocks(info["tris"])), "tris": n * 84, "hdr": n * 32, "nrows": n * 4,
        "span_off": (n + 1) * 8, "row_off": (H + 2) * 8, "state": W * H * 4, "spans": S * 32, "span_ty": S * 8,
        "hist": max(-(-info["spans"] // chunk), 1) * H * 4, "recs": R * 48,
    }
