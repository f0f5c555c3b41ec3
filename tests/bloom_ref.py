"""The bloom contract (include/cg_render.h, "Bloom") restated in numpy: bright pass, level sizes,
box, blur, up-sample, pyramid and composite, all in np.float32 with every float operation followed
by its own .astype(np.float32) so that nothing can be fused or reordered, and every select a
np.where on the comparison the contract writes.  It shares no code with the library; the tone
curves and PutPixelSDL are tests/hdr_ref.py's.  tests/test_bloom.py pins it by hand and compares
the library's host functions with it; tests/test_bloom_gpu.py compares the kernels with it.
Planes are float32[h, w, 3]; a stored pyramid is float32[total, 4] with +0.0f in the fourth float."""
import numpy as np

import hdr_ref

F = np.float32
MAX_LEVELS = 6
RULE_RT, RULE_RAST = 0, 1
_err = dict(all="ignore")


def f32(x):
    return np.asarray(x, dtype=np.float32)


def level_sizes(W, H, levels):
    """[(W_k, H_k)] for k = 1 .. levels."""
    out = []
    for _ in range(levels):
        W, H = (W + 1) // 2, (H + 1) // 2
        out.append((W, H))
    return out


def layout(W, H, levels):
    """(widths, heights, offsets, total), offsets and total in pixels."""
    sizes = level_sizes(W, H, levels)
    off, run = [], 0
    for w, h in sizes:
        off.append(run)
        run += w * h
    return [w for w, _ in sizes], [h for _, h in sizes], off, run


def bright(rgba, s, threshold, cap):
    """b of a frame float32[H, W, 4] -> float32[H, W, 3]."""
    rgba = f32(rgba)
    c = rgba[..., :3]
    with np.errstate(**_err):
        c0 = np.where(c > F(0.0), c, F(0.0)).astype(np.float32)
        v = (c0 * F(s)).astype(np.float32)
        e = (v - F(threshold)).astype(np.float32)
        b = np.where(e > F(0.0), e, F(0.0)).astype(np.float32)
        b = np.where(b < F(cap), b, F(cap)).astype(np.float32)
        cov = rgba[..., 3] > F(0.0)
    return np.where(cov[..., None], b, F(0.0)).astype(np.float32)


def box(p):
    p = f32(p)
    h, w = p.shape[:2]
    X, Y = np.arange((w + 1) // 2), np.arange((h + 1) // 2)
    x0, x1 = 2 * X, np.minimum(2 * X + 1, w - 1)
    y0, y1 = 2 * Y, np.minimum(2 * Y + 1, h - 1)
    top = (p[y0][:, x0] + p[y0][:, x1]).astype(np.float32)
    bot = (p[y1][:, x0] + p[y1][:, x1]).astype(np.float32)
    return (F(0.25) * (top + bot).astype(np.float32)).astype(np.float32)


def _blur_axis(p, axis):
    n = p.shape[axis]
    i = np.arange(n)
    t = lambda d: np.take(p, np.clip(i + d, 0, n - 1), axis=axis)
    a = (t(-2) + t(2)).astype(np.float32)
    q = (t(-1) + t(1)).astype(np.float32)
    pa = (a * F(0.0625)).astype(np.float32)
    pq = (q * F(0.25)).astype(np.float32)
    pc = (t(0) * F(0.375)).astype(np.float32)
    return ((pa + pq).astype(np.float32) + pc).astype(np.float32)


def blur(p):
    """G of a plane: the horizontal pass, then the vertical pass over its result."""
    return _blur_axis(_blur_axis(f32(p), 1), 0)


def up(u, Wf, Hf):
    """up(u) at every pixel of a fine plane Wf x Hf."""
    u = f32(u)
    h, w = u.shape[:2]
    X, Y = np.arange(Wf), np.arange(Hf)
    cx, cy = X >> 1, Y >> 1
    nx = np.where(X & 1, np.minimum(cx + 1, w - 1), np.maximum(cx - 1, 0))
    ny = np.where(Y & 1, np.minimum(cy + 1, h - 1), np.maximum(cy - 1, 0))
    a = (F(0.5625) * u[cy][:, cx]).astype(np.float32)
    b = (F(0.1875) * u[cy][:, nx]).astype(np.float32)
    c = (F(0.1875) * u[ny][:, cx]).astype(np.float32)
    d = (F(0.0625) * u[ny][:, nx]).astype(np.float32)
    return ((a + b).astype(np.float32) + (c + d).astype(np.float32)).astype(np.float32)


def pyramid_of_bright(b, levels):
    """[U_1, ..., U_levels] from a bright plane float32[H, W, 3]."""
    G, p = [], f32(b)
    for _ in range(levels):
        p = box(p)
        G.append(blur(p))
    U = [None] * levels
    U[levels - 1] = G[levels - 1]
    for k in range(levels - 2, -1, -1):
        h, w = G[k].shape[:2]
        U[k] = (G[k] + up(U[k + 1], w, h)).astype(np.float32)
    return U


def pyramid(rgba, s, levels, threshold, cap):
    return pyramid_of_bright(bright(rgba, s, threshold, cap), levels)


def stored(U):
    """float32[total, 4]: the planes one after the other, the fourth float +0.0f."""
    out = np.zeros((sum(u.shape[0] * u.shape[1] for u in U), 4), np.float32)
    at = 0
    for u in U:
        n = u.shape[0] * u.shape[1]
        out[at:at + n, :3] = u.reshape(n, 3)
        at += n
    return out


def composite(rgba, U1, s, intensity, rule, op, white2=1.0):
    """uint32[H, W]: step 7 of a frame float32[H, W, 4] with level 1 of its pyramid."""
    rgba = f32(rgba)
    H, W = rgba.shape[:2]
    g = up(U1, W, H)
    c = rgba[..., :3]
    with np.errstate(**_err):
        base = np.where(c > F(0.0), c, F(0.0)).astype(np.float32) if rule == RULE_RAST else c
        v = (base * F(s)).astype(np.float32)
        m = (F(intensity) * g).astype(np.float32)
        v2 = (v + m).astype(np.float32)
        px = hdr_ref.put_pixels(hdr_ref.tone(op, v2, white2))
        if rule == RULE_RAST:
            px = np.where(rgba[..., 3] > F(0.0), px, np.uint32(0)).astype(np.uint32)
    return px


def frame(rgba, s, levels, threshold, cap, intensity, rule, op, white2=1.0):
    """(stored pyramid, composite) of one frame."""
    U = pyramid(rgba, s, levels, threshold, cap)
    return stored(U), composite(rgba, U[0], s, intensity, rule, op, white2)


# ---- inputs shared by the CPU and GPU tests ------------------------------------------------

# W x H of the contract's size list: single pixels and rows, odd sizes, sizes around the kernels'
# 32 x 8 blur tile and the 256-lane workgroup, long thin frames either way
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 4), (8, 8), (33, 17), (63, 65), (64, 64), (65, 63), (127, 35), (130, 67),
         (259, 129), (517, 70), (2051, 9), (9, 2051)]
SCALES = [1.0, 0.37, 5.5, 0.0, -2.0, np.inf, np.nan, 2.0 ** -20, 3.0e38]
