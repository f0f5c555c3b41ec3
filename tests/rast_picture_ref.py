"""The rasteriser's float picture restated from the oracle's planes: the vec3 that the reference
gives PutPixelSDL, antiAliasing(y, x) (rasteriser skeleton.cpp:305, :1736-1753), evaluated in raster
order while the darkening of :286-303 has reached only the pixel itself and its upper and left
neighbours.  Nothing here needs a GPU, and the oracle is used as it is:

1. full = the oracle's Draw of the clipped list with buffers: the three shade buffers as they stand
   when Draw returns (every marked interior pixel darkened), the marks, the ARGB frame.
2. lit = the same Draw without the list's shadow-volume triangles (color.x < 0).  Those only set
   shadowBuffer and never touch depth, screen or the rand() order, so lit's screen buffer is the
   screen buffer before any darkening.
3. dk = each interior pixel's darkening from full's marks, exactly as :286-303 / :1725-1733 compute
   it: the sum has [y+1][x-1] twice and [y+1][x+1] never, float(k) / 9.0f in float32, compared as a
   double with 0.6, 0.7, 0.8, 0.9.
4. picture: screen taps centre, up, left from full (darkened), down, right from lit (not yet);
   low and high taps from full; ((((c + up) + down) + left) + right) / 5.0f per buffer, (val + val1)
   + val2, / 3.0f, every step rounded to float32.

`picture()` returns the self-checks' counts beside the picture; tests/test_rast_picture.py holds them
to zero on the CPU, which ties this restatement to the oracle and through it to the reference's
recorded runs.  hdr_ref supplies PutPixelSDL, the histogram, the exposure chain and the pack."""
import ctypes as C

import numpy as np

import hdr_ref
import oracle

F = np.float32


def lit_list(tris, n):
    """(RastTri array, count): the clipped list without its shadow-volume triangles."""
    keep = [i for i in range(n) if not tris[i].color.x < 0]
    out = (oracle.RastTri * max(len(keep), 1))()
    for k, i in enumerate(keep):
        C.memmove(C.byref(out, k * C.sizeof(oracle.RastTri)), C.byref(tris, i * C.sizeof(oracle.RastTri)),
                  C.sizeof(oracle.RastTri))
    return out, len(keep)


def darkening(shadow):
    """float32[H, W]: what :286-303 subtract from each interior pixel (0 where no mark is set)."""
    s = np.asarray(shadow, np.int32)
    H, W = s.shape
    dk = np.zeros((H, W), np.float32)
    c = s[1:-1, 1:-1]
    k = (c + s[:-2, 1:-1] + s[:-2, :-2] + s[:-2, 2:] + s[2:, :-2] + s[2:, 1:-1] + s[2:, :-2] + s[1:-1, :-2]
         + s[1:-1, 2:])
    val = (k.astype(np.float32) / F(9.0)).astype(np.float32).astype(np.float64)
    amount = np.where(val < 0.6, F(0.05), np.where(val < 0.7, F(0.08), np.where(val < 0.8, F(0.1),
                      np.where(val < 0.9, F(0.12), F(0.3))))).astype(np.float32)
    dk[1:-1, 1:-1] = np.where(c == 1, amount, F(0.0))
    return dk


def _five(c, up, down, left, right):
    with np.errstate(all="ignore"):
        s = (c + up).astype(np.float32)
        s = (s + down).astype(np.float32)
        s = (s + left).astype(np.float32)
        s = (s + right).astype(np.float32)
        return (s / F(5.0)).astype(np.float32)


def _taps(a):
    """centre, up, down, left, right of every interior pixel of a[H, W, 3]."""
    return a[1:-1, 1:-1], a[:-2, 1:-1], a[2:, 1:-1], a[1:-1, :-2], a[1:-1, 2:]


def picture_of(p, tris, n, light):
    """(rgba float32[H, W, 4], full, checks) of the clipped list's Draw.  full: the oracle's planes
    and "n_shaded", the fragments that drew rand() values.  checks: counts that must all be zero --`lit_marks`, `low` / `high` / `depth` (lit against full, bit patterns),
    `darken` (lit.screen - dk against full.screen on the marked pixels), `argb` (PutPixelSDL of the
    picture against full's frame inside), `border` (full's frame on the border) -- and `marked`, the
    number of marked interior pixels."""
    H, W = p.height, p.width
    full, cnt = oracle.rast_draw_list(p, tris, n, light, counters=True, buffers=True)
    full["n_shaded"] = int(cnt.n_shaded)                # fragments that drew rand() values (colour modes 1-2)
    lt, nl = lit_list(tris, n)
    lit = oracle.rast_draw_list(p, lt, nl, light, buffers=True)
    sh = full["shadow"].reshape(H, W)
    fs, ls = full["screen"].reshape(H, W, 3), lit["screen"].reshape(H, W, 3)
    lo, hi = full["low"].reshape(H, W, 3), full["high"].reshape(H, W, 3)
    dk = darkening(sh)
    marked = np.zeros((H, W), bool)
    marked[1:-1, 1:-1] = sh[1:-1, 1:-1] == 1
    with np.errstate(all="ignore"):
        darkened = (ls - dk[:, :, None]).astype(np.float32)
    bits = hdr_ref.bits
    checks = dict(
        lit_marks=int(np.count_nonzero(lit["shadow"])),
        low=int((bits(lit["low"]) != bits(full["low"])).sum()),
        high=int((bits(lit["high"]) != bits(full["high"])).sum()),
        depth=int((bits(lit["depth"]) != bits(full["depth"])).sum()),
        darken=int((bits(darkened)[marked] != bits(fs)[marked]).sum()),
        marked=int(marked.sum()),
    )
    c, up, _, left, _ = _taps(fs)
    _, _, down, _, right = _taps(ls)
    val = _five(c, up, down, left, right)
    val1 = _five(*_taps(lo))
    val2 = _five(*_taps(hi))
    with np.errstate(all="ignore"):
        s = (val + val1).astype(np.float32)
        s = (s + val2).astype(np.float32)
        out = (s / F(3.0)).astype(np.float32)
    rgba = np.zeros((H, W, 4), np.float32)
    rgba[1:-1, 1:-1, :3] = out
    rgba[1:-1, 1:-1, 3] = F(1.0)
    argb = full["argb"].reshape(H, W)
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    checks["argb"] = int((hdr_ref.put_pixels(rgba[..., :3])[inner] != argb[inner]).sum())
    checks["border"] = int(np.count_nonzero(argb[~inner]))
    return rgba, full, checks


def picture(p, scene=None):
    """picture_of over Draw's own geometry: p an oracle.RastParams, scene as oracle.rast_geometry."""
    tris, n, light = oracle.rast_geometry(p, scene)
    return picture_of(p, tris, n, light)


def clean(checks):
    return all(v == 0 for k, v in checks.items() if k != "marked")


def pack(rgba, scale, op=hdr_ref.TONE_LINEAR, white2=1.0):
    """The rasteriser's pack: hdr_ref.pack of the channels clamped as c > 0 ? c : 0, and 0 where
    !(w > 0)."""
    rgba = hdr_ref.f32(rgba)
    with np.errstate(all="ignore"):
        c0 = np.where(rgba[..., :3] > F(0.0), rgba[..., :3], F(0.0)).astype(np.float32)
        cov = rgba[..., 3] > F(0.0)
    return np.where(cov, hdr_ref.pack(c0, scale, op, white2), np.uint32(0)).astype(np.uint32)
