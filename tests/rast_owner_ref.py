"""The owner rule of the rasteriser's ordered z-buffer restated over the oracle's exposed
primitives (tests/test_rast_buffers.py proves it against cgo_rast_draw; tests/
test_rast_buffers_gpu.py checks the GPU's clip / pos / tri planes against it).

The owner of a pixel is the fragment that last wrote screenBuffer[y][x] in the reference's
drawing order (rasteriser/Source/skeleton.cpp:574-661): triangles in list order, rows top to
bottom, the first N - 1 pixels of each line left to right."""
import ctypes as C

import numpy as np

import cgamd
import oracle

PIXEL = np.dtype([("x", "<i4"), ("y", "<i4"), ("zinv", "<f4"), ("pos", "<f4", 4)])
assert PIXEL.itemsize == C.sizeof(oracle.Pixel) == 28
INT_MAX = 2**31 - 1


def _lib():
    lib = oracle.load()
    # exposed by the oracle, not declared by its Python loader
    lib.cgo_rast_vertex_shader.restype = None
    lib.cgo_rast_vertex_shader.argtypes = [C.POINTER(oracle.RastParams), oracle.V4, C.POINTER(oracle.Pixel)]
    return lib


def oracle_params(p):
    """The oracle's parameter record with a cgamd.RastParams' width, height and focal length
    (all VertexShader reads)."""
    return oracle.rast_params(p.width, p.height, p.focal)


def triangle_lines(lib, po, T):
    """The lines DrawPolygonRows interpolates for one triangle: PIXEL arrays of N samples each, of
    which the first N - 1 are drawn (:504).  Sentinel rows are skipped."""
    vp = (oracle.Pixel * 3)()
    for k, v in enumerate((T.v0, T.v1, T.v2)):
        lib.cgo_rast_vertex_shader(C.byref(po), oracle.V4(v.x, v.y, v.z, v.w), C.byref(vp[k]))
    rows = lib.cgo_rast_polygon_rows(vp, None, None, 0)
    if rows <= 0:
        return
    left, right = (oracle.Pixel * rows)(), (oracle.Pixel * rows)()
    if lib.cgo_rast_polygon_rows(vp, left, right, rows) <= 0:
        return
    H = po.height
    for j in range(rows):
        if left[j].x == INT_MAX or right[j].x == -INT_MAX:
            continue
        if not 0 <= left[j].y < H:          # off screen: PixelShader returns at once (:573)
            continue
        N = right[j].x - left[j].x + 1
        if N < 2:
            continue
        line = (oracle.Pixel * N)()
        lib.cgo_rast_interpolate(left[j], right[j], line, N)
        yield np.frombuffer(line, PIXEL)[:N - 1]


def owner_planes(params, tris, n, W, H, shadow_marks=True):
    """(depth float32, shadow int32, clip int32, pos float32[., 4]) of W * H pixels for an
    untextured clipped list: the ordered z-buffer by hand.  params: the oracle's or cgamd's.
    Without shadow_marks the shadow-volume triangles are skipped (they never own a pixel or
    write depth) and the shadow plane stays zero: for lists whose volumes cover the frame."""
    lib = _lib()
    po = oracle_params(params)
    assert (po.width, po.height) == (W, H)
    depth = np.zeros(W * H, np.float32)
    shadow = np.zeros(W * H, np.int32)
    clip = np.full(W * H, cgamd.RAST_OWNER_NONE, np.int32)
    pos = np.zeros((W * H, 4), np.float32)
    for i in range(n):
        T = tris[i]
        assert T.texture == 0, "untextured lists only"
        shades = T.color.x >= 0
        if not shades and not shadow_marks:
            continue
        for line in triangle_lines(lib, po, T):
            line = line[(line["x"] >= 0) & (line["x"] < W) & (line["y"] >= 0) & (line["y"] < H)]
            if not line.size:
                continue
            o = line["y"].astype(np.int64) * W + line["x"]      # distinct pixels: x steps by one
            if shades:                                          # zinv >= depth: depth, owner, pos
                w = line["zinv"] >= depth[o]
                depth[o[w]] = line["zinv"][w]
                clip[o[w]] = i
                pos[o[w]] = line["pos"][w]
            else:                                               # zinv > depth: the shadow mark
                shadow[o[line["zinv"] > depth[o]]] = 1
    return depth, shadow, clip, pos


def fragment_at(params, T, x, y):
    """pos3d (float32[4]) of the fragment triangle T draws at pixel (x, y), or None if it draws none."""
    lib = _lib()
    for line in triangle_lines(lib, oracle_params(params), T):
        hit = line[(line["x"] == x) & (line["y"] == y)]
        if hit.size:
            return hit["pos"][-1].copy()
    return None


def input_counts(p, room, nr, boxes, nb):
    """Clipped triangles each input leaves, in list order: room triangle k alone, then boxes[k]
    alone (with its six shadow-volume triangles) -- host-only cg_rast_prepare calls."""
    lib = cgamd.load()
    light = cgamd.Vec4()
    one = lambda arr, k: C.cast(C.byref(arr, k * C.sizeof(cgamd.RTri)), C.POINTER(cgamd.RTri))   # noqa: E731
    counts = [lib.cg_rast_prepare(C.byref(p), one(room, k), 1, boxes, 0, None, 0, C.byref(light)) for k in range(nr)]
    counts += [lib.cg_rast_prepare(C.byref(p), room, 0, one(boxes, k), 1, None, 0, C.byref(light)) for k in range(nb)]
    assert min(counts, default=0) >= 0
    return np.array(counts, np.int64)


def input_of_clip(p, room, nr, boxes, nb):
    """int32[n_clipped]: the input triangle of each clipped triangle (room k -> k, boxes[k] -> nr + k)."""
    counts = input_counts(p, room, nr, boxes, nb)
    return np.repeat(np.arange(nr + nb, dtype=np.int32), counts)
