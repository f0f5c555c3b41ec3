"""ctypes binding of the MI355X renderer's C-ABI (include/cg_render.h).

This is harness plumbing for tests/ and bench.py; the product host surface is
the C++ in host/ (the reference's Draw(screen*) shape).  Loading fails loudly
when libcgamd.so is missing: there is no CPU fallback anywhere on the product
path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CGAMD_LIB") or os.path.join(HERE, "_build", "libcgamd.so")

CG_OK, CG_E_INVALID, CG_E_NODEVICE, CG_E_HIP, CG_E_NOSCENE, CG_E_CAPACITY, CG_E_TIMEOUT = 0, -1, -2, -3, -4, -5, -6


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Vec4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Tri(C.Structure):        # raytracer Triangle, 76 B
    _fields_ = [("v0", Vec4), ("v1", Vec4), ("v2", Vec4), ("normal", Vec4), ("color", Vec3)]


class Sphere(C.Structure):     # 44 B
    _fields_ = [("radius", C.c_float), ("radiusSquared", C.c_float), ("centre", Vec3),
                ("color", Vec3), ("normal", Vec3)]


class Light(C.Structure):      # 28 B
    _fields_ = [("position", Vec4), ("colour", Vec3)]


class Isect(C.Structure):      # Intersection, 28 B
    _fields_ = [("position", Vec4), ("distance", C.c_float), ("triangleIndex", C.c_int),
                ("sphereIndex", C.c_int)]


class RtCamera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("focal", C.c_float), ("camera", Vec4),
                ("R", C.c_float * 16), ("indirect", C.c_float)]


class RtShard(C.Structure):
    """Stripes (rows == 0): RtShard(rank, nranks, stripe_h).  Band: RtShard(row0=a, rows=n).
    RGB24 window: col0=, cols= (see cg_render.h)."""
    _fields_ = [("rank", C.c_int), ("nranks", C.c_int), ("stripe_h", C.c_int), ("row0", C.c_int),
                ("rows", C.c_int), ("col0", C.c_int), ("cols", C.c_int)]


PIX_ARGB8888, PIX_RGB24, PIX_RGBA_F32 = 0, 1, 2   # cg_render.h CG_PIX_*
TONE_LINEAR, TONE_REINHARD, TONE_REINHARD_WHITE = 0, 1, 2   # cg_render.h CG_TONE_*
HDR_BINS = 256


class HdrStats(C.Structure):           # cg_hdr_stats, 32 B
    _fields_ = [("n_counted", C.c_uint32), ("n_dark", C.c_uint32), ("n_uncovered", C.c_uint32),
                ("max_bits", C.c_uint32), ("min_bits", C.c_uint32), ("pad", C.c_uint32 * 3)]


HDR_STATS_DTYPE = np.dtype([("n_counted", "<u4"), ("n_dark", "<u4"), ("n_uncovered", "<u4"), ("max_bits", "<u4"),
                            ("min_bits", "<u4"), ("pad", "<u4", 3)])


class HdrExposureParams(C.Structure):  # cg_hdr_exposure_params
    _fields_ = [("permille", C.c_int), ("target", C.c_float), ("scale_min", C.c_float), ("scale_max", C.c_float),
                ("rate", C.c_float)]


def hdr_params(permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16, rate=1.0):
    return HdrExposureParams(permille, target, scale_min, scale_max, rate)


BLOOM_MAX_LEVELS, BLOOM_RULE_RT, BLOOM_RULE_RAST = 6, 0, 1   # cg_render.h CG_BLOOM_*


class HdrBloomParams(C.Structure):     # cg_hdr_bloom_params, 16 B
    _fields_ = [("levels", C.c_int), ("threshold", C.c_float), ("cap", C.c_float), ("intensity", C.c_float)]


def hdr_bloom_params(levels=4, threshold=1.0, cap=64.0, intensity=0.25):
    return HdrBloomParams(levels, threshold, cap, intensity)


class JpegParams(C.Structure):         # cg_jpeg_params
    _fields_ = [("quality", C.c_int), ("subsampling", C.c_int)]


JPEG_444, JPEG_420 = 0, 2                  # Pillow's subsampling numbers


class PngParams(C.Structure):          # cg_png_params
    _fields_ = [("colour", C.c_int), ("filter", C.c_int)]


PNG_RGB, PNG_RGBA = 2, 6                   # PNG's colour types
PNG_FILTER_ADAPTIVE = -1                   # or a fixed PNG filter type 0 .. 4


class ExrParams(C.Structure):          # cg_exr_params
    _fields_ = [("channels", C.c_int), ("type", C.c_int), ("compression", C.c_int), ("alpha_scale", C.c_float)]


EXR_RGB, EXR_RGBA = 3, 4                   # the channels of an EXR file
EXR_HALF, EXR_FLOAT = 1, 2                 # OpenEXR's pixel types
EXR_NONE, EXR_ZIP = 0, 3                   # OpenEXR's compression numbers


class RTri(C.Structure):       # rasteriser Triangle, 84 B
    _fields_ = [("v0", Vec4), ("v1", Vec4), ("v2", Vec4), ("normal", Vec4), ("color", Vec3),
                ("texture", C.c_int), ("index", C.c_int)]


class RastParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("focal", C.c_float), ("camera", Vec4),
                ("R", C.c_float * 16), ("light_scene", Vec4), ("light_power", Vec3),
                ("indirect_first", C.c_float), ("colour_mode", C.c_int), ("yaw", C.c_float),
                ("rand_offset", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("n_tris", C.c_int),
                ("n_spans", C.c_int), ("n_shaded", C.c_longlong)]


class RastSeqFrame(C.Structure):   # cg_rast_seq_frame: one record of a frame sequence's d_info
    _fields_ = [("rand_offset", C.c_uint64), ("n_shaded", C.c_int64), ("status", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(RastSeqFrame) == 24
assert C.sizeof(Tri) == 76 and C.sizeof(Sphere) == 44 and C.sizeof(Light) == 28
assert C.sizeof(Isect) == 28 and C.sizeof(RTri) == 84

P = C.c_void_p
TEXTURE_MAPS = ("marble", "woven", "woven_ao", "woven_opacity", "woven_normal",
                "grill", "grill_opacity", "grill_normal")
TEXTURE_SHAPES = {"marble": (2000, 2000, 3)}   # the rest 1024 x 1024 x 3 (BGR)


class RastTextures(C.Structure):   # cg_rast_textures
    _fields_ = [(n, C.c_void_p) for n in TEXTURE_MAPS]


# cg_rast_buffers: the planes of a buffers call, (name, numpy dtype, values per pixel) in the
# structure's order; a null pointer = not asked for
RAST_PLANES = (("argb", np.uint32, 1), ("depth", np.float32, 1), ("shadow", np.int32, 1),
               ("screen", np.float32, 3), ("low", np.float32, 3), ("high", np.float32, 3),
               ("clip", np.int32, 1), ("tri", np.int32, 1), ("pos", np.float32, 4))
RAST_OWNER_NONE = -1


class RastBuffers(C.Structure):    # cg_rast_buffers
    _fields_ = [(n, C.c_void_p) for n, _, _ in RAST_PLANES]


def rast_buffers_planes(params, want):
    """Host planes of a buffers call (no device work): (RastBuffers, {name: array}) for the plane
    names in `want`, each W * H rows of its values (RAST_PLANES)."""
    names = [n for n, _, _ in RAST_PLANES]
    bad = [w for w in want if w not in names]
    if bad:
        raise ValueError(f"no such rasteriser plane: {bad} (one of {names})")
    npx = params.width * params.height
    out, b = {}, RastBuffers()
    for n, dt, k in RAST_PLANES:
        if n in want:
            out[n] = np.zeros(npx if k == 1 else (npx, k), dt)
            setattr(b, n, out[n].ctypes.data)
    return b, out


_SIGS = {
    "cg_create": (C.c_int, [C.c_int, C.POINTER(P)]),
    "cg_destroy": (None, [P]),
    "cg_last_error": (C.c_char_p, [P]),
    "cg_device_count": (C.c_int, []),
    "cg_debug_live": (C.c_int, [C.POINTER(C.c_longlong)]),
    "cg_rt_load_test_model": (C.c_int, [C.POINTER(Tri), C.c_int, C.POINTER(Sphere)]),
    "cg_glibc_rand": (C.c_int, [C.c_uint64, C.c_int, P]),
    "cg_starfield_init": (C.c_int, [P, C.c_int]),
    "cg_starfield_update": (C.c_int, [P, C.c_int, C.c_float]),
    "cg_starfield_draw": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P]),
    "cg_starfield_set": (C.c_int, [P, P, C.c_int]),
    "cg_starfield_get": (C.c_int, [P, P, C.c_int]),
    "cg_starfield_run_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_size_t, P]),
    "cg_starfield_advance_device": (C.c_int, [P, P, C.c_int, P]),
    "cg_starfield_run": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_size_t, C.c_int,
                                   C.POINTER(Stats)]),
    "cg_starfield_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_rt_area_lights": (C.c_int, [C.POINTER(Light), C.c_float, C.c_int, C.POINTER(Light), C.c_int]),
    "cg_rt_random_scene": (C.c_int, [C.c_uint64, C.c_int, C.POINTER(Tri)]),
    "cg_rt_set_scene": (C.c_int, [P, C.POINTER(Tri), C.c_int, C.POINTER(Sphere), C.c_int]),
    "cg_rt_set_scene_device": (C.c_int, [P, P, C.c_int, C.POINTER(Sphere), C.c_int, P]),
    "cg_rt_set_grid_caps": (C.c_int, [P, C.c_longlong, C.c_longlong]),
    "cg_rt_grid_dims": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "cg_rt_grid_get": (C.c_int, [P, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), P, C.c_size_t, P,
                                 C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "cg_rt_grid_info": (C.c_int, [P, C.POINTER(C.c_uint64)]),
    "cg_rt_grid_phase_ms": (C.c_int, [P, C.POINTER(C.c_double)]),
    "cg_rt_set_pending_cap": (C.c_int, [P, C.c_int]),
    "cg_rt_scratch_info": (C.c_int, [P, C.POINTER(C.c_uint64)]),
    "cg_rt_pool_demand": (C.c_int, [P, C.POINTER(C.c_uint64)]),
    "cg_rt_tile_masks": (C.c_int, [P, C.c_int, P, P, C.POINTER(C.c_int)]),
    "cg_rt_lattice_path": (C.c_int, [P, C.POINTER(C.c_int)]),
    "cg_rt_route": (C.c_int, [C.POINTER(RtCamera), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cg_rt_set_pool_caps": (C.c_int, [P, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong]),
    "cg_rt_render_brute_device": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, C.c_int, P, P]),
    "cg_rt_render": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), P, C.POINTER(Stats)]),
    "cg_rt_render_frames": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, P,
                                      C.c_size_t, C.c_int, C.POINTER(Stats)]),
    "cg_kernel_timing": (C.c_int, [C.c_int]),
    "cg_kernel_time": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "cg_rt_render_device": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera),
                                      C.POINTER(RtShard), P, P]),
    "cg_rt_render_frames_device": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int,
                                             C.POINTER(RtShard), P, C.c_size_t, C.c_int, P]),
    "cg_rt_render_sequence_device": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int,
                                               C.POINTER(RtShard), P, C.c_size_t, C.c_int, P]),
    "cg_pix_bytes": (C.c_int, [C.c_int]),
    "cg_rt_render_radiance": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), P, C.POINTER(Stats)]),
    "cg_rt_pack_radiance_device": (C.c_int, [P, P, C.c_size_t, C.c_float, P, P]),
    "cg_hdr_luminance": (C.c_float, [C.c_float, C.c_float, C.c_float]),
    "cg_hdr_bin": (C.c_int, [C.c_float]),
    "cg_hdr_bin_edge": (C.c_float, [C.c_int]),
    "cg_hdr_exposure": (C.c_int, [P, C.c_int, C.POINTER(HdrExposureParams), P, P]),
    "cg_hdr_tone": (C.c_float, [C.c_int, C.c_float, C.c_float]),
    "cg_hdr_histogram_device": (C.c_int, [P, P, C.c_int, C.c_size_t, C.c_int, C.c_size_t, P, P, P]),
    "cg_hdr_exposure_device": (C.c_int, [P, P, C.c_int, C.POINTER(HdrExposureParams), P, P, P]),
    "cg_rt_tonemap_pack_device": (C.c_int, [P, P, C.c_size_t, C.c_int, C.c_size_t, P, C.c_int, C.c_float, P,
                                            C.c_size_t, P]),
    "cg_rt_render_exposed_device": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, C.c_int,
                                              C.POINTER(HdrExposureParams), P, C.c_int, C.c_float, P, C.c_size_t, P,
                                              P]),
    "cg_rt_render_exposed": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, C.c_int,
                                       C.POINTER(HdrExposureParams), P, C.c_int, C.c_float, P, C.c_size_t, P,
                                       C.POINTER(Stats)]),
    "cg_hdr_bloom_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "cg_hdr_bloom": (C.c_int, [P, C.c_int, C.c_int, C.c_float, C.POINTER(HdrBloomParams), P]),
    "cg_hdr_bloom_pack": (C.c_int, [P, P, C.c_int, C.c_int, C.c_float, C.POINTER(HdrBloomParams), C.c_int, C.c_int,
                                    C.c_float, P]),
    "cg_hdr_bloom_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_size_t, P, C.POINTER(HdrBloomParams), P,
                                      C.c_size_t, P]),
    "cg_hdr_bloom_pack_device": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, P,
                                           C.POINTER(HdrBloomParams), C.c_int, C.c_int, C.c_float, P, C.c_size_t, P]),
    "cg_rt_render_exposed_bloom_device": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int,
                                                    C.c_int, C.POINTER(HdrExposureParams), P, C.c_int, C.c_float,
                                                    C.POINTER(HdrBloomParams), P, C.c_size_t, P, P]),
    "cg_rt_render_exposed_bloom": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, C.c_int,
                                             C.POINTER(HdrExposureParams), P, C.c_int, C.c_float,
                                             C.POINTER(HdrBloomParams), P, C.c_size_t, P, C.POINTER(Stats)]),
    "cg_rt_render_sequence": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, P,
                                        C.c_size_t, C.c_int, C.POINTER(Stats)]),
    "cg_rt_sequence_runs": (C.c_int, [C.POINTER(RtCamera), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RtShard),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "cg_rt_assemble_device": (C.c_int, [P, P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                        C.c_int, C.c_int, P, C.c_size_t, C.c_int, C.c_int, P]),
    "cg_rt_frame_columns": (C.c_int, [C.POINTER(Tri), C.c_int, C.POINTER(Sphere), C.c_int, C.POINTER(RtCamera),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_rt_shard_rows": (C.c_int, [C.c_int, C.POINTER(RtShard)]),
    "cg_rt_unstripe_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "cg_rt_unstripe_batch_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "cg_rt_pixel_ray": (C.c_int, [C.POINTER(RtCamera), C.c_int, C.c_int, C.c_int, C.POINTER(Vec4), C.POINTER(Vec4)]),
    "cg_rt_hits_device": (C.c_int, [P, C.POINTER(RtCamera), C.c_int, C.c_void_p, P, P, P, P]),
    "cg_rt_hits": (C.c_int, [P, C.POINTER(RtCamera), C.c_int, P, P, P]),
    "cg_rt_pick": (C.c_int, [P, C.POINTER(RtCamera), C.c_int, C.c_int, C.c_int, C.POINTER(Isect),
                             C.POINTER(C.c_int)]),
    "cg_rt_probe_closest": (C.c_int, [P, C.POINTER(Vec4), C.POINTER(Vec4), C.c_int,
                                      C.POINTER(Isect), C.POINTER(C.c_int)]),
    "cg_rt_probe_direct_light": (C.c_int, [P, C.POINTER(Isect), C.POINTER(Light), C.c_int,
                                           C.POINTER(Vec3)]),
    "cg_rt_probe_div3_device": (C.c_int, [P, P, C.c_int, P, P]),
    "cg_rt_probe_rmag_device": (C.c_int, [P, C.c_int, P, P]),
    "cg_rast_load_test_model": (C.c_int, [C.POINTER(RTri), C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(RTri), C.c_int, C.POINTER(C.c_int)]),
    "cg_rast_prepare": (C.c_int, [C.POINTER(RastParams), C.POINTER(RTri), C.c_int, C.POINTER(RTri),
                                  C.c_int, C.POINTER(RTri), C.c_int, C.POINTER(Vec4)]),
    "cg_rast_render": (C.c_int, [P, C.POINTER(RTri), C.c_int, C.POINTER(RastParams), Vec4, P, P, P,
                                 C.POINTER(Stats)]),
    "cg_rast_render_device": (C.c_int, [P, P, C.c_int, C.POINTER(RastParams), Vec4, P, P, P, P]),
    "cg_rast_set_scene": (C.c_int, [P, C.POINTER(RTri), C.c_int, C.POINTER(RTri), C.c_int]),
    "cg_rast_set_textures": (C.c_int, [P, C.POINTER(RastTextures)]),
    "cg_rast_opacity_map": (C.c_int, [P, C.c_int, P]),
    "cg_rast_draw": (C.c_int, [P, C.POINTER(RastParams), P, P, P, C.POINTER(Stats)]),
    "cg_rast_draw_device": (C.c_int, [P, C.POINTER(RastParams), P, P, P, P]),
    "cg_rast_draw_frames_device": (C.c_int, [P, C.POINTER(RastParams), C.c_int, P, P, P, C.c_size_t, P]),
    "cg_rast_draw_sequence_device": (C.c_int, [P, C.POINTER(RastParams), C.c_int, P, P, P, C.c_size_t, P, P]),
    "cg_rast_draw_sequence": (C.c_int, [P, C.POINTER(RastParams), C.c_int, P, P, P, C.c_size_t, C.c_int,
                                        C.POINTER(RastSeqFrame), C.POINTER(Stats)]),
    "cg_rast_set_rand_capacity": (C.c_int, [P, C.c_longlong]),
    "cg_rast_draw_picture_device": (C.c_int, [P, C.POINTER(RastParams), P, P, P, P]),
    "cg_rast_draw_picture": (C.c_int, [P, C.POINTER(RastParams), P, C.POINTER(Stats)]),
    "cg_rast_draw_sequence_picture_device": (C.c_int, [P, C.POINTER(RastParams), C.c_int, P, P, P, C.c_size_t, P,
                                                       P]),
    "cg_rast_tonemap_pack_device": (C.c_int, [P, P, C.c_size_t, C.c_int, C.c_size_t, P, C.c_int, C.c_float, P,
                                              C.c_size_t, P]),
    "cg_rast_pack_pixel": (C.c_uint32, [P, C.c_float, C.c_int, C.c_float]),
    "cg_rast_draw_exposed_device": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(HdrExposureParams), P,
                                              C.c_int, C.c_float, P, C.c_size_t, P, P, P]),
    "cg_rast_draw_exposed": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(HdrExposureParams), P, C.c_int,
                                       C.c_float, P, C.c_size_t, P, C.POINTER(RastSeqFrame), C.POINTER(Stats)]),
    "cg_rast_draw_exposed_bloom_device": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(HdrExposureParams),
                                                    P, C.c_int, C.c_float, C.POINTER(HdrBloomParams), P, C.c_size_t, P,
                                                    P, P]),
    "cg_rast_draw_exposed_bloom": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(HdrExposureParams), P,
                                             C.c_int, C.c_float, C.POINTER(HdrBloomParams), P, C.c_size_t, P,
                                             C.POINTER(RastSeqFrame), C.POINTER(Stats)]),
    "cg_rast_route": (C.c_int, [C.c_longlong]),
    "cg_rast_set_route": (C.c_int, [P, C.c_int]),
    "cg_rast_set_route_limit": (C.c_int, [P, C.c_longlong]),
    "cg_rast_span_segments": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "cg_rast_scratch_info": (C.c_int, [P, C.POINTER(C.c_uint64)]),
    "cg_rast_row_blocks": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_rast_random_scene": (C.c_int, [C.c_uint64, C.c_int, C.c_float, C.POINTER(RTri)]),
    "cg_glibc_rand_device": (C.c_int, [P, P, C.c_int, P, P]),
    "cg_rast_draw_buffers_device": (C.c_int, [P, C.POINTER(RastParams), C.POINTER(RastBuffers), P]),
    "cg_rast_draw_buffers": (C.c_int, [P, C.POINTER(RastParams), C.POINTER(RastBuffers), C.POINTER(Stats)]),
    "cg_rast_render_buffers_device": (C.c_int, [P, P, C.c_int, C.POINTER(RastParams), Vec4,
                                                C.POINTER(RastBuffers), P]),
    "cg_rast_render_buffers": (C.c_int, [P, C.POINTER(RTri), C.c_int, C.POINTER(RastParams), Vec4,
                                         C.POINTER(RastBuffers), C.POINTER(Stats)]),
    "cg_rast_pick": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.c_int, C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32), C.POINTER(Vec4), C.POINTER(C.c_int)]),
    "cg_rast_state_bytes": (C.c_int, [P]),
    "cg_dist_unique_id": (C.c_int, [P]),
    "cg_dist_create": (C.c_int, [P, C.c_int, C.c_int, P, C.POINTER(P)]),
    "cg_dist_create_timed": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, C.POINTER(P)]),
    "cg_dist_set_timeout": (C.c_int, [P, C.c_int]),
    "cg_dist_wait": (C.c_int, [P, P]),
    "cg_dist_create_local": (C.c_int, [C.POINTER(P), C.c_int, C.POINTER(P)]),
    "cg_dist_destroy": (None, [P]),
    "cg_dist_set_bands": (C.c_int, [P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_dist_get_bands": (C.c_int, [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_dist_set_chunk": (C.c_int, [P, C.c_int]),
    "cg_dist_set_pipeline": (C.c_int, [P, C.c_int]),
    "cg_dist_rebalance": (C.c_int, [P]),
    "cg_dist_last_times": (C.c_int, [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cg_rt_render_frames_dist": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int, P,
                                           C.c_size_t, P]),
    "cg_dist_band_partition": (C.c_int, [P, C.c_int, C.c_int, P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_image_jpeg_info": (C.c_int, [P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_image_jpeg_check": (C.c_int, [P, C.c_size_t]),
    "cg_image_decode_jpeg": (C.c_int, [P, P, C.c_size_t, P, C.c_size_t]),
    "cg_image_decode_jpeg_device": (C.c_int, [P, P, C.c_size_t, P, C.c_size_t, P]),
    "cg_image_encode_jpeg_host": (C.c_int, [P, C.c_int, C.c_int, C.c_size_t, C.POINTER(JpegParams), P, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "cg_image_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.POINTER(JpegParams), P, C.c_size_t]),
    "cg_image_jpeg_bound": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "cg_image_jpeg_enc_limits": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_image_encode_jpeg_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(JpegParams), P,
                                              C.c_size_t, P, P]),
    "cg_image_encode_jpeg": (C.c_int, [P, P, C.c_int, C.c_int, C.c_size_t, C.POINTER(JpegParams), P, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "cg_rt_render_sequence_jpeg": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int,
                                             C.POINTER(JpegParams), P, C.c_size_t, C.POINTER(C.c_size_t), C.c_int,
                                             C.POINTER(Stats)]),
    "cg_rast_draw_sequence_jpeg": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(JpegParams), P, C.c_size_t,
                                             C.POINTER(C.c_size_t), C.c_int, C.POINTER(RastSeqFrame), C.POINTER(Stats)]),
    "cg_image_encode_png_host": (C.c_int, [P, C.c_int, C.c_int, C.c_size_t, C.POINTER(PngParams), P, C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "cg_image_png_bound": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "cg_image_png_code_lengths": (C.c_int, [P, C.c_int, C.c_int, P]),
    "cg_image_png_enc_limits": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_image_encode_png_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(PngParams), P,
                                             C.c_size_t, P, P]),
    "cg_image_encode_png": (C.c_int, [P, P, C.c_int, C.c_int, C.c_size_t, C.POINTER(PngParams), P, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "cg_rt_render_sequence_png": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int,
                                            C.POINTER(PngParams), P, C.c_size_t, C.POINTER(C.c_size_t), C.c_int,
                                            C.POINTER(Stats)]),
    "cg_rast_draw_sequence_png": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(PngParams), P, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.c_int, C.POINTER(RastSeqFrame), C.POINTER(Stats)]),
    "cg_image_encode_exr_host": (C.c_int, [P, C.c_int, C.c_int, C.c_size_t, C.POINTER(ExrParams), P, C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "cg_image_exr_bound": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "cg_image_exr_header": (C.c_int, [C.c_int, C.c_int, C.POINTER(ExrParams), P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "cg_image_exr_half": (C.c_int, [P, C.c_int, P]),
    "cg_image_exr_enc_limits": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cg_image_encode_exr_device": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(ExrParams), P,
                                             C.c_size_t, P, P]),
    "cg_image_encode_exr": (C.c_int, [P, P, C.c_int, C.c_int, C.c_size_t, C.POINTER(ExrParams), P, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "cg_rt_render_sequence_exr": (C.c_int, [P, C.POINTER(Light), C.c_int, C.POINTER(RtCamera), C.c_int,
                                            C.POINTER(ExrParams), P, C.c_size_t, C.POINTER(C.c_size_t), C.c_int,
                                            C.POINTER(Stats)]),
    "cg_rast_draw_sequence_exr": (C.c_int, [P, C.POINTER(RastParams), C.c_int, C.POINTER(ExrParams), P, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.c_int, C.POINTER(RastSeqFrame), C.POINTER(Stats)]),
}
EXPORTS = tuple(_SIGS)

# skeleton.cpp:135-146: the file each cg_rast_textures map is read from
TEXTURE_FILES = {"marble": "Marble2000x2000.jpg", "woven": "woven1024x1024.jpg",
                 "woven_ao": "Wood_wicker_003_ambientOcclusion.jpg",
                 "woven_opacity": "Wood_wicker_003_opacity.jpg", "woven_normal": "Wood_wicker_003_normal.jpg",
                 "grill": "Metal_Grill_002_basecolor.jpg", "grill_opacity": "Metal_Grill_002_opacity.jpg",
                 "grill_normal": "Metal_Grill_002_normal.jpg"}

_lib = None


def load(path: str = LIB_PATH):
    """Load libcgamd.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libcgamd.so not built at {path}; run __graft_entry__.build()")
    try:   # one HIP runtime per process: torch's (it bundles libamdhip64) must load first
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def identity16():
    return (C.c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])


def yaw_matrix(yaw: float):
    """R for a yaw angle exactly as Update() sets it (RT skeleton.cpp:236-238):
    R[0][0]=cos R[0][2]=-sin R[2][0]=sin R[2][2]=cos, float32 cos/sin."""
    y = np.float32(yaw)
    c, s = np.cos(y, dtype=np.float32), np.sin(y, dtype=np.float32)
    m = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    m[0 * 4 + 0], m[0 * 4 + 2] = float(c), float(-s)
    m[2 * 4 + 0], m[2 * 4 + 2] = float(s), float(c)
    return (C.c_float * 16)(*m)


def pix_bytes(pix_format):
    """cg_pix_bytes: bytes per pixel of a PIX_* format (host-only; no GPU needed)."""
    n = load().cg_pix_bytes(pix_format)
    if n < 0:
        raise ValueError(f"pix_format {pix_format}")
    return n


def hdr_luminance(x, y, z):
    """cg_hdr_luminance elementwise: (0.2126 x + 0.7152 y) + 0.0722 z in float32 (host-only; no GPU needed)."""
    lib = load()
    x, y, z = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(z, np.float32))
    out = np.empty(x.shape, np.float32)
    for i, (a, b, c) in enumerate(zip(x.ravel().tolist(), y.ravel().tolist(), z.ravel().tolist())):
        out.flat[i] = lib.cg_hdr_luminance(a, b, c)
    return out


def _f32_arg(bits):
    """A float32 bit pattern as a ctypes argument: through c_float's buffer, so that a NaN keeps its payload."""
    return C.c_float.from_buffer_copy(np.uint32(bits).tobytes())


def hdr_bin(L):
    """cg_hdr_bin elementwise: the histogram bin of a luminance, -1 when it is not counted."""
    lib = load()
    L = np.asarray(L, np.float32)
    out = np.empty(L.shape, np.int32)
    for i, b in enumerate(L.ravel().view(np.uint32).tolist()):
        out.flat[i] = lib.cg_hdr_bin(_f32_arg(b))
    return out


def hdr_bin_edge(b):
    """cg_hdr_bin_edge elementwise: the upper edge of bins 0 .. 255."""
    lib = load()
    b = np.asarray(b, np.int32)
    if ((b < 0) | (b >= HDR_BINS)).any():
        raise ValueError("bin outside 0..255")
    out = np.empty(b.shape, np.float32)
    for i, v in enumerate(b.ravel().tolist()):
        out.flat[i] = lib.cg_hdr_bin_edge(v)
    return out


def hdr_tone(op, v, white2=1.0):
    """cg_hdr_tone elementwise."""
    lib = load()
    v = np.asarray(v, np.float32)
    out = np.empty(v.shape, np.float32)
    for i, b in enumerate(v.ravel().view(np.uint32).tolist()):
        out.flat[i] = lib.cg_hdr_tone(op, _f32_arg(b), white2)
    return out


def rast_pack_pixel(rgba, scale=1.0, op=TONE_LINEAR, white2=1.0):
    """cg_rast_pack_pixel over float32[..., 4] pixels: the rasteriser's pack of each (an uncovered
    pixel, !(w > 0), gives 0; a channel that is not positive is 0 before the scale) as uint32[...]
    (host-only; no GPU needed).  The scale passes by bit pattern, the pixels by address."""
    lib = load()
    px = np.ascontiguousarray(rgba, np.float32)
    if px.shape[-1:] != (4,):
        raise ValueError("pixels of four floats")
    out = np.empty(px.shape[:-1], np.uint32)
    flat = px.reshape(-1, 4)
    s = _f32_arg(np.float32(scale).view(np.uint32))
    base = flat.ctypes.data
    for i in range(len(flat)):
        out.flat[i] = lib.cg_rast_pack_pixel(P(base + 16 * i), s, op, white2)
    return out


def hdr_exposure(hist, params=None, prev=None, **kw):
    """cg_hdr_exposure: the scales s_f of histograms uint32[n, 256] (params: HdrExposureParams, or
    hdr_params' keywords; prev: the previous scale or None)."""
    lib = load()
    params = hdr_params(**kw) if params is None else params
    hist = np.ascontiguousarray(hist, np.uint32).reshape(-1, HDR_BINS)
    scales = np.zeros(len(hist), np.float32)
    pv = None if prev is None else np.array([prev], np.float32)
    rc = lib.cg_hdr_exposure(hist.ctypes.data_as(P), len(hist), C.byref(params),
                             pv.ctypes.data_as(P) if pv is not None else None, scales.ctypes.data_as(P))
    if rc:
        raise ValueError(f"cg_hdr_exposure: {rc}")
    return scales


def hdr_bloom_layout(width, height, levels):
    """cg_hdr_bloom_layout: (widths, heights, offsets, total) of levels 1 .. levels, offsets and total
    in pixels (host-only; no GPU needed)."""
    n = max(int(levels), 1)
    w, h, off, total = (C.c_int * n)(), (C.c_int * n)(), (C.c_size_t * n)(), C.c_size_t(0)
    rc = load().cg_hdr_bloom_layout(width, height, levels, w, h, off, C.byref(total))
    if rc < 1 or rc != levels:
        raise ValueError(f"cg_hdr_bloom_layout: {rc}")
    return list(w), list(h), list(off), total.value


def _bloom_arg(bloom, kw):
    return hdr_bloom_params(**kw) if bloom is None else bloom


def hdr_bloom(rgba, scale=1.0, bloom=None, **kw):
    """cg_hdr_bloom: the pyramid float32[total, 4] of one frame float32[H, W, 4] (bloom: HdrBloomParams,
    or hdr_bloom_params' keywords).  The scale passes by bit pattern (host-only; no GPU needed)."""
    bloom = _bloom_arg(bloom, kw)
    px = np.ascontiguousarray(rgba, np.float32)
    if px.ndim != 3 or px.shape[2] != 4:
        raise ValueError("a frame float32[H, W, 4]")
    H, W = px.shape[:2]
    total = hdr_bloom_layout(W, H, bloom.levels)[3]
    pyr = np.empty((total, 4), np.float32)
    rc = load().cg_hdr_bloom(px.ctypes.data_as(P), W, H, _f32_arg(np.float32(scale).view(np.uint32)), C.byref(bloom),
                             pyr.ctypes.data_as(P))
    if rc:
        raise ValueError(f"cg_hdr_bloom: {rc}")
    return pyr


def hdr_bloom_pack(rgba, pyr, scale=1.0, bloom=None, rule=BLOOM_RULE_RT, op=TONE_LINEAR, white2=1.0, **kw):
    """cg_hdr_bloom_pack: the composite uint32[H, W] of one frame float32[H, W, 4] and its pyramid."""
    bloom = _bloom_arg(bloom, kw)
    px = np.ascontiguousarray(rgba, np.float32)
    if px.ndim != 3 or px.shape[2] != 4:
        raise ValueError("a frame float32[H, W, 4]")
    H, W = px.shape[:2]
    total = hdr_bloom_layout(W, H, bloom.levels)[3]
    pyr = np.ascontiguousarray(pyr, np.float32)
    if pyr.size < total * 4:
        raise ValueError("a pyramid of float32[total, 4]")
    out = np.empty((H, W), np.uint32)
    rc = load().cg_hdr_bloom_pack(px.ctypes.data_as(P), pyr.ctypes.data_as(P), W, H,
                                  _f32_arg(np.float32(scale).view(np.uint32)), C.byref(bloom), rule, op, white2,
                                  out.ctypes.data_as(P))
    if rc:
        raise ValueError(f"cg_hdr_bloom_pack: {rc}")
    return out


ROUTES = ("pixel", "lattice", "lattice_yaw", "lights", "lights_yaw", "big_pixel", "big_lattice", "big_lattice_yaw")


def rt_route(cam, n_tris, n_spheres, n_lights, shard=None):
    """cg_rt_route: the kernels a frame of this shape takes (host-only; no GPU
    needed), as a name from ROUTES."""
    lib = load()
    rc = lib.cg_rt_route(C.byref(cam), n_tris, n_spheres, n_lights, C.cast(C.byref(shard), C.c_void_p) if shard else None)
    if rc < 0:
        raise ValueError(f"cg_rt_route: {rc}")
    return ROUTES[rc]


def rt_sequence_runs(cams, n_tris, n_spheres, n_lights, shard=None):
    """cg_rt_sequence_runs: how a frame sequence is launched (host-only; no GPU needed), as a
    list of (start, stop, route name): consecutive frames on the same route form a run."""
    lib = load()
    arr = (RtCamera * max(len(cams), 1))(*cams)
    sh = C.byref(shard) if shard is not None else None
    cap = 8
    while True:
        start, route = (C.c_int * (cap + 1))(), (C.c_int * cap)()
        n = lib.cg_rt_sequence_runs(arr, len(cams), n_tris, n_spheres, n_lights, sh, start, route, cap)
        if n < 0:
            raise ValueError(f"cg_rt_sequence_runs: {n}")
        if n <= cap:
            return [(start[r], start[r + 1], ROUTES[route[r]]) for r in range(n)]
        cap = n


def sequence_lights(lights_per_frame):
    """A sequence's lights as one Light array, frame-major, and the common count per frame:
    lights_per_frame is a list of per-frame light lists (or Light arrays) of equal length."""
    n = len(lights_per_frame[0]) if len(lights_per_frame) else 0
    if any(len(fl) != n for fl in lights_per_frame):
        raise ValueError("every frame of a sequence has the same number of lights")
    arr = (Light * max(len(lights_per_frame) * n, 1))()
    for f, fl in enumerate(lights_per_frame):
        for k in range(n):
            arr[f * n + k].position = fl[k].position
            arr[f * n + k].colour = fl[k].colour
    return arr, n


def rt_camera(width, height, focal=256.0, cam=(0.0, 0.0, -3.0, 1.0), R=None, indirect=0.5):
    c = RtCamera()
    c.width, c.height, c.focal = width, height, focal
    c.camera = Vec4(*cam)
    c.R = R if R is not None else identity16()
    c.indirect = indirect
    return c


HIT_NONE = -(1 << 31)   # cg_render.h CG_RT_HIT_NONE
# cg_isect as a numpy record: 28 B, the reference's Intersection
ISECT_DTYPE = np.dtype([("position", np.float32, 4), ("distance", np.float32), ("triangleIndex", np.int32),
                        ("sphereIndex", np.int32)])
assert ISECT_DTYPE.itemsize == C.sizeof(Isect)


def rt_pixel_ray(cam, x, y, sub_ray=4):
    """cg_rt_pixel_ray (host-only; no GPU needed): (start, dir) of pixel (x, y)'s sub-ray as two
    float32[4] arrays; ValueError for a pixel outside the frame or a sub-ray outside 0..8."""
    s, d = Vec4(), Vec4()
    rc = load().cg_rt_pixel_ray(C.byref(cam), x, y, sub_ray, C.byref(s), C.byref(d))
    if rc != CG_OK:
        raise ValueError(f"cg_rt_pixel_ray: {rc}")
    return (np.array([s.x, s.y, s.z, s.w], np.float32), np.array([d.x, d.y, d.z, d.w], np.float32))


def rt_pixel_rays(cam, sub_ray=4, pixels=None):
    """cg_rt_pixel_ray for many pixels: (starts, dirs) as float32[n, 4]; pixels an iterable of flat
    indices y * W + x (None: the whole frame, row-major)."""
    lib, W = load(), cam.width
    idx = range(W * cam.height) if pixels is None else [int(p) for p in pixels]
    n = len(idx)
    starts, dirs = np.zeros((max(n, 1), 4), np.float32), np.zeros((max(n, 1), 4), np.float32)
    ps, pd = C.cast(starts.ctypes.data, C.POINTER(Vec4)), C.cast(dirs.ctypes.data, C.POINTER(Vec4))
    fn, pc = lib.cg_rt_pixel_ray, C.byref(cam)
    for k, p in enumerate(idx):
        if fn(pc, p % W, p // W, sub_ray, C.byref(ps[k]), C.byref(pd[k])) != CG_OK:
            raise ValueError(f"cg_rt_pixel_ray: pixel {p}, sub-ray {sub_ray}")
    return starts[:n], dirs[:n]


def default_lights():
    """skeleton.cpp:86-89: one light at (0,-0.5,-0.7), colour 14*(1,1,1)."""
    arr = (Light * 1)()
    arr[0].position = Vec4(0.0, -0.5, -0.7, 1.0)
    f = float(np.float32(14.0) * np.float32(1.0))
    arr[0].colour = Vec3(f, f, f)
    return arr


def area_lights(centre=None, side=0.1, n=8):
    """C4 soft-shadow light set (cg_rt_area_lights): n*n lights, default around
    the reference light (skeleton.cpp:86-89)."""
    lib = load()
    c = default_lights()[0] if centre is None else centre
    out = (Light * (n * n))()
    k = lib.cg_rt_area_lights(C.byref(c), side, n, out, n * n)
    if k != n * n:
        raise RuntimeError(f"cg_rt_area_lights failed: {k}")
    return out


def glibc_rand(offset, n):
    """cg_glibc_rand: n values of glibc rand() from call `offset` (seed 1)."""
    lib = load()
    out = np.zeros(max(n, 1), np.int32)
    rc = lib.cg_glibc_rand(offset, n, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise RuntimeError(f"cg_glibc_rand failed: {rc}")
    return out[:n]


def starfield_init(n=1000):
    """cg_starfield_init: (n, 3) float32 stars (starfield/Source/skeleton.cpp:41-46)."""
    st = np.zeros((n, 3), np.float32)
    rc = load().cg_starfield_init(st.ctypes.data_as(C.c_void_p), n)
    if rc:
        raise RuntimeError(f"cg_starfield_init failed: {rc}")
    return st


def starfield_update(stars, dt):
    rc = load().cg_starfield_update(stars.ctypes.data_as(C.c_void_p), len(stars), dt)
    if rc:
        raise RuntimeError(f"cg_starfield_update failed: {rc}")


def starfield_plan(n_stars, n_frames):
    """cg_starfield_plan: how a run of n_frames frames is cut (host-only; no GPU needed), as
    (launches, frames_per_launch, frames_per_block)."""
    L, B = C.c_int(), C.c_int()
    n = load().cg_starfield_plan(n_stars, n_frames, C.byref(L), C.byref(B))
    if n < 0:
        raise ValueError(f"cg_starfield_plan: {n}")
    return n, L.value, B.value


def _dts(dts):
    return np.ascontiguousarray(dts, np.float32).reshape(-1)


def random_scene(n, seed=0x5EED):
    """C5 random triangles (cg_rt_random_scene): ctypes Tri array of n."""
    lib = load()
    tris = (Tri * max(n, 1))()
    k = lib.cg_rt_random_scene(seed, n, tris)
    if k != n:
        raise RuntimeError(f"cg_rt_random_scene failed: {k}")
    return tris


RAST_ROUTE_DENSE, RAST_ROUTE_COMPACT = 0, 1   # cg_render.h CG_RAST_ROUTE_*


def rt_grid_dims(vmin, vmax, n_tris):
    """cg_rt_grid_dims (host only): the scene grid's frame from the float vertex minimum / maximum
    per axis and the triangle count, as dict(lo float32[3], h, inv_h float32, res int[3]), or None
    for "no grid"."""
    lib = load()
    lo, res = (C.c_float * 3)(), (C.c_int * 3)()
    h, inv_h = C.c_float(), C.c_float()
    rc = lib.cg_rt_grid_dims((C.c_float * 3)(*vmin), (C.c_float * 3)(*vmax), n_tris, lo, C.byref(h), C.byref(inv_h), res)
    if rc < 0:
        raise RuntimeError(f"cg_rt_grid_dims failed: {rc}")
    if rc == 0:
        return None
    return dict(lo=np.array(lo[:], np.float32), h=np.float32(h.value), inv_h=np.float32(inv_h.value),
                res=np.array(res[:], np.int32))


def rast_route(list_capacity):
    """cg_rast_route (host-only): the route a frame of this list capacity takes automatically."""
    return load().cg_rast_route(list_capacity)


def rast_span_segments(lx, rx, width):
    """cg_rast_span_segments (host-only): (count, first) of the 64-pixel fill segments a span's visible extent overlaps."""
    first = C.c_int(0)
    n = load().cg_rast_span_segments(lx, rx, width, C.byref(first))
    return n, first.value


def rast_row_blocks():
    """cg_rast_row_blocks (host-only): (batch, chunk), the block sizes of the compact route's row-list passes."""
    b, c = C.c_int(), C.c_int()
    if load().cg_rast_row_blocks(C.byref(b), C.byref(c)) != CG_OK:
        raise RuntimeError("cg_rast_row_blocks failed")
    return b.value, c.value


def rast_random_scene(n, extent=0.02, seed=0x5EED):
    """cg_rast_random_scene (host-only): ctypes RTri array of n random triangles."""
    tris = (RTri * max(n, 1))()
    k = load().cg_rast_random_scene(seed, n, extent, tris)
    if k != n:
        raise RuntimeError(f"cg_rast_random_scene failed: {k}")
    return tris


def rast_params(width, height, focal=512.0, cam=(0.0, 0.0, -3.001, 1.0), R=None,
                light=(0.0, -0.5, 0.0, 1.0), indirect_first=0.2, colour_mode=0, rand_offset=0, yaw=0.0):
    p = RastParams()
    p.width, p.height, p.focal = width, height, focal
    p.camera = Vec4(*cam)
    p.R = (C.c_float * 16)(*R) if R is not None else identity16()
    p.light_scene = Vec4(*light)
    f = float(np.float32(20.0) * np.float32(1.0))
    p.light_power = Vec3(f, f, f)
    p.indirect_first = indirect_first
    p.colour_mode = colour_mode
    p.rand_offset = rand_offset
    p.yaw = yaw
    return p


# cg_rast_seq_frame as a numpy record (rast_draw_sequence's info)
RAST_SEQ_DTYPE = np.dtype([("rand_offset", "<u8"), ("n_shaded", "<i8"), ("status", "<i4"), ("pad", "<i4")])


def rast_sequence_planes(params_list, out=None, want_depth=False, want_shadow=False, chunk=0, frame_stride=0):
    """Argument checks and host planes of Context.rast_draw_sequence (no device work):
    -> (stride, argb, depth, shadow), None for a plane not asked for.  out / want_depth /
    want_shadow may each be a destination of 4-byte elements (numpy array or torch CPU tensor,
    pageable or pinned); True allocates one.  The C entry has no capacity argument, so a
    destination shorter than (n - 1) * stride + W * H pixels is refused here."""
    n = len(params_list)
    if not 0 <= chunk <= 64:
        raise ValueError(f"chunk {chunk}: 0 (= 8) to 64")
    npx = params_list[0].width * params_list[0].height if n else 0
    stride = frame_stride or npx
    if stride < npx:
        raise ValueError(f"frame_stride {stride} < W*H = {npx}")
    if any((p.width, p.height) != (params_list[0].width, params_list[0].height) for p in params_list):
        raise ValueError("frames of one size")
    need = (n - 1) * stride + npx if n else 0

    def plane(want, dtype, what):
        if want is None or want is False:
            return None
        if want is True:
            return np.zeros(n * stride, dtype)
        isnp = isinstance(want, np.ndarray)
        if (want.itemsize if isnp else want.element_size()) != 4:
            raise ValueError(f"{what}: 4-byte elements")
        if not (want.flags["C_CONTIGUOUS"] if isnp else want.is_contiguous()):
            raise ValueError(f"{what}: contiguous memory")
        have = want.size if isnp else want.numel()
        if have < need:
            raise ValueError(f"{what} holds {have} pixels, {n} frames at stride {stride} need {need}")
        return want

    return (stride, plane(True if out is None else out, np.uint32, "out"), plane(want_depth, np.float32, "depth"),
            plane(want_shadow, np.int32, "shadow"))


def opacity_map(bgr):
    """cg_rast_opacity_map (host-only): BGR texels -> 0/255 bytes."""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    out = np.zeros(a.size // 3, np.uint8)
    rc = load().cg_rast_opacity_map(a.ctypes.data_as(P), out.size, out.ctypes.data_as(P))
    if rc != CG_OK:
        raise RuntimeError(f"cg_rast_opacity_map failed with {rc}")
    return out


def frame_columns(tris, n, sph, n_sph, cam):
    """cg_rt_frame_columns: the columns [c0, c1) an unrotated camera can see anything in."""
    lib = load()
    c0, c1 = C.c_int(), C.c_int()
    rc = lib.cg_rt_frame_columns(tris, n, sph, n_sph, C.byref(cam), C.byref(c0), C.byref(c1))
    if rc != CG_OK:
        raise RuntimeError(f"cg_rt_frame_columns failed with {rc}")
    return c0.value, c1.value


def probe_div3_device(d_x, d_den, n, d_q, stream=None):
    """cg_rt_probe_div3_device: d_q[3i + k] = d_x[3i + k] / d_den[i] as the light-set sweep divides
    (device pointers; asynchronous on `stream`)."""
    if load().cg_rt_probe_div3_device(P(d_x), P(d_den), n, P(d_q), P(stream) if stream else None) != CG_OK:
        raise RuntimeError("cg_rt_probe_div3_device failed")


def probe_rmag_device(d_r, n, d_m, stream=None):
    """cg_rt_probe_rmag_device: d_m[i] = the FP64 norm of the float triple d_r[3i .. 3i + 2], rounded
    to float, as the one-light lattice kernels form it (device pointers; asynchronous on `stream`)."""
    if load().cg_rt_probe_rmag_device(P(d_r), n, P(d_m), P(stream) if stream else None) != CG_OK:
        raise RuntimeError("cg_rt_probe_rmag_device failed")


def kernel_timing(enable: bool):
    """cg_kernel_timing: start (reset) or stop the live per-kernel HIP-event timing."""
    if load().cg_kernel_timing(1 if enable else 0) != CG_OK:
        raise RuntimeError("cg_kernel_timing failed")


def kernel_time(kernel: str):
    """(total ms, busy ms, launches) of one timed kernel since kernel_timing(True); busy counts
    overlapping launches (two frames in flight) once."""
    ms, busy, n = C.c_double(), C.c_double(), C.c_longlong()
    if load().cg_kernel_time(kernel.encode(), C.byref(ms), C.byref(busy), C.byref(n)) != CG_OK:
        raise ValueError(f"cg_kernel_time: {kernel} is not a timed kernel")
    return ms.value, busy.value, n.value


def rt_scene():
    lib = load()
    tris = (Tri * 64)()
    sph = Sphere()
    n = lib.cg_rt_load_test_model(tris, 64, C.byref(sph))
    if n < 0:
        raise RuntimeError(f"cg_rt_load_test_model failed: {n}")
    return tris, n, sph


def rast_scene(setting=0, setting_boxes=0):
    """LoadTestModel; setting / setting_boxes are the texture selectors of the
    room and the boxes (TestModelH.h:9-10: 0 none, 1 marble, 2 grill, 3 woven)."""
    lib = load()
    room, boxes = (RTri * 16)(), (RTri * 32)()
    nr, nb = C.c_int(), C.c_int()
    rc = lib.cg_rast_load_test_model(room, 16, C.byref(nr), boxes, 32, C.byref(nb))
    if rc < 0:
        raise RuntimeError(f"cg_rast_load_test_model failed: {rc}")
    for i in range(nr.value):
        room[i].texture = setting
    for i in range(nb.value):
        boxes[i].texture = setting_boxes
    return room, nr.value, boxes, nb.value


def rast_prepare(params, room=None, nr=None, boxes=None, nb=None):
    """Host geometry (clip etc.): returns (clipped RTri array, n, light Vec4)."""
    lib = load()
    if room is None:
        room, nr, boxes, nb = rast_scene()
    light = Vec4()
    n = lib.cg_rast_prepare(C.byref(params), room, nr, boxes, nb, None, 0, C.byref(light))
    if n < 0:
        raise RuntimeError(f"cg_rast_prepare failed: {n}")
    out = (RTri * max(n, 1))()
    n = lib.cg_rast_prepare(C.byref(params), room, nr, boxes, nb, out, n, C.byref(light))
    return out, n, light



def jpeg_info(data: bytes):
    """(width, height, channels) of a JPEG file's bytes (host-only, no GPU)."""
    lib = load()
    buf = np.frombuffer(data, np.uint8)
    w, h, ch = C.c_int(), C.c_int(), C.c_int()
    if lib.cg_image_jpeg_info(buf.ctypes.data_as(P), buf.size, C.byref(w), C.byref(h), C.byref(ch)) != 0:
        raise ValueError("not a supported JPEG")
    return w.value, h.value, ch.value


def image_jpeg_bound(width, height, subsampling=JPEG_420) -> int:
    """cg_image_jpeg_bound: a length no JPEG file of the size can exceed (host-only)."""
    n = load().cg_image_jpeg_bound(width, height, subsampling)
    if n < 0:
        raise ValueError(f"cg_image_jpeg_bound({width}, {height}, {subsampling}) failed ({n})")
    return n


def image_jpeg_header(width, height, quality=75, subsampling=JPEG_420) -> bytes:
    """cg_image_jpeg_header: the bytes before the scan (host-only)."""
    buf = np.zeros(1024, np.uint8)
    prm = JpegParams(quality, subsampling)
    n = load().cg_image_jpeg_header(width, height, C.byref(prm), buf.ctypes.data_as(P), buf.size)
    if n < 0:
        raise ValueError(f"cg_image_jpeg_header failed ({n})")
    return buf[:n].tobytes()


def image_jpeg_enc_limits():
    """cg_image_jpeg_enc_limits: (lanes of an entropy workgroup, bytes of an interval it holds in LDS)."""
    t, b = C.c_int(), C.c_int()
    load().cg_image_jpeg_enc_limits(C.byref(t), C.byref(b))
    return t.value, b.value


def _jpeg_frame(argb):
    a = np.ascontiguousarray(argb, dtype=np.uint32)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("argb: a uint32 array (H, W)")
    return a


def _jpeg_encode(fn, what, argb, quality, subsampling):
    a = _jpeg_frame(argb)
    h, w = a.shape
    prm = JpegParams(quality, subsampling)
    n = C.c_size_t()
    out = np.empty(max(4096, w * h), np.uint8)
    rc = fn(a.ctypes.data_as(P), w, h, 0, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc == CG_E_CAPACITY:
        out = np.empty(n.value, np.uint8)
        rc = fn(a.ctypes.data_as(P), w, h, 0, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc != CG_OK:
        raise ValueError(f"{what} failed ({rc})")
    return out[:n.value].tobytes()


def image_encode_jpeg_host(argb, quality=75, subsampling=JPEG_420) -> bytes:
    """cg_image_encode_jpeg_host: the baseline JPEG file of a uint32 (H, W) ARGB8888 frame, the bytes
    Pillow writes at that quality and subsampling with restart_marker_rows=1 (host-only, no GPU)."""
    return _jpeg_encode(load().cg_image_encode_jpeg_host, "cg_image_encode_jpeg_host", argb, quality, subsampling)


def image_png_bound(width, height, colour=PNG_RGB) -> int:
    """cg_image_png_bound: a length no PNG file of the size can exceed (host-only)."""
    n = load().cg_image_png_bound(width, height, colour)
    if n < 0:
        raise ValueError(f"cg_image_png_bound({width}, {height}, {colour}) failed ({n})")
    return n


def image_png_enc_limits():
    """cg_image_png_enc_limits: (lanes of a band workgroup, bytes of a band's bit string it holds in LDS)."""
    t, b = C.c_int(), C.c_int()
    load().cg_image_png_enc_limits(C.byref(t), C.byref(b))
    return t.value, b.value


def image_png_code_lengths(freq, limit) -> np.ndarray:
    """cg_image_png_code_lengths: the encoder's code lengths (uint8) for frequencies under a length limit."""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(max(f.size, 1), np.uint8)
    rc = load().cg_image_png_code_lengths(f.ctypes.data_as(P), f.size, limit, out.ctypes.data_as(P))
    if rc != CG_OK:
        raise ValueError(f"cg_image_png_code_lengths failed ({rc})")
    return out[:f.size]


def _png_encode(fn, what, argb, colour, filter):
    a = _jpeg_frame(argb)
    h, w = a.shape
    prm = PngParams(colour, filter)
    n = C.c_size_t()
    out = np.empty(max(4096, w * h), np.uint8)
    rc = fn(a.ctypes.data_as(P), w, h, 0, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc == CG_E_CAPACITY:
        out = np.empty(n.value, np.uint8)
        rc = fn(a.ctypes.data_as(P), w, h, 0, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc != CG_OK:
        raise ValueError(f"{what} failed ({rc})")
    return out[:n.value].tobytes()


def image_encode_png_host(argb, colour=PNG_RGB, filter=PNG_FILTER_ADAPTIVE) -> bytes:
    """cg_image_encode_png_host: the PNG file of a uint32 (H, W) ARGB8888 frame under the library's own
    contract (include/cg_render.h); any PNG decoder returns the pixels (host-only, no GPU)."""
    return _png_encode(load().cg_image_encode_png_host, "cg_image_encode_png_host", argb, colour, filter)


def image_exr_bound(width, height, channels=EXR_RGBA, type=EXR_HALF) -> int:
    """cg_image_exr_bound: a NONE file's exact length, which no ZIP file of the size exceeds (host-only)."""
    n = load().cg_image_exr_bound(width, height, channels, type)
    if n < 0:
        raise ValueError(f"cg_image_exr_bound({width}, {height}, {channels}, {type}) failed ({n})")
    return n


def image_exr_enc_limits():
    """cg_image_exr_enc_limits: (lanes of a chunk workgroup, bytes of a chunk's bit string it holds in LDS)."""
    t, b = C.c_int(), C.c_int()
    load().cg_image_exr_enc_limits(C.byref(t), C.byref(b))
    return t.value, b.value


def image_exr_header(width, height, channels=EXR_RGBA, type=EXR_HALF, compression=EXR_ZIP) -> bytes:
    """cg_image_exr_header: the header of the EXR file of a picture of that size (host-only)."""
    prm = ExrParams(channels, type, compression, 1.0)
    out = np.empty(512, np.uint8)
    n = C.c_size_t()
    rc = load().cg_image_exr_header(width, height, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc != CG_OK:
        raise ValueError(f"cg_image_exr_header failed ({rc})")
    return out[:n.value].tobytes()


def image_exr_half(values) -> np.ndarray:
    """cg_image_exr_half: the encoder's float32 -> half conversion, as uint16 bits of the input's shape."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(v.shape, np.uint16)
    rc = load().cg_image_exr_half(v.ctypes.data_as(P), v.size, out.ctypes.data_as(P))
    if rc != CG_OK:
        raise ValueError(f"cg_image_exr_half failed ({rc})")
    return out


def _exr_picture(rgba):
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("an EXR picture is a float32 (H, W, 4) array")
    return a


def _exr_encode(fn, what, rgba, channels, type, compression, alpha_scale):
    a = _exr_picture(rgba)
    h, w = a.shape[:2]
    prm = ExrParams(channels, type, compression, alpha_scale)
    n = C.c_size_t()
    out = np.empty(max(4096, w * h * 4), np.uint8)
    rc = fn(a.ctypes.data_as(P), w, h, 0, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc == CG_E_CAPACITY:
        out = np.empty(n.value, np.uint8)
        rc = fn(a.ctypes.data_as(P), w, h, 0, C.byref(prm), out.ctypes.data_as(P), out.size, C.byref(n))
    if rc != CG_OK:
        raise ValueError(f"{what} failed ({rc})")
    return out[:n.value].tobytes()


def image_encode_exr_host(rgba, channels=EXR_RGBA, type=EXR_HALF, compression=EXR_ZIP, alpha_scale=1.0) -> bytes:
    """cg_image_encode_exr_host: the OpenEXR file of a float32 (H, W, 4) picture under the library's own
    contract (include/cg_render.h); any EXR reader returns the samples (host-only, no GPU)."""
    return _exr_encode(load().cg_image_encode_exr_host, "cg_image_encode_exr_host", rgba, channels, type, compression,
                       alpha_scale)


DIST_ID_BYTES = 128   # cg_dist_id (an RCCL unique id)
DIST_SIGNALLED, DIST_CHUNKED = 0, 1   # cg_dist_set_pipeline


def dist_unique_id() -> bytes:
    """cg_dist_unique_id: rank 0 creates the id every rank passes to Dist."""
    buf = (C.c_char * DIST_ID_BYTES)()
    rc = load().cg_dist_unique_id(buf)
    if rc != CG_OK:
        raise RuntimeError(f"cg_dist_unique_id failed with {rc}")
    return bytes(buf.raw)


def band_partition_native(row_cost, nranks, overhead=None):
    """cg_dist_band_partition (host-only): [(row0, rows)] per rank."""
    c = np.ascontiguousarray(row_cost, dtype=np.float64)
    o = None if overhead is None else np.ascontiguousarray(overhead, dtype=np.float64)
    r0, rs = (C.c_int * nranks)(), (C.c_int * nranks)()
    rc = load().cg_dist_band_partition(c.ctypes.data_as(P), len(c), nranks, o.ctypes.data_as(P) if o is not None
                                       else None, r0, rs)
    if rc != CG_OK:
        raise RuntimeError(f"cg_dist_band_partition failed with {rc}")
    return [(r0[r], rs[r]) for r in range(nranks)]


class DistTimeout(RuntimeError):
    """A multi-GPU wait passed its deadline (CG_E_TIMEOUT); the communicator was aborted."""


class Dist:
    """Multi-GPU raytracer frames (cg_dist_*): one rank's handle.  Dist(ctx,
    nranks, rank, id) joins an RCCL communicator; Dist.local(ctxs) builds an
    in-process group (tests) and returns one handle per rank."""

    def __init__(self, ctx, nranks=1, rank=0, uid: bytes = None, _handle=None, timeout_ms=0):
        """timeout_ms: deadline of every host wait on this handle, init included (0: the
        library's default, CG_DIST_TIMEOUT_MS or 60 s); a passed deadline raises
        DistTimeout after the library aborted the communicator."""
        self.ctx, self.lib, self.nranks, self.rank = ctx, ctx.lib, nranks, rank
        if _handle is not None:
            self.h = _handle
            return
        h = P()
        idb = (C.c_char * DIST_ID_BYTES).from_buffer_copy(uid)
        self._check(self.lib.cg_dist_create_timed(ctx.h, nranks, rank, idb, int(timeout_ms), C.byref(h)),
                    "cg_dist_create")
        self.h = h

    def _check(self, rc, what):
        if rc == CG_E_TIMEOUT:
            msg = self.lib.cg_last_error(self.ctx.h)
            raise DistTimeout(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        self.ctx._check(rc, what)

    def set_timeout(self, ms):
        self._check(self.lib.cg_dist_set_timeout(self.h, int(ms)), "cg_dist_set_timeout")

    def wait(self, stream=None):
        """cg_dist_wait: bounded host wait for this rank's enqueued work (raises on a
        timeout or an RCCL error, after the library aborted the communicator)."""
        self._check(self.lib.cg_dist_wait(self.h, P(stream) if stream else None), "cg_dist_wait")

    @classmethod
    def local(cls, ctxs):
        n = len(ctxs)
        hs, outs = (P * n)(*[c.h for c in ctxs]), (P * n)()
        ctxs[0]._check(ctxs[0].lib.cg_dist_create_local(hs, n, outs), "cg_dist_create_local")
        return [cls(ctxs[r], n, r, _handle=P(outs[r])) for r in range(n)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.cg_dist_destroy(self.h)
            self.h = None

    def set_bands(self, height, bands):
        r0 = (C.c_int * self.nranks)(*[b[0] for b in bands])
        rs = (C.c_int * self.nranks)(*[b[1] for b in bands])
        self.ctx._check(self.lib.cg_dist_set_bands(self.h, height, r0, rs), "cg_dist_set_bands")

    def bands(self):
        r0, rs = (C.c_int * self.nranks)(), (C.c_int * self.nranks)()
        rc = self.lib.cg_dist_get_bands(self.h, r0, rs)
        if rc < 0:
            return None
        return [(r0[r], rs[r]) for r in range(self.nranks)]

    def set_chunk(self, frames):
        self.ctx._check(self.lib.cg_dist_set_chunk(self.h, frames), "cg_dist_set_chunk")

    def set_pipeline(self, mode):
        """DIST_SIGNALLED / DIST_CHUNKED (cg_dist_set_pipeline)."""
        self.ctx._check(self.lib.cg_dist_set_pipeline(self.h, mode), "cg_dist_set_pipeline")

    def rebalance(self):
        self._check(self.lib.cg_dist_rebalance(self.h), "cg_dist_rebalance")

    def last_times(self):
        """(render ms per frame, assembly ms per frame) of this rank's last call."""
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.cg_dist_last_times(self.h, C.byref(a), C.byref(b)), "cg_dist_last_times")
        return a.value, b.value

    def render_frames(self, cams, d_frames, stream=None, lights=None, frame_stride=0):
        """cg_rt_render_frames_dist: len(cams) frames, assembled on rank 0 at d_frames."""
        lights = default_lights() if lights is None else lights
        arr = (RtCamera * len(cams))(*cams)
        self._check(self.lib.cg_rt_render_frames_dist(self.h, lights, len(lights), arr, len(cams),
                                                          P(d_frames) if d_frames else None, frame_stride,
                                                          P(stream) if stream else None),
                        "cg_rt_render_frames_dist")


def debug_live():
    """Test hook cg_debug_live: (device allocations, pinned allocations, events, streams) that the
    process's contexts and cg_dist handles hold right now."""
    out = (C.c_longlong * 4)()
    rc = load().cg_debug_live(out)
    if rc != 0:
        raise RuntimeError(f"cg_debug_live failed ({rc})")
    return tuple(out)


class Context:
    """One GPU context (cg_create/cg_destroy)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = P()
        rc = self.lib.cg_create(device, C.byref(h))
        if rc != CG_OK:
            raise RuntimeError(f"cg_create({device}) failed with {rc} (no usable HIP device?)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.cg_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != CG_OK:
            msg = self.lib.cg_last_error(self.h)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    # -- RT --
    def rt_set_scene(self, tris, n, sph=None, n_sph=1):
        sp = C.byref(sph) if sph is not None else None
        self._check(self.lib.cg_rt_set_scene(self.h, tris, n, sp, n_sph if sph is not None else 0),
                    "cg_rt_set_scene")

    def rt_set_scene_device(self, d_tris_ptr, n, sph=None, n_sph=0, stream=None):
        """cg_rt_set_scene_device: n triangles (cg_tri, 76 B each) at the device address d_tris_ptr;
        sph is a host Sphere (n_sph of them), stream a HIP stream handle (None: the context's).
        Raises on any failure, as rt_set_scene does."""
        sp = C.byref(sph) if sph is not None else None
        self._check(self.lib.cg_rt_set_scene_device(self.h, P(d_tris_ptr) if d_tris_ptr else None, n, sp,
                                                    n_sph if sph is not None else 0, P(stream) if stream else None),
                    "cg_rt_set_scene_device")

    def rt_set_grid_caps(self, entries=0, candidates=0):
        """cg_rt_set_grid_caps: caps of the scene grid for later scene changes (0 = default)."""
        self._check(self.lib.cg_rt_set_grid_caps(self.h, entries, candidates), "cg_rt_set_grid_caps")

    def rt_grid(self):
        """cg_rt_grid_get: the installed scene grid as dict(res int32[3], lo float32[3], h float32,
        start int32[cells + 1], tris int32[entries]), or None when the scene has none."""
        res, lo, h = (C.c_int * 3)(), (C.c_float * 3)(), C.c_float()
        ns, ne = C.c_size_t(), C.c_size_t()
        rc = self.lib.cg_rt_grid_get(self.h, res, lo, C.byref(h), None, 0, None, 0, C.byref(ns), C.byref(ne))
        if rc == 0:
            return None
        if rc != 1:
            self._check(rc, "cg_rt_grid_get")
        start = np.zeros(ns.value, np.int32)
        tris = np.zeros(max(ne.value, 1), np.int32)
        rc = self.lib.cg_rt_grid_get(self.h, res, lo, C.byref(h), start.ctypes.data_as(P), start.size,
                                     tris.ctypes.data_as(P), tris.size, C.byref(ns), C.byref(ne))
        if rc != 1:
            self._check(rc if rc < 0 else CG_E_INVALID, "cg_rt_grid_get")
        return dict(res=np.array(res[:], np.int32), lo=np.array(lo[:], np.float32), h=np.float32(h.value),
                    start=start, tris=tris[:ne.value])

    def rt_grid_info(self):
        """cg_rt_grid_info: dict(cells, entries, candidates, bytes) of the latest scene change
        (candidates: pairs the device build tested, 0 after a host build)."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.cg_rt_grid_info(self.h, out), "cg_rt_grid_info")
        return dict(cells=out[0], entries=out[1], candidates=out[2], bytes=out[3])

    def rt_grid_phase_ms(self):
        """cg_rt_grid_phase_ms: device ms of the latest device build's phases, -1 where one did not run."""
        out = (C.c_double * 5)()
        self._check(self.lib.cg_rt_grid_phase_ms(self.h, out), "cg_rt_grid_phase_ms")
        return dict(zip(("bounds", "ranges", "count", "offsets", "fill_order"), out[:]))

    def rt_set_pending_cap(self, cap):
        """Test hook: capacity of the large-scene pending shadow-ray queue (0 = default)."""
        self._check(self.lib.cg_rt_set_pending_cap(self.h, cap), "cg_rt_set_pending_cap")

    def rt_set_pool_caps(self, sup=0, bin=0, sbin=0, sorted=0):
        """Test hook: pin the large-scene pool capacities (all 0 = automatic)."""
        self._check(self.lib.cg_rt_set_pool_caps(self.h, sup, bin, sbin, sorted), "cg_rt_set_pool_caps")

    def rt_render_brute_device(self, cam, row0, rows, d_out, lights=None, stream=None):
        """Test hook cg_rt_render_brute_device: rows row0 .. row0 + rows - 1 of cam's frame into the
        device buffer d_out by the reference's unaccelerated loop (synchronous)."""
        lights = default_lights() if lights is None else lights
        self._check(self.lib.cg_rt_render_brute_device(self.h, lights, len(lights), C.byref(cam), row0, rows, P(d_out),
                                                       P(stream) if stream else None), "cg_rt_render_brute_device")

    def rt_scratch_info(self):
        """Large-scene scratch after the latest frame: dict(bytes, listed, capacity, overflows)."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.cg_rt_scratch_info(self.h, out), "cg_rt_scratch_info")
        return dict(bytes=out[0], listed=out[1], capacity=out[2], overflows=out[3])

    def rt_pool_demand(self):
        """Entries the latest large-scene frame listed per pool: dict(sup, bin, sbin, sorted)."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.cg_rt_pool_demand(self.h, out), "cg_rt_pool_demand")
        return dict(sup=out[0], bin=out[1], sbin=out[2], sorted=out[3])

    def rt_tile_masks(self, frame=0):
        """Diagnostic cg_rt_tile_masks: the latest lattice call's tile certificates of one frame as
        (masks uint64[ty, tx, 2], obj uint64[ty, tx, slots] or None when none were built)."""
        info = (C.c_int * 4)()
        self._check(self.lib.cg_rt_tile_masks(self.h, frame, None, None, info), "cg_rt_tile_masks")
        tx, ty, slots = info[0], info[1], info[2]
        masks = np.zeros((ty, tx, 2), np.uint64)
        obj = np.zeros((ty, tx, slots), np.uint64) if slots else None
        self._check(self.lib.cg_rt_tile_masks(self.h, frame, masks.ctypes.data_as(P),
                                              obj.ctypes.data_as(P) if slots else None, info), "cg_rt_tile_masks")
        return masks, obj

    def rt_lattice_path(self):
        """Diagnostic cg_rt_lattice_path: the latest batched one-light lattice call's (dispatch order,
        published certificates, forced uncertified, workgroups)."""
        info = (C.c_int * 4)()
        self._check(self.lib.cg_rt_lattice_path(self.h, info), "cg_rt_lattice_path")
        return info[0], bool(info[1]), bool(info[2]), info[3]

    def rt_render(self, cam, lights=None, n_lights=None):
        lights = default_lights() if lights is None else lights
        n_lights = len(lights) if n_lights is None else n_lights
        out = np.zeros(cam.width * cam.height, np.uint32)
        st = Stats()
        self._check(self.lib.cg_rt_render(self.h, lights, n_lights, C.byref(cam),
                                          out.ctypes.data_as(P), C.byref(st)), "cg_rt_render")
        return out, st

    def rt_render_radiance(self, cam, lights=None):
        """cg_rt_render_radiance: the frame before PutPixelSDL, float32[H, W, 4] -- x, y, z the
        pixel's sum / 9, w the number of its nine sub-rays that hit (PIX_RGBA_F32)."""
        lights = default_lights() if lights is None else lights
        out = np.zeros((cam.height, cam.width, 4), np.float32)
        st = Stats()
        self._check(self.lib.cg_rt_render_radiance(self.h, lights, len(lights), C.byref(cam), out.ctypes.data_as(P),
                                                   C.byref(st)), "cg_rt_render_radiance")
        return out, st

    def rt_pack_radiance_device(self, d_rgba, n_pixels, d_argb, scale=1.0, stream=None):
        """cg_rt_pack_radiance_device: d_argb[p] = PutPixelSDL(scale * xyz of d_rgba[p])."""
        self._check(self.lib.cg_rt_pack_radiance_device(self.h, P(d_rgba), n_pixels, scale, P(d_argb),
                                                        P(stream) if stream else None),
                    "cg_rt_pack_radiance_device")

    def hdr_histogram_device(self, d_pixels, channels, n_pixels, n_frames, d_hist, d_stats=None, frame_stride=0,
                             stream=None):
        """cg_hdr_histogram_device: d_hist[f * 256 + b] and d_stats[f] of n_frames planes."""
        self._check(self.lib.cg_hdr_histogram_device(self.h, P(d_pixels), channels, n_pixels, n_frames, frame_stride,
                                                     P(d_hist), P(d_stats) if d_stats else None,
                                                     P(stream) if stream else None), "cg_hdr_histogram_device")

    def hdr_exposure_device(self, d_hist, n_frames, params, d_scales, d_prev=None, stream=None):
        """cg_hdr_exposure_device: d_scales[f] = s_f (d_prev: a device float or None)."""
        self._check(self.lib.cg_hdr_exposure_device(self.h, P(d_hist), n_frames, C.byref(params),
                                                    P(d_prev) if d_prev else None, P(d_scales),
                                                    P(stream) if stream else None), "cg_hdr_exposure_device")

    def rt_tonemap_pack_device(self, d_rgba, n_pixels, n_frames, d_scales, d_argb, op=TONE_LINEAR, white2=1.0,
                               src_stride=0, dst_stride=0, stream=None):
        """cg_rt_tonemap_pack_device: d_argb = PutPixelSDL(tone(op, c * d_scales[f])) per frame."""
        self._check(self.lib.cg_rt_tonemap_pack_device(self.h, P(d_rgba), n_pixels, n_frames, src_stride, P(d_scales),
                                                       op, white2, P(d_argb), dst_stride,
                                                       P(stream) if stream else None), "cg_rt_tonemap_pack_device")

    @staticmethod
    def _exposed_lights(cams, lights, per_frame_lights):
        if per_frame_lights:
            if len(lights) != len(cams):
                raise ValueError("one light list per frame")
            return sequence_lights(lights)
        lights = default_lights() if lights is None else lights
        return lights, len(lights)

    def rt_render_exposed_device(self, cams, d_argb, d_scales, params, lights=None, per_frame_lights=False,
                                 d_prev=None, op=TONE_LINEAR, white2=1.0, frame_stride=0, stream=None):
        """cg_rt_render_exposed_device: len(cams) frames rendered, exposed and packed into d_argb +
        f * frame_stride pixels, their scales into d_scales (device memory, no host wait)."""
        larr, n = self._exposed_lights(cams, lights, per_frame_lights)
        arr = (RtCamera * max(len(cams), 1))(*cams)
        self._check(self.lib.cg_rt_render_exposed_device(self.h, larr, n, arr, len(cams), int(bool(per_frame_lights)),
                                                         C.byref(params), P(d_prev) if d_prev else None, op, white2,
                                                         P(d_argb), frame_stride, P(d_scales),
                                                         P(stream) if stream else None),
                    "cg_rt_render_exposed_device")

    def rt_render_exposed(self, cams, lights=None, per_frame_lights=False, permille=990, target=1.0,
                          scale_min=2.0 ** -16, scale_max=2.0 ** 16, rate=1.0, prev=None, op=TONE_LINEAR, white2=1.0):
        """cg_rt_render_exposed: (frames uint32[n, H, W], scales float32[n]) in host memory."""
        n = len(cams)
        if n == 0:
            return np.zeros((0, 0, 0), np.uint32), np.zeros(0, np.float32)
        larr, nl = self._exposed_lights(cams, lights, per_frame_lights)
        arr = (RtCamera * n)(*cams)
        params = hdr_params(permille, target, scale_min, scale_max, rate)
        out = np.zeros((n, cams[0].height, cams[0].width), np.uint32)
        scales = np.zeros(n, np.float32)
        pv = None if prev is None else np.array([prev], np.float32)
        st = Stats()
        self._check(self.lib.cg_rt_render_exposed(self.h, larr, nl, arr, n, int(bool(per_frame_lights)),
                                                  C.byref(params), pv.ctypes.data_as(P) if pv is not None else None,
                                                  op, white2, out.ctypes.data_as(P), 0, scales.ctypes.data_as(P),
                                                  C.byref(st)), "cg_rt_render_exposed")
        return out, scales

    def hdr_bloom_device(self, d_rgba, width, height, n_frames, d_scales, bloom, d_pyr, src_stride=0, pyr_stride=0,
                         stream=None):
        """cg_hdr_bloom_device: the pyramids of n_frames frames into d_pyr + f * pyr_stride pixels."""
        self._check(self.lib.cg_hdr_bloom_device(self.h, P(d_rgba), width, height, n_frames, src_stride, P(d_scales),
                                                 C.byref(bloom), P(d_pyr), pyr_stride,
                                                 P(stream) if stream else None), "cg_hdr_bloom_device")

    def hdr_bloom_pack_device(self, d_rgba, d_pyr, width, height, n_frames, d_scales, bloom, d_argb,
                              rule=BLOOM_RULE_RT, op=TONE_LINEAR, white2=1.0, src_stride=0, pyr_stride=0, dst_stride=0,
                              stream=None):
        """cg_hdr_bloom_pack_device: d_argb = PutPixelSDL(tone(op, base * s + intensity * up(U_1))) per frame."""
        self._check(self.lib.cg_hdr_bloom_pack_device(self.h, P(d_rgba), P(d_pyr), width, height, n_frames, src_stride,
                                                      pyr_stride, P(d_scales), C.byref(bloom), rule, op, white2,
                                                      P(d_argb), dst_stride, P(stream) if stream else None),
                    "cg_hdr_bloom_pack_device")

    def rt_render_exposed_bloom_device(self, cams, d_argb, d_scales, params, bloom, lights=None,
                                       per_frame_lights=False, d_prev=None, op=TONE_LINEAR, white2=1.0, frame_stride=0,
                                       stream=None):
        """cg_rt_render_exposed_bloom_device: rt_render_exposed_device with bloom between exposure and
        the tone curve (bloom None: that call itself)."""
        larr, n = self._exposed_lights(cams, lights, per_frame_lights)
        arr = (RtCamera * max(len(cams), 1))(*cams)
        self._check(self.lib.cg_rt_render_exposed_bloom_device(
            self.h, larr, n, arr, len(cams), int(bool(per_frame_lights)), C.byref(params),
            P(d_prev) if d_prev else None, op, white2, C.byref(bloom) if bloom is not None else None, P(d_argb),
            frame_stride, P(d_scales), P(stream) if stream else None), "cg_rt_render_exposed_bloom_device")

    def rt_render_exposed_bloom(self, cams, bloom, lights=None, per_frame_lights=False, permille=990, target=1.0,
                                scale_min=2.0 ** -16, scale_max=2.0 ** 16, rate=1.0, prev=None, op=TONE_LINEAR,
                                white2=1.0):
        """cg_rt_render_exposed_bloom: (frames uint32[n, H, W], scales float32[n]) in host memory."""
        n = len(cams)
        if n == 0:
            return np.zeros((0, 0, 0), np.uint32), np.zeros(0, np.float32)
        larr, nl = self._exposed_lights(cams, lights, per_frame_lights)
        arr = (RtCamera * n)(*cams)
        params = hdr_params(permille, target, scale_min, scale_max, rate)
        out = np.zeros((n, cams[0].height, cams[0].width), np.uint32)
        scales = np.zeros(n, np.float32)
        pv = None if prev is None else np.array([prev], np.float32)
        st = Stats()
        self._check(self.lib.cg_rt_render_exposed_bloom(
            self.h, larr, nl, arr, n, int(bool(per_frame_lights)), C.byref(params),
            pv.ctypes.data_as(P) if pv is not None else None, op, white2,
            C.byref(bloom) if bloom is not None else None, out.ctypes.data_as(P), 0, scales.ctypes.data_as(P),
            C.byref(st)), "cg_rt_render_exposed_bloom")
        return out, scales

    def rt_render_frames(self, cams, out=None, chunk=0, lights=None, frame_stride=0):
        """cg_rt_render_frames: len(cams) frames into host memory `out` at f * frame_stride pixels
        (uint32; pageable or pinned, allocated pageable when None; frame_stride 0 = W * H),
        downloads overlapped with later renders."""
        lights = default_lights() if lights is None else lights
        arr = (RtCamera * len(cams))(*cams)
        npx = cams[0].width * cams[0].height
        stride = frame_stride or npx
        if stride < npx:
            raise ValueError(f"frame_stride {stride} < W*H = {npx}")
        if out is None:
            out = np.zeros(len(cams) * stride, np.uint32)
        # the C entry has no capacity argument: the last frame ends at (n - 1) * stride + W * H
        # pixels, and a caller's buffer shorter than that would be written past its end
        need = (len(cams) - 1) * stride + npx
        have = (out.nbytes if isinstance(out, np.ndarray) else out.numel() * out.element_size()) // 4
        if have < need:
            raise ValueError(f"out holds {have} pixels, {len(cams)} frames at stride {stride} need {need}")
        ptr = out.ctypes.data if isinstance(out, np.ndarray) else out.data_ptr()
        st = Stats()
        self._check(self.lib.cg_rt_render_frames(self.h, lights, len(lights), arr, len(cams), P(ptr), stride, chunk,
                                                 C.byref(st)), "cg_rt_render_frames")
        return out, st

    def rt_render_device(self, cam, d_out, shard=None, stream=None, lights=None):
        lights = default_lights() if lights is None else lights
        sh = C.byref(shard) if shard is not None else None
        self._check(self.lib.cg_rt_render_device(self.h, lights, len(lights), C.byref(cam), sh,
                                                 P(d_out), P(stream) if stream else None),
                    "cg_rt_render_device")

    def rt_render_frames_device(self, cams, d_out, shard=None, stream=None, lights=None, frame_stride=0,
                                pix_format=PIX_ARGB8888):
        """cg_rt_render_frames_device: len(cams) frames into d_out + f * frame_stride pixels."""
        lights = default_lights() if lights is None else lights
        arr = (RtCamera * len(cams))(*cams)
        sh = C.byref(shard) if shard is not None else None
        self._check(self.lib.cg_rt_render_frames_device(self.h, lights, len(lights), arr, len(cams), sh, P(d_out),
                                                        frame_stride, pix_format, P(stream) if stream else None),
                    "cg_rt_render_frames_device")

    def rt_render_sequence_device(self, cams, lights, d_out, shard=None, stream=None, frame_stride=0,
                                  pix_format=PIX_ARGB8888):
        """cg_rt_render_sequence_device: frame f with camera cams[f] and lights lights[f] (a list of
        per-frame light lists of equal length) into d_out + f * frame_stride pixels."""
        if len(lights) != len(cams):
            raise ValueError("one light list per frame")
        larr, n = sequence_lights(lights)
        arr = (RtCamera * max(len(cams), 1))(*cams)
        sh = C.byref(shard) if shard is not None else None
        self._check(self.lib.cg_rt_render_sequence_device(self.h, larr, n, arr, len(cams), sh, P(d_out), frame_stride,
                                                          pix_format, P(stream) if stream else None),
                    "cg_rt_render_sequence_device")

    def rt_render_sequence(self, cams, lights, out=None, chunk=0, frame_stride=0):
        """cg_rt_render_sequence: the sequence into host memory `out` (as rt_render_frames)."""
        if len(lights) != len(cams):
            raise ValueError("one light list per frame")
        if not cams:   # the C entry returns CG_OK for n_frames == 0
            return (np.zeros(0, np.uint32) if out is None else out), Stats()
        larr, n = sequence_lights(lights)
        arr = (RtCamera * max(len(cams), 1))(*cams)
        npx = cams[0].width * cams[0].height
        stride = frame_stride or npx
        if stride < npx:
            raise ValueError(f"frame_stride {stride} < W*H = {npx}")
        if out is None:
            out = np.zeros(len(cams) * stride, np.uint32)
        need = (len(cams) - 1) * stride + npx
        have = (out.nbytes if isinstance(out, np.ndarray) else out.numel() * out.element_size()) // 4
        if have < need:
            raise ValueError(f"out holds {have} pixels, {len(cams)} frames at stride {stride} need {need}")
        ptr = out.ctypes.data if isinstance(out, np.ndarray) else out.data_ptr()
        st = Stats()
        self._check(self.lib.cg_rt_render_sequence(self.h, larr, n, arr, len(cams), P(ptr), stride, chunk, C.byref(st)),
                    "cg_rt_render_sequence")
        return out, st

    def _sequence_jpeg(self, call, what, n, width, height, quality, subsampling, out, cap, prm=None):
        """A compressed delivery call: `call(params, out pointer, cap, offsets)` -> its status.  Without
        `out` the buffer starts at n * W * H / 4 bytes and the call is repeated once at the capacity it
        asks for.  -> (rc, out, offsets uint64[n + 1])."""
        prm = JpegParams(quality, subsampling) if prm is None else prm
        offsets = np.zeros(n + 1, np.uint64)
        op = C.cast(offsets.ctypes.data, C.POINTER(C.c_size_t))
        own = out is None
        if own:
            out = np.empty(max(4096, n * width * height // 4) if cap is None else cap, np.uint8)
        size = out.nbytes if isinstance(out, np.ndarray) else out.numel() * out.element_size()
        cap = size if cap is None else cap
        if cap > size:
            raise ValueError(f"cap {cap} > the {size} bytes of out")
        ptr = lambda a: P(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())  # noqa: E731
        rc = call(C.byref(prm), ptr(out), cap, op)
        if rc == CG_E_CAPACITY and own and cap == size:
            out = np.empty(int(offsets[n]), np.uint8)
            rc = call(C.byref(prm), ptr(out), out.size, op)
        if rc != CG_E_CAPACITY:
            self._check(rc, what)
        return rc, out, offsets

    @staticmethod
    def _jpeg_files(rc, out, offsets, cap):
        """The files of a delivery as bytes; after CG_E_CAPACITY those that fit whole before the first that does not."""
        host = out if isinstance(out, np.ndarray) else out.cpu().numpy()
        files = []
        for f in range(len(offsets) - 1):
            if rc == CG_E_CAPACITY and int(offsets[f + 1]) > cap:
                break
            files.append(host[int(offsets[f]):int(offsets[f + 1])].tobytes())
        return files

    def rt_render_sequence_jpeg(self, cams, lights, quality=75, subsampling=JPEG_420, chunk=0, out=None, cap=None,
                                full=False):
        """cg_rt_render_sequence_jpeg: rt_render_sequence's frames as JPEG files -> list[bytes].  out /
        cap supply the destination (a numpy array or a pinned tensor) and its capacity; full=True
        returns (rc, files that fit, offsets, stats) and does not raise on CG_E_CAPACITY."""
        if len(lights) != len(cams):
            raise ValueError("one light list per frame")
        if not cams:
            return ([] if not full else (CG_OK, [], np.zeros(1, np.uint64), Stats()))
        larr, n = sequence_lights(lights)
        arr = (RtCamera * len(cams))(*cams)
        st = Stats()
        call = lambda prm, o, c, offs: self.lib.cg_rt_render_sequence_jpeg(  # noqa: E731
            self.h, larr, n, arr, len(cams), prm, o, c, offs, chunk, C.byref(st))
        rc, buf, offsets = self._sequence_jpeg(call, "cg_rt_render_sequence_jpeg", len(cams), cams[0].width,
                                               cams[0].height, quality, subsampling, out, cap)
        size = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
        files = self._jpeg_files(rc, buf, offsets, size if cap is None else cap)
        if full:
            return rc, files, offsets, st
        self._check(rc, "cg_rt_render_sequence_jpeg")
        return files

    def rast_draw_sequence_jpeg(self, params_list, quality=75, subsampling=JPEG_420, chunk=0, out=None, cap=None,
                                full=False):
        """cg_rast_draw_sequence_jpeg: rast_draw_sequence's frames as JPEG files -> (list[bytes], info);
        full=True returns (rc, files that fit, offsets, info, stats) and does not raise on CG_E_CAPACITY."""
        n = len(params_list)
        arr = (RastParams * max(n, 1))(*params_list)
        info = np.zeros(n + 1, RAST_SEQ_DTYPE)
        st = Stats()
        if not n:
            return ([], info) if not full else (CG_OK, [], np.zeros(1, np.uint64), info, st)
        call = lambda prm, o, c, offs: self.lib.cg_rast_draw_sequence_jpeg(  # noqa: E731
            self.h, arr, n, prm, o, c, offs, chunk, C.cast(info.ctypes.data, C.POINTER(RastSeqFrame)), C.byref(st))
        rc, buf, offsets = self._sequence_jpeg(call, "cg_rast_draw_sequence_jpeg", n, params_list[0].width,
                                               params_list[0].height, quality, subsampling, out, cap)
        size = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
        files = self._jpeg_files(rc, buf, offsets, size if cap is None else cap)
        if full:
            return rc, files, offsets, info, st
        self._check(rc, "cg_rast_draw_sequence_jpeg")
        return files, info

    def rt_render_sequence_png(self, cams, lights, colour=PNG_RGB, filter=PNG_FILTER_ADAPTIVE, chunk=0, out=None, cap=None,
                               full=False):
        """cg_rt_render_sequence_png: rt_render_sequence's frames as PNG files -> list[bytes]; arguments
        and full=True as rt_render_sequence_jpeg."""
        if len(lights) != len(cams):
            raise ValueError("one light list per frame")
        if not cams:
            return ([] if not full else (CG_OK, [], np.zeros(1, np.uint64), Stats()))
        larr, n = sequence_lights(lights)
        arr = (RtCamera * len(cams))(*cams)
        st = Stats()
        call = lambda prm, o, c, offs: self.lib.cg_rt_render_sequence_png(  # noqa: E731
            self.h, larr, n, arr, len(cams), prm, o, c, offs, chunk, C.byref(st))
        rc, buf, offsets = self._sequence_jpeg(call, "cg_rt_render_sequence_png", len(cams), cams[0].width,
                                               cams[0].height, 0, 0, out, cap, PngParams(colour, filter))
        size = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
        files = self._jpeg_files(rc, buf, offsets, size if cap is None else cap)
        if full:
            return rc, files, offsets, st
        self._check(rc, "cg_rt_render_sequence_png")
        return files

    def rt_render_sequence_exr(self, cams, lights, channels=EXR_RGBA, type=EXR_HALF, compression=EXR_ZIP, alpha_scale=1.0,
                               chunk=0, out=None, cap=None, full=False):
        """cg_rt_render_sequence_exr: the CG_PIX_RGBA_F32 pictures of a key script as EXR files -> list[bytes];
        arguments and full=True as rt_render_sequence_jpeg (chunk at most 8)."""
        if len(lights) != len(cams):
            raise ValueError("one light list per frame")
        if not cams:
            return ([] if not full else (CG_OK, [], np.zeros(1, np.uint64), Stats()))
        larr, n = sequence_lights(lights)
        arr = (RtCamera * len(cams))(*cams)
        st = Stats()
        call = lambda prm, o, c, offs: self.lib.cg_rt_render_sequence_exr(  # noqa: E731
            self.h, larr, n, arr, len(cams), prm, o, c, offs, chunk, C.byref(st))
        rc, buf, offsets = self._sequence_jpeg(call, "cg_rt_render_sequence_exr", len(cams), cams[0].width, cams[0].height,
                                               0, 0, out, cap, ExrParams(channels, type, compression, alpha_scale))
        size = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
        files = self._jpeg_files(rc, buf, offsets, size if cap is None else cap)
        if full:
            return rc, files, offsets, st
        self._check(rc, "cg_rt_render_sequence_exr")
        return files

    def rast_draw_sequence_exr(self, params_list, channels=EXR_RGBA, type=EXR_HALF, compression=EXR_ZIP, alpha_scale=1.0,
                               chunk=0, out=None, cap=None, full=False):
        """cg_rast_draw_sequence_exr: the float pictures of a key script as EXR files -> (list[bytes], info);
        arguments and full=True as rast_draw_sequence_jpeg (chunk at most 8)."""
        n = len(params_list)
        arr = (RastParams * max(n, 1))(*params_list)
        info = np.zeros(n + 1, RAST_SEQ_DTYPE)
        st = Stats()
        if not n:
            return ([], info) if not full else (CG_OK, [], np.zeros(1, np.uint64), info, st)
        call = lambda prm, o, c, offs: self.lib.cg_rast_draw_sequence_exr(  # noqa: E731
            self.h, arr, n, prm, o, c, offs, chunk, C.cast(info.ctypes.data, C.POINTER(RastSeqFrame)), C.byref(st))
        rc, buf, offsets = self._sequence_jpeg(call, "cg_rast_draw_sequence_exr", n, params_list[0].width,
                                               params_list[0].height, 0, 0, out, cap,
                                               ExrParams(channels, type, compression, alpha_scale))
        size = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
        files = self._jpeg_files(rc, buf, offsets, size if cap is None else cap)
        if full:
            return rc, files, offsets, info, st
        self._check(rc, "cg_rast_draw_sequence_exr")
        return files, info

    def rast_draw_sequence_png(self, params_list, colour=PNG_RGB, filter=PNG_FILTER_ADAPTIVE, chunk=0, out=None, cap=None,
                               full=False):
        """cg_rast_draw_sequence_png: rast_draw_sequence's frames as PNG files -> (list[bytes], info);
        arguments and full=True as rast_draw_sequence_jpeg."""
        n = len(params_list)
        arr = (RastParams * max(n, 1))(*params_list)
        info = np.zeros(n + 1, RAST_SEQ_DTYPE)
        st = Stats()
        if not n:
            return ([], info) if not full else (CG_OK, [], np.zeros(1, np.uint64), info, st)
        call = lambda prm, o, c, offs: self.lib.cg_rast_draw_sequence_png(  # noqa: E731
            self.h, arr, n, prm, o, c, offs, chunk, C.cast(info.ctypes.data, C.POINTER(RastSeqFrame)), C.byref(st))
        rc, buf, offsets = self._sequence_jpeg(call, "cg_rast_draw_sequence_png", n, params_list[0].width,
                                               params_list[0].height, 0, 0, out, cap, PngParams(colour, filter))
        size = buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()
        files = self._jpeg_files(rc, buf, offsets, size if cap is None else cap)
        if full:
            return rc, files, offsets, info, st
        self._check(rc, "cg_rast_draw_sequence_png")
        return files, info

    def rt_assemble_device(self, d_src, pix_format, row0, rows, width, height, nframes, d_frames, frame_stride=0,
                           stream=None, col0=0, cols=0):
        """cg_rt_assemble_device: row blocks (row0[b], rows[b]) of nframes frames -> frames."""
        n = len(rows)
        r0, rs = (C.c_int * n)(*row0), (C.c_int * n)(*rows)
        self._check(self.lib.cg_rt_assemble_device(self.h, P(d_src), pix_format, r0, rs, n, width, height, nframes,
                                                   P(d_frames), frame_stride, col0, cols,
                                                   P(stream) if stream else None),
                    "cg_rt_assemble_device")

    def rt_unstripe_device(self, d_gathered, width, height, nranks, stripe_h, d_frame, stream=None):
        self._check(self.lib.cg_rt_unstripe_device(self.h, P(d_gathered), width, height, nranks,
                                                   stripe_h, P(d_frame), P(stream) if stream else None),
                    "cg_rt_unstripe_device")

    def rt_unstripe_batch_device(self, d_gathered, width, height, nranks, stripe_h, nframes, d_frames,
                                 stream=None):
        self._check(self.lib.cg_rt_unstripe_batch_device(self.h, P(d_gathered), width, height, nranks, stripe_h,
                                                         nframes, P(d_frames), P(stream) if stream else None),
                    "cg_rt_unstripe_batch_device")

    def rt_hits_device(self, cam, sub_ray=4, shard=None, d_isect=None, d_index=None, d_distance=None, stream=None):
        """cg_rt_hits_device: the shard's hit planes into device memory (addresses; any may be None,
        not all three): cg_rt_shard_rows() rows of W records / int32 / float32."""
        sh = C.cast(C.byref(shard), C.c_void_p) if shard is not None else None
        self._check(self.lib.cg_rt_hits_device(self.h, C.byref(cam), sub_ray, sh, P(d_isect) if d_isect else None,
                                               P(d_index) if d_index else None,
                                               P(d_distance) if d_distance else None,
                                               P(stream) if stream else None), "cg_rt_hits_device")

    def rt_hits(self, cam, sub_ray=4, isect=True, index=True, distance=True):
        """cg_rt_hits: the whole frame's hit planes in host memory as (isect ISECT_DTYPE[H * W], index
        int32[H * W], distance float32[H * W]); a plane that was not asked for is None."""
        n = cam.width * cam.height
        a = np.zeros(n, ISECT_DTYPE) if isect else None
        b = np.zeros(n, np.int32) if index else None
        d = np.zeros(n, np.float32) if distance else None
        self._check(self.lib.cg_rt_hits(self.h, C.byref(cam), sub_ray, a.ctypes.data_as(P) if isect else None,
                                        b.ctypes.data_as(P) if index else None,
                                        d.ctypes.data_as(P) if distance else None), "cg_rt_hits")
        return a, b, d

    def rt_pick(self, cam, x, y, sub_ray=4):
        """cg_rt_pick: (record as a 1-element ISECT_DTYPE array, hit) of one pixel's sub-ray."""
        out, hit = np.zeros(1, ISECT_DTYPE), C.c_int()
        self._check(self.lib.cg_rt_pick(self.h, C.byref(cam), x, y, sub_ray,
                                        C.cast(out.ctypes.data, C.POINTER(Isect)), C.byref(hit)), "cg_rt_pick")
        return out, bool(hit.value)

    def rt_probe_closest_np(self, starts, dirs):
        """cg_rt_probe_closest on float32[n, 4] arrays: (records ISECT_DTYPE[n], hit int32[n])."""
        S, D = np.ascontiguousarray(starts, np.float32), np.ascontiguousarray(dirs, np.float32)
        n = len(S)
        out, hit = np.zeros(n, ISECT_DTYPE), np.zeros(n, np.int32)
        self._check(self.lib.cg_rt_probe_closest(self.h, C.cast(S.ctypes.data, C.POINTER(Vec4)),
                                                 C.cast(D.ctypes.data, C.POINTER(Vec4)), n,
                                                 C.cast(out.ctypes.data, C.POINTER(Isect)),
                                                 C.cast(hit.ctypes.data, C.POINTER(C.c_int))), "cg_rt_probe_closest")
        return out, hit

    def rt_probe_closest(self, starts, dirs):
        n = len(starts)
        S, D = (Vec4 * n)(*[Vec4(*s) for s in starts]), (Vec4 * n)(*[Vec4(*d) for d in dirs])
        out, hit = (Isect * n)(), (C.c_int * n)()
        self._check(self.lib.cg_rt_probe_closest(self.h, S, D, n, out, hit), "cg_rt_probe_closest")
        return out, list(hit)

    def rt_probe_direct_light(self, isects, light):
        n = len(isects)
        arr = (Isect * n)(*isects)
        out = (Vec3 * n)()
        self._check(self.lib.cg_rt_probe_direct_light(self.h, arr, C.byref(light), n, out),
                    "cg_rt_probe_direct_light")
        return out

    # -- RAST --
    def starfield_draw(self, stars, width=320, height=256):
        out = np.zeros(width * height, np.uint32)
        self._check(self.lib.cg_starfield_draw(self.h, stars.ctypes.data_as(P), len(stars), width, height,
                                               out.ctypes.data_as(P)), "cg_starfield_draw")
        return out

    def starfield_set(self, stars):
        """cg_starfield_set: (n, 3) float32 stars become the context's resident stars."""
        st = np.ascontiguousarray(stars, np.float32).reshape(-1, 3)
        self._check(self.lib.cg_starfield_set(self.h, st.ctypes.data_as(P), len(st)), "cg_starfield_set")
        self._star_n = len(st)

    def starfield_get(self, cap=None):
        """cg_starfield_get: the resident stars as (n, 3) float32, after the context's starfield
        work (cap: capacity offered in stars; None = the count of the latest starfield_set)."""
        cap = getattr(self, "_star_n", 0) if cap is None else cap
        out = np.zeros((max(cap, 1), 3), np.float32)
        n = self.lib.cg_starfield_get(self.h, out.ctypes.data_as(P), cap)
        if n < 0:
            self._check(n, "cg_starfield_get")
        return out[:n].copy()

    def starfield_run_device(self, dts, n_frames, width, height, d_argb, n_updates=None, frame_stride=0,
                             stream=None):
        """cg_starfield_run_device: n_frames frames into d_argb + f * frame_stride pixels, frame f
        after f updates, update f with frame time dts[f] (n_updates: n_frames, the default, or
        n_frames - 1).  Enqueues only."""
        n_updates = n_frames if n_updates is None else n_updates
        d = _dts(dts)
        if len(d) < n_updates:
            raise ValueError(f"{n_updates} updates need {n_updates} frame times, got {len(d)}")
        self._check(self.lib.cg_starfield_run_device(self.h, d.ctypes.data_as(P) if len(d) else None, n_updates,
                                                     n_frames, width, height, P(d_argb), frame_stride,
                                                     P(stream) if stream else None), "cg_starfield_run_device")

    def starfield_advance_device(self, dts, stream=None):
        """cg_starfield_advance_device: one Update per entry of dts, no drawing.  Enqueues only."""
        d = _dts(dts)
        self._check(self.lib.cg_starfield_advance_device(self.h, d.ctypes.data_as(P) if len(d) else None, len(d),
                                                         P(stream) if stream else None),
                    "cg_starfield_advance_device")

    def starfield_run(self, dts, n_frames, width=320, height=256, n_updates=None, out=None, chunk=0,
                      frame_stride=0):
        """cg_starfield_run: the frames of starfield_run_device into host memory `out` (as
        rt_render_frames: uint32, pageable or pinned, allocated pageable when None)."""
        n_updates = n_frames if n_updates is None else n_updates
        d = _dts(dts)
        if len(d) < n_updates:
            raise ValueError(f"{n_updates} updates need {n_updates} frame times, got {len(d)}")
        npx = width * height
        stride = frame_stride or npx
        if stride < npx:
            raise ValueError(f"frame_stride {stride} < W*H = {npx}")
        if out is None:
            out = np.zeros(n_frames * stride, np.uint32)
        need = (n_frames - 1) * stride + npx if n_frames else 0
        have = (out.nbytes if isinstance(out, np.ndarray) else out.numel() * out.element_size()) // 4
        if have < need:
            raise ValueError(f"out holds {have} pixels, {n_frames} frames at stride {stride} need {need}")
        ptr = out.ctypes.data if isinstance(out, np.ndarray) else out.data_ptr()
        st = Stats()
        self._check(self.lib.cg_starfield_run(self.h, d.ctypes.data_as(P) if len(d) else None, n_updates, n_frames,
                                              width, height, P(ptr), stride, chunk, C.byref(st)), "cg_starfield_run")
        return out, st

    def rast_render(self, tris, n, params, light, want_depth=True, want_shadow=True):
        npx = params.width * params.height
        argb = np.zeros(npx, np.uint32)
        depth = np.zeros(npx, np.float32) if want_depth else None
        shadow = np.zeros(npx, np.int32) if want_shadow else None
        st = Stats()
        self._check(self.lib.cg_rast_render(
            self.h, tris, n, C.byref(params), light, argb.ctypes.data_as(P),
            depth.ctypes.data_as(P) if depth is not None else None,
            shadow.ctypes.data_as(P) if shadow is not None else None, C.byref(st)), "cg_rast_render")
        return argb, depth, shadow, st

    def rast_set_scene(self, room=None, nr=None, boxes=None, nb=None):
        if room is None:
            room, nr, boxes, nb = rast_scene()
        self._check(self.lib.cg_rast_set_scene(self.h, room, nr, boxes, nb), "cg_rast_set_scene")

    def rast_set_textures(self, maps):
        """maps: {name: uint8 (H, W, 3) BGR array} over TEXTURE_MAPS (absent = not
        loaded), as cv::imread returns them; None unloads."""
        if maps is None:
            self._check(self.lib.cg_rast_set_textures(self.h, None), "cg_rast_set_textures")
            return
        arrs = {}
        for k, v in maps.items():
            a = np.ascontiguousarray(v, dtype=np.uint8)
            if a.shape != TEXTURE_SHAPES.get(k, (1024, 1024, 3)):
                raise ValueError(f"texture {k}: shape {a.shape}")
            arrs[k] = a
        t = RastTextures(**{k: a.ctypes.data for k, a in arrs.items()})
        self._check(self.lib.cg_rast_set_textures(self.h, C.byref(t)), "cg_rast_set_textures")

    def decode_jpeg(self, data: bytes) -> np.ndarray:
        """cv::imread(..., CV_LOAD_IMAGE_UNCHANGED) of JPEG bytes (skeleton.cpp:135-146) on
        this context's GPU: uint8 (H, W, 3) BGR or (H, W) gray."""
        w, h, ch = jpeg_info(data)
        buf = np.frombuffer(data, np.uint8)
        out = np.zeros((h, w, ch), np.uint8)
        self._check(self.lib.cg_image_decode_jpeg(self.h, buf.ctypes.data_as(P), buf.size, out.ctypes.data_as(P),
                                                  out.size), "cg_image_decode_jpeg")
        return out if ch == 3 else out[:, :, 0]

    def decode_jpeg_device(self, data: bytes, d_out, cap, stream=None):
        """cg_image_decode_jpeg_device: the same bytes as decode_jpeg, written to the device
        address d_out (room for `cap` bytes), asynchronously on `stream` (a HIP stream handle;
        None: the context's).  Returns the status (CG_OK, or CG_E_CAPACITY when cap is less
        than width * height * channels, in which case nothing is written); raises on any
        other failure."""
        buf = np.frombuffer(data, np.uint8)
        rc = self.lib.cg_image_decode_jpeg_device(self.h, buf.ctypes.data_as(P), buf.size, P(d_out), cap,
                                                  P(stream) if stream else None)
        if rc != CG_E_CAPACITY:
            self._check(rc, "cg_image_decode_jpeg_device")
        return rc

    def image_encode_jpeg(self, argb, quality=75, subsampling=JPEG_420) -> bytes:
        """cg_image_encode_jpeg: image_encode_jpeg_host's file, encoded on this context's GPU."""
        fn = lambda *a: self.lib.cg_image_encode_jpeg(self.h, *a)   # noqa: E731
        return _jpeg_encode(fn, "cg_image_encode_jpeg", argb, quality, subsampling)

    def image_encode_jpeg_device(self, d_argb, width, height, n_frames, d_out, slot_bytes, d_bytes, quality=75,
                                 subsampling=JPEG_420, frame_stride=0, stream=None):
        """cg_image_encode_jpeg_device: n_frames ARGB8888 frames at the device address d_argb (frame_stride
        pixels apart; 0: width * height) to files at d_out + f * slot_bytes, their lengths (or
        CG_E_CAPACITY) to the int64 array d_bytes; enqueued on `stream` (None: the context's)."""
        prm = JpegParams(quality, subsampling)
        self._check(self.lib.cg_image_encode_jpeg_device(self.h, P(d_argb), width, height, n_frames, frame_stride,
                                                         C.byref(prm), P(d_out), slot_bytes, P(d_bytes),
                                                         P(stream) if stream else None),
                    "cg_image_encode_jpeg_device")

    def image_encode_png(self, argb, colour=PNG_RGB, filter=PNG_FILTER_ADAPTIVE) -> bytes:
        """cg_image_encode_png: image_encode_png_host's file, encoded on this context's GPU."""
        fn = lambda *a: self.lib.cg_image_encode_png(self.h, *a)   # noqa: E731
        return _png_encode(fn, "cg_image_encode_png", argb, colour, filter)

    def image_encode_png_device(self, d_argb, width, height, n_frames, d_out, slot_bytes, d_bytes, colour=PNG_RGB,
                                filter=PNG_FILTER_ADAPTIVE, frame_stride=0, stream=None):
        """cg_image_encode_png_device: n_frames ARGB8888 frames at the device address d_argb (frame_stride
        pixels apart; 0: width * height) to PNG files at d_out + f * slot_bytes, their lengths (or
        CG_E_CAPACITY) to the int64 array d_bytes; enqueued on `stream` (None: the context's)."""
        prm = PngParams(colour, filter)
        self._check(self.lib.cg_image_encode_png_device(self.h, P(d_argb), width, height, n_frames, frame_stride,
                                                        C.byref(prm), P(d_out), slot_bytes, P(d_bytes),
                                                        P(stream) if stream else None),
                    "cg_image_encode_png_device")

    def image_encode_exr(self, rgba, channels=EXR_RGBA, type=EXR_HALF, compression=EXR_ZIP, alpha_scale=1.0) -> bytes:
        """cg_image_encode_exr: image_encode_exr_host's file, encoded on this context's GPU."""
        fn = lambda *a: self.lib.cg_image_encode_exr(self.h, *a)   # noqa: E731
        return _exr_encode(fn, "cg_image_encode_exr", rgba, channels, type, compression, alpha_scale)

    def image_encode_exr_device(self, d_rgba, width, height, n_frames, d_out, slot_bytes, d_bytes, channels=EXR_RGBA,
                                type=EXR_HALF, compression=EXR_ZIP, alpha_scale=1.0, frame_stride=0, stream=None):
        """cg_image_encode_exr_device: n_frames CG_PIX_RGBA_F32 pictures at the device address d_rgba
        (frame_stride pixels apart; 0: width * height) to EXR files at d_out + f * slot_bytes, their
        lengths (or CG_E_CAPACITY) to the int64 array d_bytes; enqueued on `stream` (None: the context's)."""
        prm = ExrParams(channels, type, compression, alpha_scale)
        self._check(self.lib.cg_image_encode_exr_device(self.h, P(d_rgba), width, height, n_frames, frame_stride,
                                                        C.byref(prm), P(d_out), slot_bytes, P(d_bytes),
                                                        P(stream) if stream else None),
                    "cg_image_encode_exr_device")

    def load_textures_jpeg(self, directory: str) -> dict:
        """Decode the reference's texture files found in `directory` (names as
        skeleton.cpp:135-146) -> {map name: BGR array}, ready for rast_set_textures."""
        maps = {}
        for name, fn in TEXTURE_FILES.items():
            path = os.path.join(directory, fn)
            if os.path.exists(path):
                with open(path, "rb") as f:
                    maps[name] = self.decode_jpeg(f.read())
        return maps

    def rast_draw(self, params, want_depth=True, want_shadow=True):
        """Whole Draw on the device (geometry + fill + post)."""
        npx = params.width * params.height
        argb = np.zeros(npx, np.uint32)
        depth = np.zeros(npx, np.float32) if want_depth else None
        shadow = np.zeros(npx, np.int32) if want_shadow else None
        st = Stats()
        self._check(self.lib.cg_rast_draw(
            self.h, C.byref(params), argb.ctypes.data_as(P),
            depth.ctypes.data_as(P) if depth is not None else None,
            shadow.ctypes.data_as(P) if shadow is not None else None, C.byref(st)), "cg_rast_draw")
        return argb, depth, shadow, st

    ALL_RAST_PLANES = tuple(n for n, _, _ in RAST_PLANES)

    def rast_draw_buffers(self, params, want=ALL_RAST_PLANES, stats=None):
        """cg_rast_draw_buffers: the Draw of rast_draw with the planes named in `want` (RAST_PLANES:
        argb, depth, shadow, the HDR triple screen / low / high, the owner's clip / tri / pos) as a
        dict of numpy arrays."""
        b, out = rast_buffers_planes(params, want)
        self._check(self.lib.cg_rast_draw_buffers(self.h, C.byref(params), C.byref(b),
                                                  C.byref(stats) if stats is not None else None),
                    "cg_rast_draw_buffers")
        return out

    def rast_render_buffers(self, tris, n, params, light, want=ALL_RAST_PLANES, stats=None):
        """cg_rast_render_buffers: rast_render's frame of a clipped list with the planes in `want`
        (tri = clip: the caller's list is the clipped list)."""
        b, out = rast_buffers_planes(params, want)
        self._check(self.lib.cg_rast_render_buffers(self.h, tris, n, C.byref(params), light, C.byref(b),
                                                    C.byref(stats) if stats is not None else None),
                    "cg_rast_render_buffers")
        return out

    @staticmethod
    def _rast_buffers_device(planes):
        b = RastBuffers()
        for name, ptr in planes.items():
            if name not in Context.ALL_RAST_PLANES:
                raise ValueError(f"no such rasteriser plane: {name}")
            setattr(b, name, ptr if ptr else None)
        return b

    def rast_draw_buffers_device(self, params, stream=None, **planes):
        """cg_rast_draw_buffers_device: planes by name (argb=, depth=, ..., pos=) as device addresses."""
        b = self._rast_buffers_device(planes)
        self._check(self.lib.cg_rast_draw_buffers_device(self.h, C.byref(params), C.byref(b),
                                                         P(stream) if stream else None),
                    "cg_rast_draw_buffers_device")

    def rast_render_buffers_device(self, d_tris, n, params, light, stream=None, **planes):
        """cg_rast_render_buffers_device: as rast_draw_buffers_device over a device list."""
        b = self._rast_buffers_device(planes)
        self._check(self.lib.cg_rast_render_buffers_device(self.h, P(d_tris), n, C.byref(params), light, C.byref(b),
                                                           P(stream) if stream else None),
                    "cg_rast_render_buffers_device")

    def rast_pick(self, params, x, y):
        """cg_rast_pick: (tri, clip, pos float32[4], hit) of the fragment that owns pixel (x, y)."""
        tri, clip, pos, hit = C.c_int32(), C.c_int32(), Vec4(), C.c_int()
        self._check(self.lib.cg_rast_pick(self.h, C.byref(params), x, y, C.byref(tri), C.byref(clip), C.byref(pos),
                                          C.byref(hit)), "cg_rast_pick")
        return tri.value, clip.value, np.array([pos.x, pos.y, pos.z, pos.w], np.float32), bool(hit.value)

    def rast_state_bytes(self):
        """cg_rast_state_bytes: 2 or 4, the state word the latest frame's fill left per pixel (0: no frame)."""
        return self.lib.cg_rast_state_bytes(self.h)

    def rast_draw_device(self, params, d_argb, d_depth=None, d_shadow=None, stream=None):
        self._check(self.lib.cg_rast_draw_device(self.h, C.byref(params), P(d_argb), P(d_depth) if d_depth else None,
                                                 P(d_shadow) if d_shadow else None, P(stream) if stream else None),
                    "cg_rast_draw_device")

    def rast_draw_frames_device(self, params_list, d_argb, d_depth=None, d_shadow=None, frame_stride=0,
                                stream=None):
        """len(params_list) colour-mode-0 Draws, frame f at d_argb + f * stride pixels,
        overlapped on the context's internal streams; `stream` waits for them."""
        arr = (RastParams * len(params_list))(*params_list)
        self._check(self.lib.cg_rast_draw_frames_device(
            self.h, arr, len(params_list), P(d_argb), P(d_depth) if d_depth else None,
            P(d_shadow) if d_shadow else None, frame_stride, P(stream) if stream else None),
            "cg_rast_draw_frames_device")

    def rast_draw_sequence_device(self, params_list, d_argb, d_depth=None, d_shadow=None, frame_stride=0,
                                  d_info=None, stream=None):
        """len(params_list) successive Draws in any mix of colour modes 0-2, enqueued on `stream`
        in order; the rand() call index starts at params_list[0].rand_offset and is chained on the
        device.  d_info: device memory for len(params_list) + 1 RastSeqFrame records (24 B each)."""
        arr = (RastParams * max(len(params_list), 1))(*params_list)
        self._check(self.lib.cg_rast_draw_sequence_device(
            self.h, arr, len(params_list), P(d_argb), P(d_depth) if d_depth else None,
            P(d_shadow) if d_shadow else None, frame_stride, P(d_info) if d_info else None,
            P(stream) if stream else None), "cg_rast_draw_sequence_device")

    def rast_draw_sequence(self, params_list, out=None, want_depth=False, want_shadow=False, chunk=0,
                           frame_stride=0):
        """cg_rast_draw_sequence: the frames of rast_draw_sequence_device into host memory, frame f
        at f * frame_stride pixels (0 = W * H), chunks downloading while the next renders.
        -> (argb, depth, shadow, info, stats): info the len(params_list) + 1 records
        (RAST_SEQ_DTYPE), planes not asked for None.  out (and want_depth / want_shadow in place
        of True) may supply a destination, e.g. a pinned tensor (rast_sequence_planes)."""
        n = len(params_list)
        stride, argb, depth, shadow = rast_sequence_planes(params_list, out, want_depth, want_shadow, chunk,
                                                           frame_stride)
        ptr = lambda a: None if a is None else P(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())  # noqa: E731
        arr = (RastParams * max(n, 1))(*params_list)
        info = np.zeros(n + 1, RAST_SEQ_DTYPE)
        st = Stats()
        self._check(self.lib.cg_rast_draw_sequence(
            self.h, arr, n, ptr(argb), ptr(depth), ptr(shadow), stride, chunk,
            C.cast(info.ctypes.data, C.POINTER(RastSeqFrame)), C.byref(st)), "cg_rast_draw_sequence")
        return argb, depth, shadow, info, st

    def rast_draw_picture(self, params):
        """cg_rast_draw_picture: rast_draw's frame before PutPixelSDL clamps it, float32[H, W, 4]
        (PIX_RGBA_F32) -- x, y, z what antiAliasing returns and w = 1 inside, zeros on the border."""
        out = np.zeros((params.height, params.width, 4), np.float32)
        st = Stats()
        self._check(self.lib.cg_rast_draw_picture(self.h, C.byref(params), out.ctypes.data_as(P), C.byref(st)),
                    "cg_rast_draw_picture")
        return out, st

    def rast_draw_picture_device(self, params, d_rgba, d_depth=None, d_shadow=None, stream=None):
        """cg_rast_draw_picture_device: rast_draw_device with W * H float4 pixels at d_rgba."""
        self._check(self.lib.cg_rast_draw_picture_device(self.h, C.byref(params), P(d_rgba),
                                                         P(d_depth) if d_depth else None,
                                                         P(d_shadow) if d_shadow else None,
                                                         P(stream) if stream else None),
                    "cg_rast_draw_picture_device")

    def rast_draw_sequence_picture_device(self, params_list, d_rgba, d_depth=None, d_shadow=None, frame_stride=0,
                                          d_info=None, stream=None):
        """cg_rast_draw_sequence_picture_device: rast_draw_sequence_device with float frames, frame f
        at d_rgba + f * frame_stride pixels of 16 bytes."""
        arr = (RastParams * max(len(params_list), 1))(*params_list)
        self._check(self.lib.cg_rast_draw_sequence_picture_device(
            self.h, arr, len(params_list), P(d_rgba), P(d_depth) if d_depth else None,
            P(d_shadow) if d_shadow else None, frame_stride, P(d_info) if d_info else None,
            P(stream) if stream else None), "cg_rast_draw_sequence_picture_device")

    def rast_tonemap_pack_device(self, d_rgba, n_pixels, n_frames, d_scales, d_argb, op=TONE_LINEAR, white2=1.0,
                                 src_stride=0, dst_stride=0, stream=None):
        """cg_rast_tonemap_pack_device: rt_tonemap_pack_device with the rasteriser's border and clamp rules."""
        self._check(self.lib.cg_rast_tonemap_pack_device(self.h, P(d_rgba), n_pixels, n_frames, src_stride,
                                                         P(d_scales), op, white2, P(d_argb), dst_stride,
                                                         P(stream) if stream else None),
                    "cg_rast_tonemap_pack_device")

    def rast_draw_exposed_device(self, params_list, d_argb, d_scales, params, d_info, d_prev=None, op=TONE_LINEAR,
                                 white2=1.0, frame_stride=0, stream=None):
        """cg_rast_draw_exposed_device: the key script's frames drawn, exposed and packed into d_argb +
        f * frame_stride pixels, their scales into d_scales, their records into d_info (device
        memory, len(params_list) + 1 RastSeqFrame records)."""
        arr = (RastParams * max(len(params_list), 1))(*params_list)
        self._check(self.lib.cg_rast_draw_exposed_device(self.h, arr, len(params_list), C.byref(params),
                                                         P(d_prev) if d_prev else None, op, white2, P(d_argb),
                                                         frame_stride, P(d_scales), P(d_info) if d_info else None,
                                                         P(stream) if stream else None),
                    "cg_rast_draw_exposed_device")

    def rast_draw_exposed(self, params_list, permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16,
                          rate=1.0, prev=None, op=TONE_LINEAR, white2=1.0):
        """cg_rast_draw_exposed: (frames uint32[n, H, W], scales float32[n], info, rc) in host memory;
        rc is CG_OK, or CG_E_CAPACITY when a frame was flagged (everything is delivered all the same)."""
        n = len(params_list)
        if n == 0:
            return np.zeros((0, 0, 0), np.uint32), np.zeros(0, np.float32), np.zeros(1, RAST_SEQ_DTYPE), CG_OK
        arr = (RastParams * n)(*params_list)
        params = hdr_params(permille, target, scale_min, scale_max, rate)
        out = np.zeros((n, params_list[0].height, params_list[0].width), np.uint32)
        scales = np.zeros(n, np.float32)
        info = np.zeros(n + 1, RAST_SEQ_DTYPE)
        pv = None if prev is None else np.array([prev], np.float32)
        st = Stats()
        rc = self.lib.cg_rast_draw_exposed(self.h, arr, n, C.byref(params),
                                           pv.ctypes.data_as(P) if pv is not None else None, op, white2,
                                           out.ctypes.data_as(P), 0, scales.ctypes.data_as(P),
                                           C.cast(info.ctypes.data, C.POINTER(RastSeqFrame)), C.byref(st))
        if rc != CG_E_CAPACITY:
            self._check(rc, "cg_rast_draw_exposed")
        return out, scales, info, rc

    def rast_draw_exposed_bloom_device(self, params_list, d_argb, d_scales, params, bloom, d_info, d_prev=None,
                                       op=TONE_LINEAR, white2=1.0, frame_stride=0, stream=None):
        """cg_rast_draw_exposed_bloom_device: rast_draw_exposed_device with bloom (rule RAST) between
        exposure and the tone curve (bloom None: that call itself)."""
        arr = (RastParams * max(len(params_list), 1))(*params_list)
        self._check(self.lib.cg_rast_draw_exposed_bloom_device(
            self.h, arr, len(params_list), C.byref(params), P(d_prev) if d_prev else None, op, white2,
            C.byref(bloom) if bloom is not None else None, P(d_argb), frame_stride, P(d_scales),
            P(d_info) if d_info else None, P(stream) if stream else None), "cg_rast_draw_exposed_bloom_device")

    def rast_draw_exposed_bloom(self, params_list, bloom, permille=990, target=1.0, scale_min=2.0 ** -16,
                                scale_max=2.0 ** 16, rate=1.0, prev=None, op=TONE_LINEAR, white2=1.0):
        """cg_rast_draw_exposed_bloom: (frames uint32[n, H, W], scales float32[n], info, rc) in host memory,
        as rast_draw_exposed."""
        n = len(params_list)
        if n == 0:
            return np.zeros((0, 0, 0), np.uint32), np.zeros(0, np.float32), np.zeros(1, RAST_SEQ_DTYPE), CG_OK
        arr = (RastParams * n)(*params_list)
        params = hdr_params(permille, target, scale_min, scale_max, rate)
        out = np.zeros((n, params_list[0].height, params_list[0].width), np.uint32)
        scales = np.zeros(n, np.float32)
        info = np.zeros(n + 1, RAST_SEQ_DTYPE)
        pv = None if prev is None else np.array([prev], np.float32)
        st = Stats()
        rc = self.lib.cg_rast_draw_exposed_bloom(self.h, arr, n, C.byref(params),
                                                 pv.ctypes.data_as(P) if pv is not None else None, op, white2,
                                                 C.byref(bloom) if bloom is not None else None,
                                                 out.ctypes.data_as(P), 0, scales.ctypes.data_as(P),
                                                 C.cast(info.ctypes.data, C.POINTER(RastSeqFrame)), C.byref(st))
        if rc != CG_E_CAPACITY:
            self._check(rc, "cg_rast_draw_exposed_bloom")
        return out, scales, info, rc

    def rast_set_route(self, route):
        """Test and A/B hook: -1 automatic, RAST_ROUTE_DENSE / RAST_ROUTE_COMPACT forced."""
        self._check(self.lib.cg_rast_set_route(self.h, route), "cg_rast_set_route")

    def rast_set_route_limit(self, list_capacity):
        """Test and A/B hook: the list capacity above which frames take the compact route automatically (0: 131072)."""
        self._check(self.lib.cg_rast_set_route_limit(self.h, list_capacity), "cg_rast_set_route_limit")

    def rast_scratch_info(self):
        """Rasteriser scratch after the latest frame (waits for it): dict(bytes, route, tris, spans, recs)."""
        out = (C.c_uint64 * 5)()
        self._check(self.lib.cg_rast_scratch_info(self.h, out), "cg_rast_scratch_info")
        return dict(bytes=out[0], route=out[1], tris=out[2], spans=out[3], recs=out[4])

    def rast_set_rand_capacity(self, n):
        """Test hook: fragments the sequence's materialised rand() stream holds (0 = 4 * W * H)."""
        self._check(self.lib.cg_rast_set_rand_capacity(self.h, n), "cg_rast_set_rand_capacity")

    def glibc_rand_device(self, d_offset, n, d_out, stream=None):
        """cg_glibc_rand_device: n values of rand() into d_out (int32, device), from the uint64
        call index at d_offset (device), by the sequence's device seek and generator."""
        self._check(self.lib.cg_glibc_rand_device(self.h, P(d_offset), n, P(d_out), P(stream) if stream else None),
                    "cg_glibc_rand_device")

    def rast_render_device(self, d_tris, n, params, light, d_argb, d_depth=None, d_shadow=None,
                           stream=None):
        self._check(self.lib.cg_rast_render_device(
            self.h, P(d_tris), n, C.byref(params), light, P(d_argb),
            P(d_depth) if d_depth else None, P(d_shadow) if d_shadow else None,
            P(stream) if stream else None), "cg_rast_render_device")
