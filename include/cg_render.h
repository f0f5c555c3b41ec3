/*
 * cg_render.h -- C-ABI of the MI355X-native renderer (gfx950 HIP kernels).
 *
 * This is the drop-in boundary for the two pixel-loop hot paths of
 * fznsakib/Computer-Graphics.  The reference has no plugin/FFI API: its hot
 * paths sit behind `void Draw(screen*)`, which reads mutable globals and
 * writes ARGB pixels into the caller-owned `screen->buffer`.
 * The host surface in computer-graphics_amd/host/ keeps that exact shape
 * (same Draw(screen*), same globals, same Triangle/Sphere/Intersection/Light
 * structs, same PutPixelSDL pixel layout) and calls the entry points below.
 *
 * Conventions: plain pointers and sizes only; POD structs with the
 * reference's field order; every call returns 0 (CG_OK) or a negative
 * CG_E* code and never throws across the ABI.  A context is bound to one
 * GPU and is not thread-safe (one host thread per context, like the
 * reference's single main thread).  Host buffers are caller-owned; device
 * buffers are context-owned unless a *_device entry point is given a
 * caller-owned device pointer.  `stream` arguments are hipStream_t values
 * (NULL = the context's own stream).
 */
#ifndef CG_RENDER_H
#define CG_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CG_OK 0
#define CG_E_INVALID (-1)     /* bad argument / shape */
#define CG_E_NODEVICE (-2)    /* no HIP device / HIP init failed */
#define CG_E_HIP (-3)         /* HIP runtime error (see cg_last_error) */
#define CG_E_NOSCENE (-4)     /* render before cg_rt_set_scene */
#define CG_E_CAPACITY (-5)    /* output capacity too small */
#define CG_E_TIMEOUT (-6)     /* multi-GPU: a peer did not answer within the deadline (communicator aborted) */

typedef struct cg_ctx cg_ctx;

typedef struct { float x, y, z; } cg_vec3;
typedef struct { float x, y, z, w; } cg_vec4;

/* raytracer/Source/TestModelH.h:80-115 `Triangle` (76 B: v0@0 v1@16 v2@32 normal@48 color@64). */
typedef struct { cg_vec4 v0, v1, v2, normal; cg_vec3 color; } cg_tri;
/* raytracer/Source/TestModelH.h:14-22 `Sphere` (44 B). */
typedef struct { float radius, radiusSquared; cg_vec3 centre, color, normal; } cg_sphere;
/* raytracer/Source/skeleton.cpp:47-50 `Light` (28 B). */
typedef struct { cg_vec4 position; cg_vec3 colour; } cg_light;
/* raytracer/Source/skeleton.cpp:40-45 `Intersection` (28 B). */
typedef struct { cg_vec4 position; float distance; int triangleIndex; int sphereIndex; } cg_isect;

/* The RT globals Draw reads (raytracer/Source/skeleton.cpp:56-60, :110). */
typedef struct {
    int width, height;     /* SCREEN_WIDTH / SCREEN_HEIGHT (:19-20) */
    float focal;           /* focalLength (:56) */
    cg_vec4 camera;        /* cameraPos (:57) */
    float R[16];           /* R (:60), glm::mat4 column-major: R[c*4+r] */
    float indirect;        /* indirectLight scale (:110), 0.5 */
} cg_rt_camera;

/* Row sharding for the multi-GPU path.  Stripes (rows == 0): stripes of
 * `stripe_h` rows are dealt round-robin over `nranks`; this rank renders
 * stripes k with k % nranks == rank, packed in order into its output.  Any
 * stripe_h >= 1 is exact; for speed use a multiple of 15 for a one-light
 * camera that is unrotated or only yawed, or an unrotated light set (the
 * lattice kernels' tile height), and of 8 otherwise.
 * Band (rows > 0): this shard renders frame rows row0 .. row0 + rows - 1
 * (rows past the frame are padding); rank / nranks / stripe_h are ignored.
 * Window (cols > 0, CG_PIX_RGB24 output only): only columns col0 .. col0 +
 * cols - 1 are stored, rows `cols` pixels apart -- the caller asserts the other
 * columns are black (cg_rt_frame_columns); col0 and cols are multiples of 16
 * (cols may end at the frame's right edge). */
typedef struct { int rank, nranks, stripe_h; int row0, rows; int col0, cols; } cg_rt_shard;

/* Pixel formats of device outputs.  ARGB8888 is PutPixelSDL's uint32
 * (SDLauxiliary.h:149-161).  RGB24 is its wire form for transfers between
 * GPUs: the low three bytes (B, G, R) of each pixel, 3 bytes per pixel --
 * PutPixelSDL's alpha is always 128, so cg_rt_assemble_device restores the
 * exact uint32.  RGBA_F32 is what Draw holds before PutPixelSDL clamps it
 * (raytracer/Source/skeleton.cpp:160-165): four floats per pixel, 16 bytes,
 * 16-byte aligned -- x, y, z = pixelColour / 9.0f, the vec3 PutPixelSDL is
 * given (+0 in all three for a pixel none of whose sub-rays hit), and w = the
 * number of the pixel's nine sub-rays for which ClosestIntersection returned
 * true (0 .. 9; the reference keeps only validRay = w > 0).  Raytracer frame
 * calls only (cg_rt_render_frames_device, cg_rt_render_sequence_device). */
#define CG_PIX_ARGB8888 0
#define CG_PIX_RGB24 1
#define CG_PIX_RGBA_F32 2
/* Host-only: bytes per pixel of a format (4, 3, 16), or CG_E_INVALID. */
int cg_pix_bytes(int pix_format);

/* rasteriser/Source/TestModelH.h:13-42 `Triangle` (84 B). */
typedef struct { cg_vec4 v0, v1, v2, normal; cg_vec3 color; int texture; int index; } cg_rtri;

/* The RAST globals Draw reads (rasteriser/Source/skeleton.cpp:30-86). */
typedef struct {
    int width, height;        /* SCREEN_WIDTH / SCREEN_HEIGHT (:21-22) */
    float focal;              /* focalLength (:30) */
    cg_vec4 camera;           /* cameraPos (:31) */
    float R[16];              /* R (:35) */
    cg_vec4 light_scene;      /* sceneCoordinatesLightPos (:52) */
    cg_vec3 light_power;      /* lightPower (:53) */
    float indirect_first;     /* indirectLightPowerPerArea at frame start (:54, :581-585):
                                 0.15 on the very first frame, 0.2 after the first
                                 colour-mode-0 fragment was shaded */
    int colour_mode;          /* randColourSelect (:81, SPACE key :408): 0 lit triangle colour,
                                 1 random colour, 2 night vision (:647-662) */
    float yaw;                /* yaw (:34): findU/findV (:1756-1825) map through inverse(R)
                                 when it is non-zero (texture modes 1-3 only) */
    uint64_t rand_offset;     /* modes 1-2: glibc rand() calls made before this frame (the
                                 reference never seeds: srand(1)); each shaded fragment
                                 consumes 3 (cg_stats.n_shaded) */
} cg_rast_params;

typedef struct {
    double kernel_ms;        /* device time of the frame's kernels (HIP events) */
    double total_ms;         /* host wall time of the call */
    int n_tris;              /* triangles rendered (RAST: after clipping) */
    int n_spans;             /* RAST: row spans produced by span setup */
    long long n_shaded;      /* RAST colour modes 1-2: fragments shaded (rand() calls / 3); -1 otherwise */
} cg_stats;

/* ---- context ---------------------------------------------------------- */
int  cg_create(int device, cg_ctx **out);
void cg_destroy(cg_ctx *ctx);
const char *cg_last_error(const cg_ctx *ctx);
/* Number of visible HIP devices (0 without a GPU); never fails loudly. */
int  cg_device_count(void);
/* Test hook: what the process's contexts and cg_dist handles hold right now -- out[0] device
 * allocations, out[1] pinned host allocations, out[2] events, out[3] streams.  A destroyed
 * context or handle leaves none behind. */
int  cg_debug_live(long long out[4]);

/* ---- raytracer -------------------------------------------------------- */
/* LoadTestModel (raytracer/Source/TestModelH.h:121-279): 28 triangles +
 * one sphere, scaled to [-1,1]^3.  Returns the triangle count. */
int cg_rt_load_test_model(cg_tri *tris, int cap, cg_sphere *sphere);
/* Build-defined workloads of SURVEY.md 8d (not in the reference; host-only,
 * no device work).  C4: n x n point lights at the cell centres of a square of
 * side `side` in the xz-plane centred on *centre, each with colour/(n*n);
 * light (i, j) -> out[j*n + i], x = c.x + side*(((float)i + 0.5f)/n - 0.5f),
 * z likewise with j.  Returns n*n.  C5: n random triangles from PCG32
 * (seed, stream 54): centroid ~ U[-1,1]^3, each vertex = centroid +
 * U[-0.02,0.02]^3, colour ~ U[0.15,0.75]^3, w = 1, normal by ComputeNormal
 * (TestModelH.h:96-105).  Returns n. */
int cg_rt_area_lights(const cg_light *centre, float side, int n, cg_light *out, int cap);
int cg_rt_random_scene(uint64_t seed, int n, cg_tri *out);
/* Upload the scene LoadTestModel built (TestModelH.h:121-279); kept device
 * resident until the next call.  Replaces the per-frame `vector<Triangle>`
 * the reference rebuilds in Draw (skeleton.cpp:113-116). */
int cg_rt_set_scene(cg_ctx *ctx, const cg_tri *tris, int n_tris,
                    const cg_sphere *spheres, int n_spheres);
/* cg_rt_set_scene for triangles that live in device memory (cg_tri, 76 B each); the spheres are
 * host memory.  d_tris is read after the work already queued on `stream` (NULL: the context's own),
 * so a producer kernel on that stream is ordered before it; the triangles are copied into the
 * context's buffer and on return the caller's buffer is no longer read.  Frames of the previous
 * scene still in flight on this context are waited for.  The context is left as cg_rt_set_scene
 * leaves it for the same bytes -- the scene bounds and, for n_tris > 64, the grid are computed on
 * the device (cg_rt_grid.hip) and equal the host's bit for bit -- so every later call works
 * unchanged.  Host waits, each a hipStreamSynchronize on `stream` after a small copy: one for the
 * reduced bounds, two for the grid's totals (candidate pairs, entries), and a closing one after
 * which frames may follow on any stream.  The grid is declined (frames then take the no-grid path,
 * as when the host builder gives up) when it would hold more entries than the entries cap or when
 * more candidate (triangle, cell) pairs would have to be tested than the candidates cap
 * (cg_rt_set_grid_caps); the host form has no candidates cap and, for scenes of many large thin
 * triangles, builds a grid this form declines. */
int cg_rt_set_scene_device(cg_ctx *ctx, const cg_tri *d_tris, int n_tris,
                           const cg_sphere *spheres /* host */, int n_spheres, void *stream);
/* Caps of the scene grid, 0 = default: `entries` (both forms; default 64 << 20) and `candidates`
 * (device form only; default 16 x the entries cap).  They apply to later scene changes. */
int cg_rt_set_grid_caps(cg_ctx *ctx, long long entries, long long candidates);
/* Host-only (no device work): the grid's sizing rule.  From the float minimum / maximum of the
 * vertices per axis and the triangle count: lo[3], h, inv_h, res[3].  Returns 1, or 0 for "no
 * grid" (n_tris <= 0 or bounds that are not finite; the outputs are then 0). */
int cg_rt_grid_dims(const float vmin[3], const float vmax[3], int n_tris, float lo[3], float *h,
                    float *inv_h, int res[3]);
/* Diagnostic: the installed grid.  Returns 1 and res / lo / h (each may be NULL), *n_start =
 * cells + 1 and *n_entries; with buffers, also start[cells + 1] and tris[entries] (CG_E_CAPACITY if
 * a given buffer is smaller).  Returns 0 when the scene has no grid (small scene, or declined). */
int cg_rt_grid_get(cg_ctx *ctx, int res[3], float lo[3], float *h, int *start, size_t start_cap,
                   int *tris, size_t tris_cap, size_t *n_start, size_t *n_entries);
/* Diagnostic: out = cells, entries, candidate pairs the device build tested (0 after a host
 * build), device bytes the device builder holds.  After a declined device build cells, candidates
 * and (when the entries cap declined it) entries are the declined grid's. */
int cg_rt_grid_info(cg_ctx *ctx, uint64_t out[4]);
/* Diagnostic: device time in ms of the latest device build's phases (bounds, ranges, count,
 * offsets, fill / order), -1 for a phase that did not run. */
int cg_rt_grid_phase_ms(cg_ctx *ctx, double out[5]);
/* One frame of raytracer Draw (skeleton.cpp:104-169): per pixel 3x3
 * sub-rays, ClosestIntersection (:263-363) and DirectLight (:366-415),
 * PutPixelSDL packing (SDLauxiliary.h:149-161).  Writes W*H ARGB into the
 * caller-owned host buffer `argb` (row-major, top row first), exactly what
 * the reference leaves in screen->buffer. */
int cg_rt_render(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                 uint32_t *argb, cg_stats *stats);   /* 0 <= n_lights <= 4096 */
/* n_frames successive Draw()s into caller-owned HOST memory (pageable, as
 * screen->buffer, or pinned): frame f with camera cams[f] at argb + f *
 * frame_stride pixels (0 = W*H), each what cg_rt_render leaves.  The frames
 * render `chunk` at a time (0 = 8) through cg_rt_render_frames_device into
 * device slots while the previous chunk downloads on a second stream (the
 * main loop of skeleton.cpp:91-94 with the D2H of frame N overlapped with
 * the render of later frames).  Returns once every frame is in host memory;
 * stats->kernel_ms spans the renders, total_ms the call. */
int cg_rt_render_frames(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                        int n_frames, uint32_t *argb, size_t frame_stride, int chunk, cg_stats *stats);
/* Device-resident form: renders this shard's rows into the caller-owned
 * device buffer d_out (cg_rt_shard_rows() rows of W pixels), enqueued on
 * `stream`, no synchronisation.  shard may be NULL (= whole frame). */
int cg_rt_render_device(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                        const cg_rt_shard *shard, uint32_t *d_out, void *stream);
/* n_frames successive frames (the reference's main loop: Update() moves the
 * camera, Draw() renders, raytracer/Source/skeleton.cpp:91-94 + :104-169),
 * frame f with camera cams[f] into d_out + f * frame_stride pixels
 * (frame_stride 0 = cg_rt_shard_rows() * W) in pix_format (CG_PIX_*; for
 * RGB24, d_out is a byte buffer and pixel offsets count 3 bytes; for
 * RGBA_F32, d_out is 16-byte aligned and pixel offsets count 16 bytes --
 * every route's kernel stores the float sums it holds, no ARGB frame in
 * between; padding rows are zero bytes; a column window is CG_E_INVALID).  All
 * cameras share width and height; lights and the shard are common.  Frames of
 * the unrotated one-light camera that differ only in cameraPos are rendered up
 * to 32 per kernel launch (a whole GPU's worth of tiles even for a small
 * shard); others are enqueued one by one.  Each frame equals
 * cg_rt_render_device's. */
int cg_rt_render_frames_device(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                               int n_frames, const cg_rt_shard *shard, void *d_out, size_t frame_stride,
                               int pix_format, void *stream);
/* Draw's float radiance and coverage, whole frame, synchronous: one
 * cg_rt_render_frames_device of a single CG_PIX_RGBA_F32 frame into context
 * scratch, then a download into the caller-owned host buffer rgba (W*H*4
 * floats, row-major, top row first).  CG_E_NOSCENE before a scene is set. */
int cg_rt_render_radiance(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                          float *rgba, cg_stats *stats);
/* d_argb[p] = PutPixelSDL(scale * (x, y, z) of d_rgba[p]) for n_pixels
 * CG_PIX_RGBA_F32 pixels (d_rgba 16-byte aligned), enqueued on `stream`, no
 * synchronisation.  scale 1.0f gives cg_rt_render_device's frame bit for bit
 * (x * 1.0f is exact); any other scale is the caller's exposure. */
int cg_rt_pack_radiance_device(cg_ctx *ctx, const float *d_rgba, size_t n_pixels, float scale,
                               uint32_t *d_argb, void *stream);

/* ---- Auto-exposure and tone mapping (cg_hdr.hip; arithmetic in csrc/cg_hdr.h) ----
 * Every step is integer arithmetic or single IEEE float32 operations in the
 * order stated, so kernels and host helpers agree bit for bit.
 *
 * Luminance  L = (0.2126f * x + 0.7152f * y) + 0.0722f * z.
 * Bin        a pixel is counted when L > 0.0f (+inf yes; NaN, +-0, negatives
 *            no); its bin is clamp((bits(L) >> 20) - 888, 0, 255): eight bins
 *            an octave from 2^-16 to 2^16, bin 0 also everything smaller, bin
 *            255 everything from 2^15 * 15/8 up.  The upper edge of bin b is
 *            the float with bits (888 + b + 1) << 20 (bin 255: 2^16).
 * Exposure   of frame f from its histogram h[256]: total = sum h,
 *            k = max(1, (total * permille + 999) / 1000) in 64 bits, b = the
 *            first bin whose running sum reaches k, t_f = target / edge(b)
 *            (1.0f when total == 0), then fminf(fmaxf(t_f, scale_min),
 *            scale_max).  s_0 = the previous scale where the caller gives one,
 *            else t_0; s_f = s_{f-1} + (t_f - s_{f-1}) * rate for f > 0.
 * Tone       per channel on v = c * s: LINEAR v; REINHARD v / (1.0f + v);
 *            REINHARD_WHITE (v * (1.0f + v / white2)) / (1.0f + v).  The
 *            result goes to PutPixelSDL unchanged. */
#define CG_HDR_BINS 256
#define CG_TONE_LINEAR 0
#define CG_TONE_REINHARD 1
#define CG_TONE_REINHARD_WHITE 2
/* Per-frame record beside a histogram, 32 bytes.  A plane has fewer than 2^32
 * pixels, so no count wraps.  n_dark: covered pixels with !(L > 0);
 * n_uncovered (4-float pixels only): pixels with !(w > 0.0f), neither counted
 * nor dark; max_bits / min_bits: over the bits of the counted pixels' L, 0 and
 * 0xFFFFFFFF when there are none.  All fields are order-independent. */
typedef struct {
    uint32_t n_counted, n_dark, n_uncovered, max_bits, min_bits;
    uint32_t pad[3];
} cg_hdr_stats;
/* permille 0..1000, rate in [0, 1] (1 = no adaptation), scale_min <= scale_max. */
typedef struct { int permille; float target, scale_min, scale_max, rate; } cg_hdr_exposure_params;
/* Host-only restatements (no device, no context).  cg_hdr_bin: -1 when L is
 * not counted.  cg_hdr_bin_edge: 0.0f for a bin outside 0..255.
 * cg_hdr_exposure: scales[f] = s_f for n_frames histograms of 256 counts each
 * (prev may be NULL); CG_E_INVALID for NULL pointers, n_frames < 0 or bad
 * parameters.  cg_hdr_tone: an unknown op is treated as LINEAR. */
float cg_hdr_luminance(float x, float y, float z);
int cg_hdr_bin(float L);
float cg_hdr_bin_edge(int bin);
int cg_hdr_exposure(const uint32_t *hist, int n_frames, const cg_hdr_exposure_params *params, const float *prev,
                    float *scales);
float cg_hdr_tone(int op, float v, float white2);
/* The device entry points below enqueue on `stream` (NULL: the context's) and
 * do not synchronise.  CG_E_INVALID: NULL or misaligned pointers, channels
 * outside {3, 4}, a stride below the plane, permille outside 0..1000, rate
 * outside [0, 1], scale_min > scale_max, an unknown tone op, white2 <= 0 where
 * it is used.  n_frames == 0 returns CG_OK and touches nothing.
 *
 * Histogram and record of n_frames planes of n_pixels pixels of `channels`
 * floats: 4 = CG_PIX_RGBA_F32 (16-byte aligned, w the coverage), 3 = a 3-float
 * plane such as the rasteriser's screen (every pixel covered).  Frame f starts
 * at d_pixels + f * frame_stride pixels (0: n_pixels); the pixels between
 * frames are never read.  Writes d_hist[f * 256 + b] and d_stats[f] (d_stats
 * may be NULL); the call clears both itself, on the stream. */
int cg_hdr_histogram_device(cg_ctx *ctx, const float *d_pixels, int channels, size_t n_pixels, int n_frames,
                            size_t frame_stride, uint32_t *d_hist, cg_hdr_stats *d_stats, void *stream);
/* d_scales[f] = s_f of the n_frames histograms at d_hist.  d_prev (a device
 * float, may be NULL) may point at an element of an earlier call's d_scales,
 * this call's array included as long as it is not one of its n_frames outputs. */
int cg_hdr_exposure_device(cg_ctx *ctx, const uint32_t *d_hist, int n_frames, const cg_hdr_exposure_params *params,
                           const float *d_prev, float *d_scales, void *stream);
/* d_argb[f * dst_stride + p] = PutPixelSDL(tone(op, c * d_scales[f])) of the
 * CG_PIX_RGBA_F32 pixel d_rgba[f * src_stride + p], p < n_pixels (strides in
 * pixels, 0: n_pixels); one launch for all frames, the scale read on the
 * device.  LINEAR with a scale of exactly 1.0f gives cg_rt_render_device's
 * frame bit for bit. */
int cg_rt_tonemap_pack_device(cg_ctx *ctx, const float *d_rgba, size_t n_pixels, int n_frames, size_t src_stride,
                              const float *d_scales, int op, float white2, uint32_t *d_argb, size_t dst_stride,
                              void *stream);
/* n_frames whole frames rendered, exposed and packed without a host wait:
 * frame f as ARGB8888 at d_argb + f * frame_stride pixels (0: W * H) and its
 * scale in d_scales[f] (device, n_frames floats, required).
 * per_frame_lights 0: the frames of cg_rt_render_frames_device; 1: those of
 * cg_rt_render_sequence_device, frame f lit by lights[f * n_lights ..].  The
 * frames go in chunks of 8 through those calls as CG_PIX_RGBA_F32 into scratch
 * the context owns (grow-only, 8 * W * H * 16 bytes), then histogram, exposure
 * and pack per chunk.  Frame 0 of the call takes d_prev (device, may be NULL)
 * as its previous scale, frame 0 of a later chunk d_scales[f - 1]: by the
 * definition above such a frame shows that scale itself, so the chunk of 8 is
 * part of what the call computes.  After the first call of a size it neither
 * allocates nor waits for the device.  CG_E_NOSCENE before a scene is set. */
int cg_rt_render_exposed_device(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                int n_frames, int per_frame_lights, const cg_hdr_exposure_params *params,
                                const float *d_prev, int op, float white2, uint32_t *d_argb, size_t frame_stride,
                                float *d_scales, void *stream);
/* Host-memory form, synchronous: the same frames into argb + f * frame_stride
 * pixels and the same scales into scales[n_frames] (both host memory; prev a
 * host float or NULL); each chunk's download follows its render. */
int cg_rt_render_exposed(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                         int per_frame_lights, const cg_hdr_exposure_params *params, const float *prev, int op,
                         float white2, uint32_t *argb, size_t frame_stride, float *scales, cg_stats *stats);

/* ---- Bloom (cg_bloom.hip; arithmetic in csrc/cg_bloom.h) ----
 * Glare around whatever exceeds the display range, between exposure and the tone curve.  A frame
 * is W x H pixels of CG_PIX_RGBA_F32 (x, y, z, w) with scale s.  Every line below is one IEEE
 * float32 operation or a select written as a ternary (a NaN takes the branch `false` names), in
 * the order stated; no FMA is formed, so kernels and host helpers agree bit for bit.
 *
 * Parameters  valid when 1 <= levels <= 6, threshold >= 0, 0 < cap <= 0x1p+64f and
 *             0 <= intensity <= 0x1p+32f (a NaN fails each comparison).  Under these limits every
 *             pyramid value and intensity * g are finite whatever the pixels and the scale hold.
 * 1 Bright    per channel c: c0 = c > 0.0f ? c : 0.0f; v = c0 * s; e = v - threshold;
 *             b = e > 0.0f ? e : 0.0f; b = b < cap ? b : cap.  A pixel with !(w > 0.0f) has b = 0
 *             in all three channels.  b is finite and in [0, cap]: a NaN gives 0, +inf gives cap.
 * 2 Sizes     W_0 = W, W_k = (W_{k-1} + 1) / 2, likewise H, k = 1 .. levels.  A level may be
 *             1 x 1, and the levels past it stay 1 x 1.
 * 3 Box       B_k(X, Y) = 0.25f * ((p(x0, y0) + p(x1, y0)) + (p(x0, y1) + p(x1, y1))) with
 *             x0 = 2X, x1 = min(2X + 1, W_{k-1} - 1), y0 = 2Y, y1 = min(2Y + 1, H_{k-1} - 1); p is
 *             b for k = 1 and B_{k-1} otherwise.
 * 4 Blur      separable, indices clamped to the level; t(d) the sample at offset d:
 *             a = t(-2) + t(2); q = t(-1) + t(1); r = (a * 0.0625f + q * 0.25f) + t(0) * 0.375f,
 *             each product and sum rounded on its own.  The horizontal pass runs over B_k, the
 *             vertical pass over its result and gives G_k.
 * 5 Up        from a coarse plane u (w x h) to fine pixel (X, Y): cx = X >> 1;
 *             nx = (X & 1) ? min(cx + 1, w - 1) : max(cx - 1, 0); likewise cy, ny;
 *             up = (0.5625f * u(cx, cy) + 0.1875f * u(nx, cy)) + (0.1875f * u(cx, ny) + 0.0625f * u(nx, ny)).
 * 6 Pyramid   U_levels = G_levels; U_k = G_k + up(U_{k+1}) for k = levels - 1 .. 1.  A pyramid
 *             pixel is four floats, the fourth +0.0f.  The pyramid of a frame is U_1, U_2, ...,
 *             U_levels one after the other: level k starts at sum_{j<k} W_j * H_j pixels.
 * 7 Composite of pixel (x, y): g = up(U_1) at (x, y) from W_1 x H_1; per channel v = base * s;
 *             m = intensity * g; v2 = v + m; then tone(op, v2, white2) and PutPixelSDL unchanged.
 *             CG_BLOOM_RULE_RT: base = c and every pixel is packed -- glow spills onto the
 *             background, so a pixel with w = 0 is no longer necessarily 0x80000000.
 *             CG_BLOOM_RULE_RAST: base = c > 0.0f ? c : 0.0f and a pixel with !(w > 0.0f) packs to
 *             0u: the border the reference never writes stays 0.  With intensity == 0 either rule
 *             gives cg_rt_tonemap_pack_device's / cg_rast_tonemap_pack_device's frame bit for bit. */
#define CG_BLOOM_MAX_LEVELS 6
#define CG_BLOOM_RULE_RT 0
#define CG_BLOOM_RULE_RAST 1
typedef struct { int levels; float threshold, cap, intensity; } cg_hdr_bloom_params;  /* 16 bytes */
/* Host-only (no device, no context).  cg_hdr_bloom_layout: widths / heights / offsets (pixels) of
 * levels 1 .. levels into arrays of `levels` entries and the pyramid's pixels into *total; any
 * pointer may be NULL; returns `levels`, or CG_E_INVALID for sizes <= 0 or levels outside 1..6.
 * cg_hdr_bloom: one frame's whole pyramid, total * 4 floats.  cg_hdr_bloom_pack: step 7 for one
 * frame; only level 1 of `pyr` is read.  Both: CG_E_INVALID for NULL pointers, invalid
 * parameters, sizes <= 0, an unknown rule or tone op. */
int cg_hdr_bloom_layout(int width, int height, int levels, int *widths, int *heights, size_t *offsets, size_t *total);
int cg_hdr_bloom(const float *rgba, int width, int height, float scale, const cg_hdr_bloom_params *bloom, float *pyr);
int cg_hdr_bloom_pack(const float *rgba, const float *pyr, int width, int height, float scale,
                      const cg_hdr_bloom_params *bloom, int rule, int op, float white2, uint32_t *argb);
/* The pyramids of n_frames frames, enqueued on `stream` (NULL: the context's) without a host
 * wait.  Frame f is read at d_rgba + f * src_stride pixels and its pyramid goes to d_pyr + f *
 * pyr_stride pixels (strides in 16-byte pixels; 0: W * H and `total`); its scale is read on the
 * device from d_scales[f].  The unblurred planes B_k live in grow-only scratch the context owns.
 * That scratch (and the pyramids of the exposed calls below) is one set of buffers per context, used
 * on whatever stream a call names: calls on one context that use it must be ordered among
 * themselves, by one stream or by events; calls on different contexts are independent.
 * Pixels between frames are neither read nor written.  CG_E_INVALID as the cg_hdr_* calls, and
 * for invalid bloom parameters, a stride below its plane, W * H >= 2^32; n_frames == 0 returns
 * CG_OK and touches nothing. */
int cg_hdr_bloom_device(cg_ctx *ctx, const float *d_rgba, int width, int height, int n_frames, size_t src_stride,
                        const float *d_scales, const cg_hdr_bloom_params *bloom, float *d_pyr, size_t pyr_stride,
                        void *stream);
/* Step 7 over n_frames frames: d_argb[f * dst_stride + p] from d_rgba[f * src_stride + p] and
 * level 1 of the pyramid at d_pyr + f * pyr_stride (strides as above; dst_stride in pixels, 0: W * H). */
int cg_hdr_bloom_pack_device(cg_ctx *ctx, const float *d_rgba, const float *d_pyr, int width, int height, int n_frames,
                             size_t src_stride, size_t pyr_stride, const float *d_scales,
                             const cg_hdr_bloom_params *bloom, int rule, int op, float white2, uint32_t *d_argb,
                             size_t dst_stride, void *stream);
/* cg_rt_render_exposed_device / cg_rt_render_exposed with bloom: a chunk of 8 frames is rendered
 * float, then histogram, exposure, bloom and the composite (rule RT), the pyramids in scratch the
 * context owns.  The scales are exactly those of the call without bloom.  bloom == NULL runs that
 * call's chunk unchanged.  After the first call of a size it neither allocates nor waits. */
int cg_rt_render_exposed_bloom_device(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                      int n_frames, int per_frame_lights, const cg_hdr_exposure_params *params,
                                      const float *d_prev, int op, float white2, const cg_hdr_bloom_params *bloom,
                                      uint32_t *d_argb, size_t frame_stride, float *d_scales, void *stream);
int cg_rt_render_exposed_bloom(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                               int n_frames, int per_frame_lights, const cg_hdr_exposure_params *params,
                               const float *prev, int op, float white2, const cg_hdr_bloom_params *bloom,
                               uint32_t *argb, size_t frame_stride, float *scales, cg_stats *stats);

/* Frame assembly after a transfer of band shards: d_src holds n_blocks row
 * blocks in order, block b = n_frames x rows[b] rows of `width` pixels in
 * pix_format, landing at frame rows row0[b] .. row0[b] + rows[b] - 1 (rows
 * outside the frame are skipped) of frame f = d_frames + f * frame_stride
 * pixels (ARGB8888).  With cols > 0 the source rows hold only the window
 * columns col0 .. col0 + cols - 1 (4-aligned) and the rest of each row is set
 * to 0x80000000.  row0 / rows are host arrays, n_blocks <= 64.
 * CG_PIX_RGBA_F32 is CG_E_INVALID here (no multi-GPU transfer of float frames). */
int cg_rt_assemble_device(cg_ctx *ctx, const void *d_src, int pix_format, const int *row0, const int *rows,
                          int n_blocks, int width, int height, int n_frames, uint32_t *d_frames,
                          size_t frame_stride, int col0, int cols, void *stream);
/* The columns an unrotated camera can see anything in: every sub-ray of the
 * pixels outside [*col0, *col1) certainly misses all triangles and spheres,
 * so those pixels are PutPixelSDL(0, 0, 0) = 0x80000000 (skeleton.cpp:160-166).
 * From the scene's bounding box widened by 0.02 (every accepted float hit
 * lies within ~1e-6 relative of its triangle and within 4e-3 |cameraPos -
 * centre| of its sphere), projected through the pinhole (the projection of a
 * box in front of the camera lies in the hull of its corners' projections),
 * plus 2 pixels, rounded out to 16-pixel boundaries.  Returns the full width
 * for rotated cameras or when the box reaches behind the camera.  Host-only
 * (no device work), usable to crop CG_PIX_RGB24 transfers (cg_rt_shard). */
int cg_rt_frame_columns(const cg_tri *tris, int n_tris, const cg_sphere *spheres, int n_spheres,
                        const cg_rt_camera *cam, int *col0, int *col1);
/* Rows a shard renders (including padding rows of its last stripe). */
int cg_rt_shard_rows(int height, const cg_rt_shard *shard);
/* Which kernels a frame of this shape takes (host-only, no device work):
 * CG_RT_ROUTE_* below, or CG_E_INVALID.  The lattice kernels share sub-rays
 * between pixels (half-pixel columns for an unrotated camera, per-pixel
 * columns with shared rows under a yaw); the large-scene path (n_tris > 64)
 * has the same two lattice modes and a per-pixel mode.  Every route gives
 * the reference's image; this only says how. */
enum {
    CG_RT_ROUTE_PIXEL = 0,            /* rt_pixel_kernel: 9 sub-rays per pixel */
    CG_RT_ROUTE_LATTICE = 1,          /* rt_lattice_kernel, one light */
    CG_RT_ROUTE_LATTICE_YAW = 2,      /* the same, per-pixel columns */
    CG_RT_ROUTE_LIGHTS = 3,           /* rt_lattice_lights_kernel, 2..64 lights */
    CG_RT_ROUTE_LIGHTS_YAW = 4,
    CG_RT_ROUTE_BIG_PIXEL = 5,        /* large scene, per-pixel mode */
    CG_RT_ROUTE_BIG_LATTICE = 6,      /* large scene, lattice mode */
    CG_RT_ROUTE_BIG_LATTICE_YAW = 7
};
int cg_rt_route(const cg_rt_camera *cam, int n_tris, int n_spheres, int n_lights, const cg_rt_shard *shard);
/* n_frames successive Draw()s as the main loop makes them after any keys of Update()
 * (skeleton.cpp:192-256): frame f with camera cams[f] and lights
 * lights[f * n_lights .. f * n_lights + n_lights - 1]; n_lights is common
 * (0 <= n_lights <= 4096; lights may be NULL when it is 0), width/height common.
 * Frame f equals cg_rt_render_device(ctx, lights + f * n_lights, n_lights, &cams[f], shard, ...).
 * Output, shard, frame_stride, pix_format, stream as cg_rt_render_frames_device.
 * The lights and a per-frame table (cameraPos, focal, indirect, R, the light-set
 * summary) are uploaded once per call; consecutive frames on the same lattice route
 * (cg_rt_sequence_runs) share launches of up to 32 frames whatever they differ in.
 * Calls may be queued back to back without a synchronise between them: two calls in flight keep
 * their own lights and tables.  A third call issued while the first call's upload has not yet run
 * (it is the first thing that call enqueues) blocks the host until it has; apart from that, and
 * after the first call of a size, a call neither allocates nor waits for the device. */
int cg_rt_render_sequence_device(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                 int n_frames, const cg_rt_shard *shard, void *d_out, size_t frame_stride,
                                 int pix_format, void *stream);
/* Host-memory form, pipelined like cg_rt_render_frames (chunks render while the previous chunk downloads). */
int cg_rt_render_sequence(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                          uint32_t *argb, size_t frame_stride, int chunk, cg_stats *stats);
/* Host-only (no device work): how a sequence is launched.  Consecutive frames on the same route
 * (CG_RT_ROUTE_*; size, shard and light count are the call's) form a run; run r covers frames
 * run_start[r] .. run_start[r+1]-1 and takes run_route[r].  Writes min(runs, cap) runs: run_route
 * holds cap entries, run_start cap + 1 (the entry after the last written run closes it).  Frames
 * of a lattice run may differ in cameraPos, focal, indirect, the yaw angle and every light; a
 * change of route (unrotated <-> yawed, lattice <-> per-pixel) ends the run.  Returns the number
 * of runs (may exceed cap: the caller re-sizes) or CG_E_INVALID. */
int cg_rt_sequence_runs(const cg_rt_camera *cams, int n_frames, int n_tris, int n_spheres, int n_lights,
                        const cg_rt_shard *shard, int *run_start, int *run_route, int cap);
/* Reassemble a frame from gathered shards: d_gathered holds nranks blocks of
 * cg_rt_shard_rows() rows each, in rank order. */
int cg_rt_unstripe_device(cg_ctx *ctx, const uint32_t *d_gathered, int width, int height,
                          int nranks, int stripe_h, uint32_t *d_frame, void *stream);
/* Batched form: d_gathered holds, per rank in rank order, `nframes` shards of
 * cg_rt_shard_rows() rows each (frame-major); d_frames receives nframes
 * frames of W*H.  Lets a caller gather several frames per collective. */
int cg_rt_unstripe_batch_device(cg_ctx *ctx, const uint32_t *d_gathered, int width, int height,
                                int nranks, int stripe_h, int nframes, uint32_t *d_frames, void *stream);
/* Single-ray probes for known-answer tests: device evaluation of
 * ClosestIntersection (:263-363) and DirectLight (:366-415) on n rays. */
int cg_rt_probe_closest(cg_ctx *ctx, const cg_vec4 *starts, const cg_vec4 *dirs, int n,
                        cg_isect *out, int *hit);
int cg_rt_probe_direct_light(cg_ctx *ctx, const cg_isect *isects, const cg_light *light, int n,
                             cg_vec3 *out);
/* ---- per-pixel hit records and picking --------------------------------------
 * Every sub-ray Draw traces ends in an Intersection (skeleton.cpp:40-45, 263-363); these calls hand
 * it back instead of a colour.  No light set is involved.  They work for any R, do not disturb
 * frames in flight (a large scene's hits-only pass has buffers of its own) and leave later renders
 * on the context unchanged. */
enum { CG_RT_HIT_NONE = INT32_MIN };   /* d_index: triangle k >= 0, sphere q as -1 - q, else this */

/* Host-only, no device work: the ray Draw traces for pixel (x, y), sub-ray s = 3 (i + 1) + (j + 1)
 * (skeleton.cpp:126-137; s = 4 is the pixel centre): start = cameraPos, dir = (d.x + 0.5 i,
 * d.y + 0.5 j, focal, 1) with d = R * (x - W/2, y - H/2, focal, 1), formed with the library's own
 * matrix product, so that it is the ray every kernel forms.  CG_E_INVALID for sub_ray outside 0..8
 * or a pixel outside the frame. */
int cg_rt_pixel_ray(const cg_rt_camera *cam, int x, int y, int sub_ray, cg_vec4 *start, cg_vec4 *dir);

/* ClosestIntersection of sub-ray `sub_ray` (0..8) of every pixel of this shard's rows, enqueued on
 * `stream`, no synchronisation after the first call of a scene or frame shape (a large scene sizes
 * its list pools then, as its first frame does).  Any of the three outputs may be NULL, not all
 * three.  The planes are cg_rt_shard_rows() rows of W, row-major, like cg_rt_render_device's output.
 * d_isect[p] holds exactly the bytes cg_rt_probe_closest writes for that pixel's ray, the miss record
 * included (distance FLT_MAX, position 0, both indices 0); d_index[p] is as the enum says;
 * d_distance[p] is the record's distance.  Padding rows of the last stripe are misses.
 * Scenes of at most 64 triangles test every triangle per pixel; larger ones run the large-scene
 * path's certificate and list passes and a walk of one ray per pixel (no shadow or shading pass);
 * cg_rt_scratch_info / cg_rt_pool_demand report for it, and a pool overflow takes the same fallback
 * over every triangle.  CG_E_NOSCENE before a scene is set; CG_E_INVALID for sub_ray outside 0..8
 * or all outputs NULL. */
int cg_rt_hits_device(cg_ctx *ctx, const cg_rt_camera *cam, int sub_ray, const cg_rt_shard *shard,
                      cg_isect *d_isect, int32_t *d_index, float *d_distance, void *stream);
/* Host-memory form, whole frame (H rows of W), synchronous. */
int cg_rt_hits(cg_ctx *ctx, const cg_rt_camera *cam, int sub_ray, cg_isect *isect, int32_t *index, float *distance);
/* One pixel, synchronous, without building a frame's lists: every triangle against the one ray,
 * workgroups striding over the scene, the lexicographic minimum of (distance, index).  *out is the
 * record cg_rt_hits gives for the pixel, *hit whether anything was hit.  CG_E_INVALID for a pixel
 * outside the frame. */
int cg_rt_pick(cg_ctx *ctx, const cg_rt_camera *cam, int x, int y, int sub_ray, cg_isect *out, int *hit);

/* DirectLight's three divides by one area (:412) as the light-set sweep performs
 * them (a shared reciprocal inside a range guard, IEEE x / d outside it), on
 * device arrays: d_q[3i + k] = d_x[3i + k] / d_den[i]; a test that they are
 * IEEE-exact. */
int cg_rt_probe_div3_device(const float *d_x, const float *d_den, int n, float *d_q, void *stream);
/* r_magnitude (:371), the FP64 norm of a float vector rounded to float, as the
 * one-light lattice kernels form it (the compiler's sqrt(double) without its
 * range scaling), on device arrays: d_m[i] = |(d_r[3i], d_r[3i + 1], d_r[3i + 2])|;
 * a test that it is float(sqrt(double sum)) bit for bit. */
int cg_rt_probe_rmag_device(const float *d_r, int n, float *d_m, void *stream);
/* Test hook for large scenes (n_tris > 64): capacity of the device queue of
 * shadow rays the blocker hints leave to the certified lit search (0 = the
 * default, 65536).  Rays past the queue are searched per pixel by the shading
 * kernel instead; the image is the same either way. */
int cg_rt_set_pending_cap(cg_ctx *ctx, int cap);
/* Large-scene scratch after the latest frame (waits for it): out[0] device
 * bytes held, out[1] entries the frame listed in the pools (super-bin, bin,
 * bucketed and shadow lists), out[2] the pools' capacity in entries, out[3]
 * frames that overflowed a pool (rendered correctly through the fallback). */
int cg_rt_scratch_info(cg_ctx *ctx, uint64_t *out);
/* Large-scene list demand of the latest frame, per pool (waits for it): out[0]
 * super-bin lists, out[1] bin lists, out[2] many-light shadow lists, out[3]
 * bucketed (per half-bin) lists, in entries. */
int cg_rt_pool_demand(cg_ctx *ctx, uint64_t *out);
/* Diagnostic: the lattice tile certificates of frame `frame` of the latest
 * lattice call on this context (waits for it).  info[0..3] = tile columns,
 * tile rows, shadow masks per object a tile holds (0: none were built) and
 * the call's frames.  masks (optional): two 64-bit words per tile, row-major
 * -- the primary mask (bit k: triangle k may be hit; bit 63: a sphere; bit
 * 62: the one candidate covers the tile) and the shadow mask (bit k: triangle
 * k may block a shadow ray of the tile; bit 63: a sphere).  obj_masks
 * (optional): info[2] words per tile -- word j < info[2] - 1 the shadow mask
 * for hits on the j-th set triangle of the primary mask, the last word for
 * hits on a sphere.  With both null only info is filled. */
int cg_rt_tile_masks(cg_ctx *ctx, int frame, uint64_t *masks, uint64_t *obj_masks, int *info);
/* Diagnostic: how the latest batched one-light lattice call on this context
 * (cg_rt_render_frames_device and the calls built on it) launched its lattice
 * kernel.  info[0] = the dispatch order (0 default, 1 frame-major measured,
 * 2 interleaved measured), info[1] = 1 when its workgroups waited for
 * certificates published beside the launch (CG_CERT_CONC=1 on a call in the
 * default order), info[2] = 1 when every workgroup was forced onto the
 * uncertified path (CG_LAT_FORCE_UNCERT=1), info[3] = its workgroups.  All 0
 * before any such call. */
int cg_rt_lattice_path(cg_ctx *ctx, int *info);
/* Test hook: pin the large-scene pool capacities (entries: super-bin, bin,
 * many-light shadow and bucketed lists; all 0 = automatic sizing).  Lists past a capacity take the fallback over every triangle; the
 * image is the same. */
int cg_rt_set_pool_caps(cg_ctx *ctx, long long sup, long long bin, long long sbin, long long sorted);
/* Test hook, a defect detector for the certificate machinery (never a product
 * path): rows row0 .. row0 + rows - 1 of the camera's frame (rows x width
 * pixels into d_out, device memory) by the reference's own loop with no
 * acceleration at all -- every sub-ray against every triangle and sphere, every
 * shadow ray against every triangle and sphere until its first blocker
 * (raytracer/Source/skeleton.cpp:120-166, 263-415).  Synchronous; at most 64
 * lights.  C5 at 1080p: tens of seconds on one MI355X. */
int cg_rt_render_brute_device(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                              int row0, int rows, uint32_t *d_out, void *stream);

/* ---- multi-GPU raytracer ------------------------------- */
/* One process per GPU.  The reference renders every pixel of Draw
 * (raytracer/Source/skeleton.cpp:104-169) on one CPU thread; pixels are
 * independent, so N GPUs each render one contiguous band of frame rows and
 * rank 0 assembles the frames: ranks > 0 render their band in CG_PIX_RGB24
 * (only the columns the camera can see anything in, cg_rt_frame_columns) and
 * send it to rank 0 with RCCL point-to-point over xGMI (every peer has its own
 * link to rank 0); rank 0 renders its own band straight into the frames and
 * expands the received bands in place (cg_rt_assemble_device).  Frames are
 * processed in chunks: the transfer of chunk j overlaps the render of chunk
 * j + 1.  A cg_dist is bound to one context and is not thread-safe. */
typedef struct cg_dist cg_dist;
typedef struct { char bytes[128]; } cg_dist_id;    /* an RCCL unique id (ncclUniqueId) */
/* Rank 0 creates the id and hands it to every rank (MPI, sockets, ...). */
int cg_dist_unique_id(cg_dist_id *id);
/* Collective over the nranks processes: RCCL communicator on ctx's device.
 * Every host wait of the multi-GPU path is bounded: the communicator is
 * non-blocking, and init, cg_dist_rebalance, cg_dist_last_times, cg_dist_wait
 * and cg_dist_destroy poll completion and the communicator's asynchronous
 * error against a deadline (default: CG_DIST_TIMEOUT_MS from the environment,
 * else 60000 ms).  An RCCL error returns CG_E_HIP and a passed deadline
 * CG_E_TIMEOUT; either aborts the communicator (ncclCommAbort: kernels still
 * waiting on a peer exit) and every later call on the handle fails CG_E_HIP.
 * A missing peer therefore ends the job with an error instead of a hang.
 * The deadline runs from the last progress of a wait (its start, or the
 * latest of its events seen complete), but one event covers everything queued
 * before it: cg_dist_wait's deadline must exceed the rank's queued backlog.
 * If the abort itself does not return within 10 s it is left running and
 * cg_dist_destroy deliberately leaks the handle's device buffers and transfer
 * stream (RCCL kernels may still be using them). */
int cg_dist_create(cg_ctx *ctx, int nranks, int rank, const cg_dist_id *id, cg_dist **out);
/* cg_dist_create with an explicit deadline in ms (0: the default above). */
int cg_dist_create_timed(cg_ctx *ctx, int nranks, int rank, const cg_dist_id *id, int timeout_ms, cg_dist **out);
/* Deadline (ms, > 0) of every later host wait on this handle. */
int cg_dist_set_timeout(cg_dist *d, int timeout_ms);
/* Bounded host wait until this rank's work of its calls so far has drained:
 * `stream` (NULL: the last call's stream) and the transfer stream.  0, or
 * CG_E_TIMEOUT / CG_E_HIP after aborting the communicator.  Use it instead of
 * an unbounded device synchronise after cg_rt_render_frames_dist. */
int cg_dist_wait(cg_dist *d, void *stream);
/* In-process transport for tests: nranks contexts (any devices, possibly one)
 * in one process and thread, one cg_dist per rank in outs[]; bands move by
 * device-to-device copies.  Each render call must be made on ranks
 * nranks-1 .. 1 before rank 0 (their work is only enqueued). */
int cg_dist_create_local(cg_ctx *const *ctxs, int nranks, cg_dist **outs);
void cg_dist_destroy(cg_dist *d);
/* Band partition: rank r renders rows row0[r] .. row0[r] + rows[r] - 1; the
 * bands must tile [0, height) in rank order.  Default (and after a height
 * change): equal bands on multiples of 15 rows (the lattice tile height). */
int cg_dist_set_bands(cg_dist *d, int height, const int *row0, const int *rows);
int cg_dist_get_bands(const cg_dist *d, int *row0, int *rows);
/* Frames per chunk of the render/transfer pipeline (default 4). */
int cg_dist_set_chunk(cg_dist *d, int frames);
/* Pipeline: CG_DIST_SIGNALLED (the default where the device supports stream
 * waits on memory) renders a call's frames in full-size launches and sends
 * each chunk when its frames' tiles are all stored (per-frame completion
 * counts); CG_DIST_CHUNKED launches each chunk separately and orders the
 * transfers with events. */
#define CG_DIST_SIGNALLED 0
#define CG_DIST_CHUNKED 1
int cg_dist_set_pipeline(cg_dist *d, int mode);
/* Collective: new bands from every rank's measured render time per frame in
 * its last cg_rt_render_frames_dist call (cost density uniform within each
 * old band; rank 0 also pays the assembly), so the bands take equal time. */
int cg_dist_rebalance(cg_dist *d);
/* This rank's device time per frame in its last cg_rt_render_frames_dist
 * call (waits for it): its band's render and, on rank 0, the assembly. */
int cg_dist_last_times(cg_dist *d, double *render_ms_per_frame, double *assemble_ms_per_frame);
/* Collective: n_frames frames (cams as cg_rt_render_frames_device; one size),
 * assembled on rank 0 into d_frames + f * frame_stride pixels (ARGB8888;
 * frame_stride 0 = W*H).  d_frames is ignored on ranks > 0.  Enqueued on
 * `stream` (NULL: the context's); when `stream` has drained, rank 0's frames
 * are complete. */
int cg_rt_render_frames_dist(cg_dist *d, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                             int n_frames, uint32_t *d_frames, size_t frame_stride, void *stream);
/* Host-only: contiguous bands minimising max_r (sum of row_cost over band r
 * + overhead[r]) (overhead may be NULL); every rank gets >= 1 row when
 * height >= nranks. */
int cg_dist_band_partition(const double *row_cost, int height, int nranks, const double *overhead, int *row0,
                           int *rows);

/* ---- rasteriser ------------------------------------------------------- */
/* glibc rand() as colour modes 1-2 consume it (seed 1, never reseeded by the
 * reference): n values starting at call index `offset`.  Host-only probe of
 * the generator the device path uses (jump-ahead restatement of glibc's
 * TYPE_3 random_r). */
int cg_glibc_rand(uint64_t offset, int n, int32_t *out);
/* LoadTestModel (rasteriser/Source/TestModelH.h:48-312) with texture
 * selectors 0: room (10) and boxes (20). Returns n_room + n_boxes. */
int cg_rast_load_test_model(cg_rtri *room, int room_cap, int *n_room, cg_rtri *boxes,
                            int boxes_cap, int *n_boxes);
/* Host geometry of rasteriser Draw (skeleton.cpp:205-241): camera space
 * (:701-716), createShadowVolume (:1676-1722), rotation by R (:223-228),
 * clip space w = z/f (:691-699), clip planes 1..6 (:720-1673).  Writes the
 * ordered clipped triangle list (up to `cap`) and the rotated camera-space
 * light; returns the triangle count (may exceed cap: CG_E_CAPACITY is not
 * raised, the caller re-sizes) or a negative error. */
int cg_rast_prepare(const cg_rast_params *p, const cg_rtri *room, int n_room,
                    const cg_rtri *boxes, int n_boxes, cg_rtri *out, int cap,
                    cg_vec4 *light_out);
/* One frame of the rasteriser fill + post-pass (skeleton.cpp:243-307):
 * DrawPolygon / VertexShader / ComputePolygonRows / DrawPolygonRows /
 * Interpolate / PixelShader / calculateIllumination over the ordered list,
 * then surroundingShadowSum + antiAliasing + PutPixelSDL.  Outputs are
 * caller-owned host buffers of W*H (any may be NULL except argb):
 * argb = screen->buffer, depth = depthBuffer, shadow = shadowBuffer. */
int cg_rast_render(cg_ctx *ctx, const cg_rtri *tris, int n, const cg_rast_params *p,
                   cg_vec4 light, uint32_t *argb, float *depth, int32_t *shadow,
                   cg_stats *stats);
/* Device-resident form: triangles already on the device (d_tris), outputs
 * into caller-owned device buffers (d_depth / d_shadow may be NULL). */
int cg_rast_render_device(cg_ctx *ctx, const cg_rtri *d_tris, int n, const cg_rast_params *p,
                          cg_vec4 light, uint32_t *d_argb, float *d_depth, int32_t *d_shadow,
                          void *stream);

/* Whole rasteriser Draw on the device (skeleton.cpp:203-308): upload the
 * LoadTestModel room/boxes once, then each frame runs the geometry
 * (shadow volumes, rotation, clip) AND the fill + post-pass on the GPU --
 * the same lists cg_rast_prepare builds on the host.
 * n_room + 7 * n_boxes (a box triangle brings its 6 shadow-volume triangles)
 * may be up to 4194304; above that CG_E_INVALID with a message.
 *
 * cg_rast_draw_device on the dense route (below) only enqueues and never
 * waits.  On the compact route it waits on the host, on `stream`, for the
 * frame's own counts -- the clipped triangle count, then the span total, then
 * the record total and the longest row -- and allocates exactly what the frame
 * needs, grow-only: no pool can overflow and there is no fallback path.  (So a
 * compact-route frame cannot be captured into a graph.)  cg_rast_render_device
 * on the compact route waits likewise for the last two.  A colour mode 1-2
 * frame on the compact route waits twice more, for its segment total and for
 * its shaded-fragment count S (the rand() stream is sized by it), and returns
 * after the frame ran, as the dense route's colour modes do. */
int cg_rast_set_scene(cg_ctx *ctx, const cg_rtri *room, int n_room, const cg_rtri *boxes, int n_boxes);
int cg_rast_draw(cg_ctx *ctx, const cg_rast_params *p, uint32_t *argb, float *depth, int32_t *shadow,
                 cg_stats *stats);
int cg_rast_draw_device(cg_ctx *ctx, const cg_rast_params *p, uint32_t *d_argb, float *d_depth,
                        int32_t *d_shadow, void *stream);

/* The buffers Draw leaves behind besides the picture (skeleton.cpp:243-307), and what lies
 * under each pixel.  screen / low / high: the float vec3 globals screenBuffer, lowLightBuffer,
 * highLightBuffer as they stand when Draw returns -- `screen` with the post-pass darkening
 * (:286-303, interior pixels, subtracted once); colour modes 1-2 leave low and high at 0 (the
 * reference only clears them); a pixel no fragment wrote is 0, or -dk on `screen` where a
 * shadow mark darkened the background.  The owner of a pixel is the fragment that last wrote
 * screenBuffer[y][x] in drawing order (:574-661): a shadow-volume triangle never owns, and a
 * fragment of texture 2/3 on a transparent texel sets the depth to 0 without owning (the
 * earlier owner stays, so depth is not always the owner's zinv).  clip: the owner's index in
 * the frame's clipped list (cg_rast_prepare's order); tri: its input triangle for the draw
 * entries (room k -> k, boxes[k] -> n_room + k; the render entries' list is the clipped list:
 * tri = clip); pos: the owner fragment's pos3d as Interpolate leaves it (:546-549),
 * (X / zinv, Y / zinv, 1 / zinv, 1).  Without an owner clip = tri = CG_RAST_OWNER_NONE and
 * pos = 0.  Every plane is W * H entries, row-major; any may be NULL, not all. */
enum { CG_RAST_OWNER_NONE = -1 };
typedef struct {
    uint32_t *argb; float *depth; int32_t *shadow;   /* as cg_rast_draw's; each may be NULL */
    float *screen, *low, *high;   /* 3 floats per pixel (x, y, z of the vec3), row-major, W*H*3 */
    int32_t *clip;                /* owner: index in the frame's clipped list (cg_rast_prepare's order) */
    int32_t *tri;                 /* owner: input triangle -- room k -> k, boxes[k] -> n_room + k */
    cg_vec4 *pos;                 /* owner fragment's pos3d as Interpolate leaves it (:546-549) */
} cg_rast_buffers;                /* at least one pointer non-NULL */
/* A call runs the frame cg_rast_draw_device / cg_rast_render_device would run for the same
 * parameters (route, colour modes, rand_offset, indirect_first, textures, what waits on which
 * route, n_shaded, cg_rast_scratch_info afterwards; without argb the post-pass is skipped), then
 * one more kernel on the same stream that fills the other planes from the frame's scratch.  In
 * colour modes 1-2 the ordered z-buffer's fill runs once more for the owner.  kernel_ms in the
 * stats covers the frame's own kernels.  CG_E_INVALID when every pointer is NULL. */
int cg_rast_draw_buffers_device(cg_ctx *ctx, const cg_rast_params *p, const cg_rast_buffers *d, void *stream);
int cg_rast_draw_buffers(cg_ctx *ctx, const cg_rast_params *p, const cg_rast_buffers *h, cg_stats *stats);
int cg_rast_render_buffers_device(cg_ctx *ctx, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light,
                                  const cg_rast_buffers *d, void *stream);
int cg_rast_render_buffers(cg_ctx *ctx, const cg_rtri *tris, int n, const cg_rast_params *p, cg_vec4 light,
                           const cg_rast_buffers *h, cg_stats *stats);
/* Synchronous: the tri / clip / pos the planes hold at (x, y) (each may be NULL), *hit = 0
 * without an owner.  Runs the frame's passes through the fill into context scratch (no
 * post-pass; a colour mode 1-2 pick draws nothing from the rand() stream) and gathers the one
 * pixel: no output plane is allocated or written for it.  CG_E_INVALID for a pixel outside the
 * frame, CG_E_NOSCENE before cg_rast_set_scene. */
int cg_rast_pick(cg_ctx *ctx, const cg_rast_params *p, int x, int y, int32_t *tri, int32_t *clip, cg_vec4 *pos,
                 int *hit);
/* Host-only: the bytes of the state word the latest frame's ordered z-buffer left per pixel
 * for the buffers kernel (2 below 32768 records a row, else 4; 0 before a frame). */
int cg_rast_state_bytes(cg_ctx *ctx);

/* Two routes render the same Draw, every plane bit for bit the same.  DENSE:
 * spans and row records sized at list capacity x H, the kernels of the
 * coursework scene.  COMPACT (large scenes): scratch and work follow what the
 * frame covers -- spans packed per triangle, a row's records packed in
 * triangle order by a stable counting sort of the spans.  cg_rast_route
 * (host-only) is the automatic choice: DENSE for list_capacity <= 131072,
 * else COMPACT; list_capacity is 32 * (n_room + 7 * n_boxes) for the
 * cg_rast_draw* entries and n for cg_rast_render*.  A colour mode 1-2 frame
 * takes COMPACT already for list_capacity > 20480: the dense route's colour
 * fill counts fragments per list slot in LDS (8 bytes a slot, 160 KiB); a
 * cg_rast_draw_sequence_device call with such a frame runs all its frames
 * there.  A forced dense route or a route limit that puts such a frame on the
 * dense route fails with CG_E_INVALID and a message.
 * The compact route serves cg_rast_draw, cg_rast_draw_device, cg_rast_render
 * and cg_rast_render_device in colour modes 0-2 with texture modes 0-3 (modes
 * 1-2 ignore textures, as the reference does) and the indirect_first rule;
 * cg_rast_draw_frames_device and cg_rast_draw_sequence_device run its frames
 * one after another on `stream` (no lanes: each would hold its own copy of
 * the scratch).  Its colour modes 1-2 number the shaded fragments from the
 * span order itself (triangle, row, 64-pixel segment) and generate exactly
 * 3 S rand() values; the 16-byte state, the segment counts and the stream are
 * held only once a mode 1-2 frame ran, grow-only, and count in
 * cg_rast_scratch_info's out[0]. */
enum { CG_RAST_ROUTE_DENSE = 0, CG_RAST_ROUTE_COMPACT = 1 };
int cg_rast_route(long long list_capacity);
/* Test and A/B hook for colour mode 0: -1 automatic (the default), 0 forces
 * DENSE, 1 forces COMPACT for this context's frames (its lanes follow).  A
 * forced dense cg_rast_draw* of more than 4096 input triangles fails with
 * CG_E_INVALID; so does a colour mode 1-2 frame forced onto the compact route
 * (with a message): modes 1-2 take that route on the automatic choice only. */
int cg_rast_set_route(cg_ctx *ctx, int route);
/* Test and A/B hook: the list capacity above which this context's frames take the compact
 * route on the automatic choice; 0 = the default (131072, what cg_rast_route applies).
 * Negative: CG_E_INVALID. */
int cg_rast_set_route_limit(cg_ctx *ctx, long long list_capacity);
/* Host-only: the 64-pixel fill segments that the visible extent [max(lx, 0), min(rx, width))
 * of a span with fragments x in [lx, rx) overlaps -- the entries the compact route's colour
 * modes 1-2 keep for it.  Returns their number (0: nothing on screen) and writes the first
 * segment to *first (may be NULL). */
int cg_rast_span_segments(int lx, int rx, int width, int *first);
/* Rasteriser scratch after the latest rasteriser frame (waits for it, on the
 * stream it ran on): out[0] device bytes held for rasteriser scratch (lanes
 * included), out[1] the route the frame took, out[2] its clipped triangles,
 * out[3] its spans (the dense route does not count them: 0), out[4] its row
 * records.  All 0 before the first frame. */
int cg_rast_scratch_info(cg_ctx *ctx, uint64_t out[5]);
/* Host-only: the block sizes of the compact route's row-list passes -- the
 * spans a wave ranks per round (*batch) and the consecutive spans a wave owns
 * (*chunk); record order must hold across both boundaries. */
int cg_rast_row_blocks(int *batch, int *chunk);
/* Host-only, no device work: n random triangles from PCG32 (seed, stream 54)
 * as cg_rt_random_scene draws them: centroid ~ U[-1,1]^3, each vertex =
 * centroid + U[-extent,extent]^3 with w = 1, colour ~ U[0.15,0.75]^3, texture 0,
 * index 0, normal by ComputeNormal (rasteriser TestModelH.h:32-41).  Returns n. */
int cg_rast_random_scene(uint64_t seed, int n, float extent, cg_rtri *out);
/* n_frames whole Draws (colour mode 0, one size; each frame its own params --
 * camera, light, R, first-frame indirect) into frame f at d_argb + f *
 * frame_stride pixels (0: W*H), likewise d_depth / d_shadow (may be NULL).
 * The frames overlap on internal streams (the reference's main loop draws
 * them one after another; frames are independent given their params);
 * `stream` waits for all of them.  Colour modes 1-2 chain the rand() offset
 * from frame to frame: use cg_rast_draw_device per frame for those. */
int cg_rast_draw_frames_device(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, uint32_t *d_argb,
                               float *d_depth, int32_t *d_shadow, size_t frame_stride, void *stream);

/* One record per frame of a sequence, plus one closing record. */
typedef struct { uint64_t rand_offset; int64_t n_shaded; int32_t status; int32_t pad; } cg_rast_seq_frame; /* 24 B */

/* n_frames successive whole Draws as the main loop makes them (skeleton.cpp:203-308),
 * any mix of colour modes 0/1/2, one size.  The rand() call index starts at
 * ps[0].rand_offset; ps[f > 0].rand_offset is ignored.  A mode 1-2 frame starts at
 * the chained index and advances it by 3 * its shaded fragments; a mode 0 frame
 * leaves it alone.  Planes as cg_rast_draw_frames_device.  d_info (device,
 * n_frames + 1 records, required): record f = the index frame f started at, its
 * shaded fragments (-1 in mode 0) and its status; record n_frames = the index
 * after the last frame, n_shaded -1, status 0.  Enqueued on `stream`: the frames
 * start after the work already on it and it waits for all of them; between
 * those points they overlap on internal streams, only the index passing from
 * each frame to the next in order.  Nothing is read back, so after the first
 * call of a size and capacity (which allocates and uploads the generator's
 * tables) the call never waits.
 * A mode 1-2 frame that shades more fragments than the rand() stream's capacity
 * gets status CG_E_CAPACITY and its planes are left as they were; its record
 * and every later frame stay exact (render it alone with cg_rast_draw at
 * d_info[f].rand_offset).  One sequence per context at a time.
 * On the compact route the frames run in turn on `stream` and the call waits for
 * each frame's counts; a mode 1-2 frame sizes its stream from its own shaded
 * fragments, so it never reports CG_E_CAPACITY and cg_rast_set_rand_capacity
 * is ignored there.  The records are the same. */
int cg_rast_draw_sequence_device(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, uint32_t *d_argb,
                                 float *d_depth, int32_t *d_shadow, size_t frame_stride,
                                 cg_rast_seq_frame *d_info, void *stream);
/* Host-memory form: the frames of cg_rast_draw_sequence_device (the same chain: it starts at
 * ps[0].rand_offset, ps[f > 0].rand_offset is ignored, each frame takes ps[f].indirect_first as
 * given) into caller-owned host memory, pageable or pinned: frame f at argb + f * frame_stride
 * pixels (0: W * H; below W * H CG_E_INVALID), likewise depth / shadow (may be NULL); pixels
 * between frames are not written.  Every plane equals what cg_rast_draw leaves for the same
 * params at the chained index.  info (host, optional): n_frames + 1 records as d_info.
 * The frames render `chunk` at a time (0: 8, at most 64) through the device sequence into two
 * sets of context-owned device slots; chunk j downloads on the context's transfer stream while
 * chunk j + 1 renders, like cg_rt_render_frames.  The records are one device array for the whole
 * call and a chunk's first frame reads its start index from the record the previous chunk closed:
 * the index is never read back between chunks.  A frame flagged CG_E_CAPACITY is then rendered
 * alone with cg_rast_draw at its recorded index, straight into its host slot, and reports status
 * 0; a status that is non-zero on return means that frame is not in host memory, and the call
 * returns that code.  Both routes as the device form (compact-route frames in turn, all three
 * colour modes).  stats (optional): kernel_ms the device time spanning the renders, total_ms the
 * call, n_tris the last frame's clipped count, n_shaded the sum over the mode 1-2 frames (-1: none).
 * Returns when every frame, and info, is in host memory; the only host waits are those of the
 * downloads and the closing synchronise.  Slots and records grow only: after the first call of a
 * size the call allocates nothing.  cg_rast_scratch_info afterwards reports the last frame.
 * CG_E_NOSCENE before cg_rast_set_scene; CG_E_INVALID for NULL ps / argb with n_frames > 0,
 * frames of several sizes, a colour mode outside 0-2, chunk < 0 or > 64, a bad stride;
 * n_frames == 0 returns CG_OK and touches nothing. */
int cg_rast_draw_sequence(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, uint32_t *argb, float *depth,
                          int32_t *shadow, size_t frame_stride, int chunk, cg_rast_seq_frame *info, cg_stats *stats);

/* ---- The float picture (CG_PIX_RGBA_F32) and exposed frames ----
 * The picture before PutPixelSDL clamps it: W * H pixels of four floats, 16-byte aligned.
 * Interior pixel (1 <= x < W - 1, 1 <= y < H - 1): x, y, z the vec3 that antiAliasing(y, x)
 * returns (skeleton.cpp:305, :1736-1753), evaluated in raster order as the reference does, w =
 * 1.0f.  Border pixel: +0 four times -- the reference never calls PutPixelSDL there, and w = 0
 * makes it "uncovered" for cg_hdr_histogram_device.  PutPixelSDL of the interior pixels is
 * cg_rast_draw_device's frame.  It cannot be rebuilt from cg_rast_draw_buffers' planes: those
 * hold every pixel's darkening, the picture's lower and right taps are from before theirs.
 *
 * One Draw; d_rgba is W * H float4.  Route, colour mode, rand_offset, indirect_first, textures
 * and the waits per route are as cg_rast_draw_device; d_depth / d_shadow (may be NULL) too. */
int cg_rast_draw_picture_device(cg_ctx *ctx, const cg_rast_params *p, float *d_rgba, float *d_depth,
                                int32_t *d_shadow, void *stream);
/* Host-memory form, synchronous: rgba is W * H * 4 floats. */
int cg_rast_draw_picture(cg_ctx *ctx, const cg_rast_params *p, float *rgba, cg_stats *stats);
/* cg_rast_draw_sequence_device with float frames: frame f at d_rgba + f * frame_stride pixels
 * of 16 bytes (0 = W * H).  Same rand() chain, same d_info records, same lanes.  The one
 * difference: a frame whose status is non-zero (CG_E_CAPACITY, dense route) gets all-zero pixels
 * with w = 0 -- the plane is defined, not left as it was (its depth and shadow planes are left). */
int cg_rast_draw_sequence_picture_device(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, float *d_rgba,
                                         float *d_depth, int32_t *d_shadow, size_t frame_stride,
                                         cg_rast_seq_frame *d_info, void *stream);
/* The rasteriser's pack: cg_rt_tonemap_pack_device (arguments, strides, errors) with two rules
 * of its own.  Border rule: a pixel with !(w > 0.0f) packs to 0u (the raytracer's pack would
 * write 0x80000000 there).  Clamp rule: each channel is c0 = c > 0.0f ? c : 0.0f before v = c0 *
 * scale, so a NaN or a negative channel is black as PutPixelSDL shows it, whatever the scale and
 * curve (Reinhard's v / (1 + v) has a pole at -1).  LINEAR with a scale of exactly 1.0f gives
 * cg_rast_draw_device's frame bit for bit, border included.  Histogram and exposure of float
 * pictures are cg_hdr_histogram_device (channels = 4: the border is uncovered, n_uncovered =
 * 2 W + 2 H - 4; a pixel whose luminance is not positive is dark) and cg_hdr_exposure_device. */
int cg_rast_tonemap_pack_device(cg_ctx *ctx, const float *d_rgba, size_t n_pixels, int n_frames, size_t src_stride,
                                const float *d_scales, int op, float white2, uint32_t *d_argb, size_t dst_stride,
                                void *stream);
/* Host-only restatement of one pixel of it (no device, no context); NULL rgba gives 0. */
uint32_t cg_rast_pack_pixel(const float rgba[4], float scale, int op, float white2);
/* A key script rendered, exposed and packed without a host wait, as cg_rt_render_exposed_device:
 * the frames of cg_rast_draw_sequence_picture_device in chunks of 8 into scratch the context
 * owns (grow-only, 8 * W * H * 16 bytes), then histogram, exposure and the pack above per chunk.
 * Frame f as ARGB8888 at d_argb + f * frame_stride pixels (0: W * H), its scale in d_scales[f]
 * (device, n_frames floats, required), its record in d_info (device, n_frames + 1 records,
 * required); the rand() index passes from chunk to chunk through d_info and is never read back.
 * Frame 0 of the call takes d_prev (device, may be NULL) as its previous scale, frame 0 of a
 * later chunk d_scales[f - 1], as cg_rt_render_exposed_device defines it.  A frame flagged
 * CG_E_CAPACITY is the all-uncovered picture: an empty histogram, t_f = 1.0f clamped, ARGB 0; the
 * call still returns CG_OK.  On the dense route, after the first call of a size it neither
 * allocates nor waits for the device; on the compact route it waits where
 * cg_rast_draw_sequence_device waits.  CG_E_NOSCENE before cg_rast_set_scene; CG_E_INVALID as
 * cg_rast_draw_sequence_device and the cg_hdr_* calls; n_frames == 0 touches nothing. */
int cg_rast_draw_exposed_device(cg_ctx *ctx, const cg_rast_params *ps, int n_frames,
                                const cg_hdr_exposure_params *params, const float *d_prev, int op, float white2,
                                uint32_t *d_argb, size_t frame_stride, float *d_scales,
                                cg_rast_seq_frame *d_info, void *stream);
/* Host-memory form, synchronous: the same frames, scales[n_frames] and (optional) info[n_frames +
 * 1] in host memory, prev a host float or NULL; each chunk's download follows its render.
 * Returns CG_E_CAPACITY, after delivering everything, if a frame was flagged. */
int cg_rast_draw_exposed(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, const cg_hdr_exposure_params *params,
                         const float *prev, int op, float white2, uint32_t *argb, size_t frame_stride,
                         float *scales, cg_rast_seq_frame *info, cg_stats *stats);
/* cg_rast_draw_exposed_device / cg_rast_draw_exposed with bloom (the Bloom section above, rule
 * RAST): both routes, every colour mode, the rand() index passing from chunk to chunk; a frame
 * flagged CG_E_CAPACITY is the all-uncovered picture, ARGB 0.  bloom == NULL runs the call without
 * bloom unchanged. */
int cg_rast_draw_exposed_bloom_device(cg_ctx *ctx, const cg_rast_params *ps, int n_frames,
                                      const cg_hdr_exposure_params *params, const float *d_prev, int op, float white2,
                                      const cg_hdr_bloom_params *bloom, uint32_t *d_argb, size_t frame_stride,
                                      float *d_scales, cg_rast_seq_frame *d_info, void *stream);
int cg_rast_draw_exposed_bloom(cg_ctx *ctx, const cg_rast_params *ps, int n_frames,
                               const cg_hdr_exposure_params *params, const float *prev, int op, float white2,
                               const cg_hdr_bloom_params *bloom, uint32_t *argb, size_t frame_stride, float *scales,
                               cg_rast_seq_frame *info, cg_stats *stats);
/* Test hook: capacity of the materialised rand() stream in fragments (3 values each);
 * 0 = automatic, 4 * W * H. */
int cg_rast_set_rand_capacity(cg_ctx *ctx, long long fragments);
/* Probe: n values of glibc rand() starting at the 64-bit call index held in device
 * memory, produced by the device seek + generator the sequence uses. */
int cg_glibc_rand_device(cg_ctx *ctx, const uint64_t *d_offset, int n, int32_t *d_out, void *stream);

/* Texture modes 1-3 (skeleton.cpp:588-645; a triangle's `texture` field,
 * TestModelH.h:21: 1 marble, 2 metal grill, 3 woven wood -- set it on the
 * room/boxes lists, as `setting` / `settingBoxes` do, TestModelH.h:9-10).
 * The maps as cv::imread(..., CV_LOAD_IMAGE_UNCHANGED) returns them
 * (:135-146): row-major BGR, 3 bytes per texel; marble 2000 x 2000, the rest
 * 1024 x 1024.  NULL = not loaded; a texture is renderable when all its maps
 * are (marble: marble; grill: grill, grill_opacity, grill_normal; woven: all
 * four woven maps), and rendering a triangle with a texture that is not
 * fails with CG_E_INVALID (the reference reads an empty cv::Mat). */
typedef struct {
    const uint8_t *marble;                                   /* Marble2000x2000.jpg */
    const uint8_t *woven;                                    /* woven1024x1024.jpg */
    const uint8_t *woven_ao;                                 /* Wood_wicker_003_ambientOcclusion.jpg */
    const uint8_t *woven_opacity;                            /* Wood_wicker_003_opacity.jpg */
    const uint8_t *woven_normal;                             /* Wood_wicker_003_normal.jpg */
    const uint8_t *grill;                                    /* Metal_Grill_002_basecolor.jpg */
    const uint8_t *grill_opacity;                            /* Metal_Grill_002_opacity.jpg */
    const uint8_t *grill_normal;                             /* Metal_Grill_002_normal.jpg */
} cg_rast_textures;
/* Upload the maps and build what main() derives from them at start-up
 * (:148-170): the opacity maps (cg_rast_opacity_map) and, with marble, the
 * normal-noise map from the process's first 3 * 2000 * 2000 rand() calls --
 * colour modes 1-2 then start at rand_offset 12,000,000.  NULL unloads. */
int cg_rast_set_textures(cg_ctx *ctx, const cg_rast_textures *tex);
/* Host-only: OpenCV 3.4 cvtColor(CV_BGR2GRAY) on 8-bit BGR (fixed point,
 * 14-bit coefficients) then threshold(100, 255, THRESH_BINARY) (:149-155):
 * n texels in, n bytes (0 or 255) out. */
int cg_rast_opacity_map(const uint8_t *bgr, int n, uint8_t *out);

/* ---- texture loading (rasteriser/Source/skeleton.cpp:135-146) ----------- */
/* The reference loads its maps with cv::imread(path, CV_LOAD_IMAGE_UNCHANGED)
 * (OpenCV 3.4 over IJG libjpeg 9).  These decode a JPEG file's bytes to what
 * that call returns: row-major BGR (3 bytes per pixel; gray for 1-component
 * files), bit-identical to libjpeg 9's islow IDCT with 16x16 scaled chroma.
 * Baseline and progressive Huffman JPEG, 8-bit, 1 or 3 components, 4:4:4 or
 * 4:2:0; anything else is CG_E_INVALID.  Entropy decoding runs on the host,
 * the IDCT and colour conversion on the context's GPU. */
int cg_image_jpeg_info(const uint8_t *data, size_t n, int *width, int *height, int *channels);
/* Host-only: entropy-decode the whole file without a device (0, or CG_E_INVALID
 * for a corrupt or unsupported stream). */
int cg_image_jpeg_check(const uint8_t *data, size_t n);
/* out: caller-owned host buffer of >= width * height * channels bytes (cap). */
int cg_image_decode_jpeg(cg_ctx *ctx, const uint8_t *data, size_t n, uint8_t *out, size_t cap);
/* Same into device memory, enqueued on `stream` (NULL: the context's). */
int cg_image_decode_jpeg_device(cg_ctx *ctx, const uint8_t *data, size_t n, uint8_t *d_out, size_t cap,
                                void *stream);

/* ---- JPEG encoding ------------------------------------------------------ */
/* A baseline JPEG encoder for ARGB8888 frames.  The contract is bit-exact: the file is, byte for
 * byte, what Pillow over libjpeg-turbo writes with
 *     Image.fromarray(rgb).save(f, format="JPEG", quality=Q, subsampling=S, restart_marker_rows=1)
 * and no other option, where rgb[y][x] = (bits 16-23, bits 8-15, bits 0-7) of pixel (x, y); the
 * alpha byte is ignored.  Q is 1 .. 100, S is CG_JPEG_444 or CG_JPEG_420.  All arithmetic is int32,
 * `>>` arithmetic, each operation in the order stated; the host function and the kernels share it
 * (csrc/cg_jpeg_enc.h).
 *
 * 1 Colour    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *             Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 * 2 Planes    The MCU is 8 x 8 pixels at 4:4:4 and 16 x 16 at 4:2:0; MX = ceil(W / mcu), MY =
 *             ceil(H / mcu).  A full-resolution plane is padded by replicating its last column and
 *             last row.  At 4:2:0 a chroma sample is c[y][x] = (p[2y][2x] + p[2y][2x+1] + p[2y+1][2x]
 *             + p[2y+1][2x+1] + bias) >> 2, bias 1 for even x and 2 for odd, over the plane padded to
 *             16 MX columns and an even number of rows; rows of c beyond ceil(H / 2) repeat the last.
 * 3 Dummies   At 4:2:0 a Y block at or beyond block column ceil(W / 8) or block row ceil(H / 8) is
 *             not transformed: its AC coefficients are 0 and its DC is the quantised DC of the
 *             previous block of its MCU, in the order 00, 01, 10, 11 (the first is always real).
 * 4 FDCT      libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2) on sample - 128, rows then columns;
 *             DESCALE(x, n) = (x + (1 << (n - 1))) >> n; n = 11 for rows, 15 for columns.
 *             t0 = d0+d7, t7 = d0-d7, t1 = d1+d6, t6 = d1-d6, t2 = d2+d5, t5 = d2-d5, t3 = d3+d4,
 *             t4 = d3-d4; t10 = t0+t3, t13 = t0-t3, t11 = t1+t2, t12 = t1-t2.
 *             rows: o0 = (t10+t11) << 2, o4 = (t10-t11) << 2; columns: o0 = DESCALE(t10+t11, 2),
 *             o4 = DESCALE(t10-t11, 2).  z1 = (t12+t13) * 4433; o2 = DESCALE(z1 + t13 * 6270, n);
 *             o6 = DESCALE(z1 - t12 * 15137, n).  z1 = t4+t7, z2 = t5+t6, z3 = t4+t6, z4 = t5+t7,
 *             z5 = (z3+z4) * 9633; t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299; z1 *= -7373,
 *             z2 *= -20995, z3 *= -16069, z4 *= -3196; z3 += z5, z4 += z5;
 *             o7 = DESCALE(t4+z1+z3, n), o5 = DESCALE(t5+z2+z4, n), o3 = DESCALE(t6+z2+z3, n),
 *             o1 = DESCALE(t7+z1+z4, n).
 * 5 Quantise  scale = Q < 50 ? 5000 / Q : 200 - 2 Q; q = clamp((base * scale + 50) / 100, 1, 255)
 *             over the Annex K.1 tables (luminance for Y, chrominance for Cb and Cr); the coefficient
 *             is sign(c) * ((|c| + (8 q >> 1)) / (8 q)), integer division (the FDCT carries a factor 8).
 * 6 Entropy   The four Annex K.3 Huffman tables, Y with tables 0, Cb and Cr with tables 1.  DC: the
 *             category of the difference to the previous block of the component, then its low bits,
 *             a negative v sent as v - 1.  AC in zig-zag order: run/size symbols, 0xF0 for each 16
 *             zeros before a coefficient, 0x00 if the block ends in zeros.  Bits fill bytes from the
 *             top; a 00 follows every FF byte.  MCUs run left to right, top to bottom, their blocks
 *             Y (00 01 10 11 at 4:2:0), Cb, Cr.  The restart interval is MX: before every MCU row k
 *             >= 1 the last byte is padded with 1-bits, FF D0+((k-1) mod 8) is written and the three
 *             predictors return to 0.  After the last row: pad, FF D9.
 * 7 Header    629 bytes: SOI; APP0 (JFIF 1.1, no units, 1:1, no thumbnail); DQT 0; DQT 1 (separate
 *             segments, zig-zag order); SOF0 (precision 8, H, W, components 1 22|11 0, 2 11 1,
 *             3 11 1); DHT DC0, AC0, DC1, AC1; DRI MX; SOS (1 00, 2 11, 3 11, 00 3F 00). */
#define CG_JPEG_444 0
#define CG_JPEG_420 2
typedef struct { int quality; int subsampling; } cg_jpeg_params;
/* Host-only (no device, no context).  cg_image_encode_jpeg_host: the file of width x height
 * pixels, rows row_stride_pixels apart (0: width), into out[0 .. cap) and its length into *n;
 * CG_E_CAPACITY with *n = the length needed when cap is short (no byte at or past cap is written;
 * out may be NULL with cap 0).  cg_image_jpeg_header: the bytes before the scan, the same for
 * every frame of a size and params; returns their count (629) or CG_E_CAPACITY.
 * cg_image_jpeg_bound: a length no file of the size can exceed -- every block at its longest code
 * (22 bits of DC, 63 coefficients of 16 + 10 bits) and every byte of the scan stuffed.
 * cg_image_jpeg_enc_limits: the entropy kernel's workgroup size and the bytes of an interval it
 * holds in LDS at a time (tests size their cases from these).  CG_E_INVALID for a width or height
 * outside 1 .. 65535, a quality outside 1 .. 100, another subsampling, NULL pointers. */
int cg_image_encode_jpeg_host(const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                              const cg_jpeg_params *params, uint8_t *out, size_t cap, size_t *n);
int cg_image_jpeg_header(int width, int height, const cg_jpeg_params *params, uint8_t *out, size_t cap);
long long cg_image_jpeg_bound(int width, int height, int subsampling);
int cg_image_jpeg_enc_limits(int *threads, int *stage_bytes);
/* n_frames frames in device memory, enqueued on `stream` (NULL: the context's) without a host
 * wait.  Frame f is read at d_argb + f * frame_stride pixels (0: width * height; rows are width
 * apart); its file goes to d_out + f * slot_bytes and its length to d_bytes[f] (8-byte aligned), or
 * CG_E_CAPACITY there when the file is longer than slot_bytes: then nothing is written to that
 * slot, and the other frames are unaffected.  Nothing is written past a file's last byte.  The
 * coefficients and staged intervals of up to 8 frames live in grow-only scratch the context owns,
 * one set per context: calls on one context must be ordered among themselves, by one stream or by
 * events; calls on different contexts are independent.  After the first call of a size it does not
 * allocate.  n_frames == 0 returns CG_OK and touches nothing. */
int cg_image_encode_jpeg_device(cg_ctx *ctx, const uint32_t *d_argb, int width, int height, int n_frames,
                                size_t frame_stride, const cg_jpeg_params *params, uint8_t *d_out, size_t slot_bytes,
                                int64_t *d_bytes, void *stream);
/* One frame in host memory through the device encoder, arguments as cg_image_encode_jpeg_host;
 * waits for the file. */
int cg_image_encode_jpeg(cg_ctx *ctx, const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                         const cg_jpeg_params *params, uint8_t *out, size_t cap, size_t *n);
/* Frame sequences delivered into host memory compressed: cg_rt_render_sequence's and
 * cg_rast_draw_sequence's frames (arguments as there; ARGB only), rendered in chunks of `chunk`
 * frames (0: 8, at most 64) into the chunk slots of those calls and encoded on the device into
 * slots of width * height bytes.  A chunk's lengths are read back and exactly its files' bytes are
 * copied into `out` back to back while the next chunk renders; a file longer than its slot is
 * encoded again alone into a slot of cg_image_jpeg_bound.  offsets has n_frames + 1 entries:
 * offsets[f] .. offsets[f + 1] is frame f's file.  If `out` (cap bytes) is short the call returns
 * CG_E_CAPACITY: the files that fit whole before the first that does not are intact, nothing is
 * written past cap, and offsets[n_frames] is the capacity a second call needs.  The rasteriser's
 * rand() index chain and `info` records equal cg_rast_draw_sequence's.  CG_E_INVALID as the calls
 * they mirror and the encoder (a side above 65535, invalid params, NULL offsets). */
int cg_rt_render_sequence_jpeg(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                               const cg_jpeg_params *params, uint8_t *out, size_t cap, size_t *offsets, int chunk,
                               cg_stats *stats);
int cg_rast_draw_sequence_jpeg(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, const cg_jpeg_params *params,
                               uint8_t *out, size_t cap, size_t *offsets, int chunk, cg_rast_seq_frame *info,
                               cg_stats *stats);

/* ---- PNG encoding ------------------------------------------------------- */
/* A lossless PNG encoder for ARGB8888 frames: 8-bit samples, no interlace, the chunks IHDR, IDAT
 * (one per band) and IEND and no other.  Any PNG decoder returns the input pixels.  The bytes are
 * this library's own -- an LZ77 parse over the whole image, as zlib makes it, is one serial pass
 * -- and are fixed by the rules below, all integer arithmetic; the host function and the kernels
 * share them (csrc/cg_png_enc.h) and produce the same file.
 *
 * 1 Samples   colour CG_PNG_RGB (colour type 2): a pixel's bytes are bits 16-23, 8-15, 0-7 (R, G,
 *             B), bits 24-31 are ignored; CG_PNG_RGBA (colour type 6): bits 24-31 follow as A.  bpp
 *             = 3 or 4.
 * 2 Filters   Per row, PNG's types 0 None, 1 Sub, 2 Up, 3 Average ((a + b) >> 1), 4 Paeth, with a
 *             the byte bpp to the left, b the byte above, c the byte above a; bytes outside the
 *             image are 0.  Paeth: p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|; a if
 *             pa <= pb and pa <= pc, else b if pb <= pc, else c.  filter 0 .. 4 uses that type for
 *             every row; CG_PNG_FILTER_ADAPTIVE gives a row the type whose filtered bytes, read as
 *             int8, have the smallest sum of absolute values (-128 counts 128), the lowest type on
 *             a tie.  A filtered row is its type byte and W * bpp bytes.
 * 3 Bands     Rows 16 k .. 16 k + 15 (fewer in the last) are band k.  A band's filtered rows, back
 *             to back, are compressed alone and are one IDAT chunk.
 * 4 Tokens    Within a band, a maximal run of n equal bytes (runs cross rows) with n < 4 is n
 *             literals.  With n >= 4 it is one literal, then matches of length 258 and distance 1
 *             while at least 258 bytes of the run remain, then one match of the remainder r if r
 *             >= 3, else r literals.
 * 5 Lengths   A code's lengths come from frequencies f and a limit L: the symbols with f > 0
 *             sorted by (f, symbol); a Huffman merge over two queues -- the sorted leaves and the
 *             internal nodes in the order made -- that takes the leaf when a leaf and a node weigh
 *             the same; count[d] = the leaves at depth d, depths above L counted at L; while the
 *             Kraft sum (count[d] * 2^(L - d) over d) exceeds 2^L: with d the largest depth below
 *             L that has a leaf, count[d] -= 1, count[d + 1] += 2, count[L] -= 1 (the sum falls by
 *             one); then the sorted symbols take their lengths in order, count[L] of them L, the
 *             next count[L - 1] of them L - 1, and so on.  Two or more symbols give a complete
 *             code; one symbol gets length 1.  Codes are canonical (RFC 1951 3.2.2).
 * 6 Block     One dynamic block per band.  Literal/length code: f from the band's tokens plus one
 *             end-of-block, L = 15; HLIT covers the highest used symbol (at least 257).  Distance
 *             code: HDIST = 2, both lengths 1, so distance 1 is the single bit 0.  The HLIT lengths
 *             and the two distance lengths are one sequence, coded from the left: a run of r zeros
 *             sends symbol 18 (min(r, 138)) while r >= 11, then 17 (r) if r >= 3, else r zeros; a
 *             run of r lengths v > 0 sends v, then 16 (min(rest, 6)) while the rest is >= 3, then
 *             the rest as v.  Code-length code: f from that sequence, L = 7; HCLEN ends at the last
 *             length other than 0 in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (at
 *             least 4).
 * 7 Stored    If the dynamic block's bits (3 + 14 + 3 HCLEN + the coded lengths + the tokens + the
 *             end-of-block) are not fewer than 8 n + 40 ceil(n / 65535) for the band's n bytes, the
 *             band is stored blocks of 65535 bytes, the last shorter.
 * 8 Stream    The first chunk's data begins 78 01.  A band that is not the last is followed by an
 *             empty stored block (000, zero bits to the byte, 00 00 FF FF), so every chunk is whole
 *             bytes; the last band's last block has BFINAL set, is padded with zero bits and is
 *             followed by the Adler-32 of all filtered bytes, most significant byte first. */
#define CG_PNG_RGB 2
#define CG_PNG_RGBA 6
#define CG_PNG_FILTER_ADAPTIVE (-1)
typedef struct { int colour; int filter; } cg_png_params;
/* Host-only (no device, no context).  cg_image_encode_png_host: as cg_image_encode_jpeg_host --
 * the file into out[0 .. cap), its length into *n, CG_E_CAPACITY with *n = the length needed when
 * cap is short (no byte at or past cap is written; out may be NULL with cap 0).
 * cg_image_png_bound: a length no file of the size can exceed: 8 + 25 + 12 bytes of signature,
 * IHDR and IEND, 2 + 4 of zlib header and Adler-32, and per band of n bytes 12 of chunk, n + 5
 * ceil(n / 65535) stored, 5 of empty block after all but the last; a frame whose bands are all
 * stored is exactly that long.  cg_image_png_code_lengths: rule 5 alone, lengths[0 .. n) from
 * freq[0 .. n), n <= 286, limit 1 .. 15, at most 2^limit used symbols, frequencies summing below
 * 2^32.  cg_image_png_enc_limits: the lanes of a band workgroup (the bytes of a band it takes at a
 * time) and the bytes of a band's bit string it holds in LDS.  CG_E_INVALID for a width or height
 * outside 1 .. 65535, another colour or filter, NULL pointers. */
int cg_image_encode_png_host(const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                             const cg_png_params *params, uint8_t *out, size_t cap, size_t *n);
long long cg_image_png_bound(int width, int height, int colour);
int cg_image_png_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *lengths);
int cg_image_png_enc_limits(int *threads, int *window_bytes);
/* n_frames frames in device memory, with cg_image_encode_jpeg_device's conventions: enqueued on
 * `stream` (NULL: the context's) without a host wait; frame f is read at d_argb + f * frame_stride
 * pixels (0: width * height), its file goes to d_out + f * slot_bytes and its length to d_bytes[f]
 * (8-byte aligned), or CG_E_CAPACITY there when the file is longer than slot_bytes: then nothing
 * is written to that slot, and the other frames are unaffected.  Nothing is written past a file's
 * last byte.  The filtered rows and staged bands of up to 8 frames live in grow-only scratch the
 * context owns, one set per context: calls on one context must be ordered among themselves; calls
 * on different contexts are independent.  After the first call of a size it does not allocate.
 * n_frames == 0 returns CG_OK and touches nothing. */
int cg_image_encode_png_device(cg_ctx *ctx, const uint32_t *d_argb, int width, int height, int n_frames,
                               size_t frame_stride, const cg_png_params *params, uint8_t *d_out, size_t slot_bytes,
                               int64_t *d_bytes, void *stream);
/* One frame in host memory through the device encoder, arguments as cg_image_encode_png_host;
 * waits for the file. */
int cg_image_encode_png(cg_ctx *ctx, const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                        const cg_png_params *params, uint8_t *out, size_t cap, size_t *n);
/* Frame sequences delivered into host memory exact: cg_rt_render_sequence_jpeg's and
 * cg_rast_draw_sequence_jpeg's arguments and behaviour with PNG files -- chunks of `chunk` frames
 * (0: 8, at most 64) are encoded on the device behind their render into slots of
 * cg_image_png_bound, so no file is encoded twice, and exactly a chunk's file bytes are copied
 * into `out` back to back while the next chunk renders.  offsets[f] .. offsets[f + 1] is frame
 * f's file, which decodes to the frame cg_rt_render_sequence / cg_rast_draw_sequence delivers (all
 * 32 bits of it with CG_PNG_RGBA).  If `out` (cap bytes) is short the call returns CG_E_CAPACITY:
 * the files that fit whole before the first that does not are intact, nothing is written past
 * cap, and offsets[n_frames] is the capacity a second call needs.  The rasteriser's rand() index
 * chain and `info` records equal cg_rast_draw_sequence's. */
int cg_rt_render_sequence_png(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                              const cg_png_params *params, uint8_t *out, size_t cap, size_t *offsets, int chunk,
                              cg_stats *stats);
int cg_rast_draw_sequence_png(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, const cg_png_params *params,
                              uint8_t *out, size_t cap, size_t *offsets, int chunk, cg_rast_seq_frame *info,
                              cg_stats *stats);

/* ---- EXR encoding ------------------------------------------------------- */
/* An OpenEXR encoder for CG_PIX_RGBA_F32 pictures: a single-part scanline OpenEXR 2 file that any
 * EXR reader accepts.  As with the PNG encoder the bytes are this library's own and are fixed by
 * the rules below, all integer arithmetic except the one float32 product of rule 1; the host
 * function and the kernels share them (csrc/cg_exr_enc.h) and produce the same file.
 *
 * 1 Samples   Source pixel (x, y, z, w) gives R = x, G = y, B = z, and A = w when alpha_scale's
 *             bits are 0x3F800000, else the single float32 product w * alpha_scale (the raytracer's
 *             w counts 0 .. 9 samples; its app passes 1.0f / 9.0f).  CG_EXR_FLOAT stores the 32
 *             bits unchanged.  CG_EXR_HALF rounds to nearest even: with a = the bits without the
 *             sign, a > 0x7F800000 (NaN) gives 0x7C00 | (mantissa >> 13), bit 0 set when that
 *             leaves the mantissa 0; a >= 0x47800000 gives inf; a >= 0x38800000 gives (a -
 *             0x38000000) >> 13, one more when the 13 bits dropped exceed 0x1000 or equal it with
 *             the result odd (a carry into the exponent is right, up to inf); a < 0x33000000 gives
 *             0; otherwise (0x800000 | mantissa) >> (126 - exponent) rounded the same way on the
 *             bits dropped.  The sign is kept throughout.  numpy's astype(float16) gives the same
 *             bits.  Samples are little endian.
 * 2 Header    76 2F 31 01, 02 00 00 00, then the attributes channels (chlist), compression
 *             (compression: one byte 0 or 3), dataWindow (box2i 0, 0, W - 1, H - 1), displayWindow
 *             (the same), lineOrder (lineOrder: byte 0), pixelAspectRatio (float 1.0),
 *             screenWindowCenter (v2f 0, 0), screenWindowWidth (float 1.0) in that order, each as
 *             name\0, type\0, int32 size, value; then one 0 byte.  A chlist entry is name\0, int32
 *             pixel type (1 half, 2 float), a byte 0, three bytes 0, int32 1, int32 1; the list
 *             ends with a 0 byte.  Channels are in name order, A B G R or B G R.  331 bytes for
 *             RGBA, 313 for RGB.  A 2 x 1 RGB half ZIP file's header:
 *               762f3101 02000000 6368616e6e656c7300 63686c69737400 37000000
 *               4200 01000000 00000000 01000000 01000000  4700 01000000 00000000 01000000 01000000
 *               5200 01000000 00000000 01000000 01000000  00
 *               636f6d7072657373696f6e00 636f6d7072657373696f6e00 01000000 03
 *               6461746157696e646f7700 626f78326900 10000000 00000000 00000000 01000000 00000000
 *               646973706c617957696e646f7700 626f78326900 10000000 00000000 00000000 01000000 00000000
 *               6c696e654f7264657200 6c696e654f7264657200 01000000 00
 *               706978656c417370656374526174696f00 666c6f617400 04000000 0000803f
 *               73637265656e57696e646f7743656e74657200 76326600 08000000 00000000 00000000
 *               73637265656e57696e646f77576964746800 666c6f617400 04000000 0000803f  00
 * 3 Chunks    CG_EXR_NONE: one scanline a chunk.  CG_EXR_ZIP: scanlines 16 k .. 16 k + 15, fewer
 *             in the last.  After the header one uint64 per chunk, its offset from the start of
 *             the file; then the chunks in order, each int32 first y, int32 data length, data.
 * 4 Pixels    A chunk's n raw bytes are, per scanline, each channel's W samples back to back in
 *             channel order.  n is even.
 * 5 ZIP       t = the raw bytes at even positions, then those at odd positions.  d[0] = t[0], d[i]
 *             = (t[i] - t[i - 1] + 128) mod 256.  The zlib stream of d is what the PNG rules 4 - 8
 *             give a file of this one band: 78 01, the band's block(s) with BFINAL on the last,
 *             zero bits to the byte, the Adler-32 of d.  If the stream has fewer than n bytes it
 *             is the chunk's data; otherwise the data is the n raw bytes (OpenEXR's own fallback:
 *             its readers take a chunk of exactly n bytes as uncompressed). */
#define CG_EXR_RGB 3
#define CG_EXR_RGBA 4
#define CG_EXR_HALF 1
#define CG_EXR_FLOAT 2
#define CG_EXR_NONE 0
#define CG_EXR_ZIP 3
typedef struct { int channels; int type; int compression; float alpha_scale; } cg_exr_params;
/* Host-only (no device, no context).  A NULL params is RGBA, HALF, ZIP, alpha scale 1.
 * cg_image_encode_exr_host: as cg_image_encode_png_host -- the file of the picture rgba (4 floats
 * a pixel, rows row_stride_pixels apart, 0: width) into out[0 .. cap), its length into *n,
 * CG_E_CAPACITY with *n = the length needed when cap is short (no byte at or past cap is written;
 * out may be NULL with cap 0).  cg_image_exr_bound: header + 8 * chunks + the sum of 8 + n over
 * the chunks: a NONE file's exact length, and no ZIP file exceeds it.  cg_image_exr_header: the
 * header's bytes into out[0 .. cap), their count into *n (CG_E_CAPACITY if cap is short).
 * cg_image_exr_half: rule 1's conversion of n floats.  cg_image_exr_enc_limits: the lanes of a
 * chunk workgroup (the bytes of d it takes at a time) and the bytes of a chunk's bit string it
 * holds in LDS.  CG_E_INVALID for a width or height outside 1 .. 65535, unknown enum values, an
 * alpha_scale that is not finite, NULL pointers. */
int cg_image_encode_exr_host(const float *rgba, int width, int height, size_t row_stride_pixels,
                             const cg_exr_params *params, uint8_t *out, size_t cap, size_t *n);
long long cg_image_exr_bound(int width, int height, int channels, int type);
int cg_image_exr_header(int width, int height, const cg_exr_params *params, uint8_t *out, size_t cap, size_t *n);
int cg_image_exr_half(const float *values, int n, uint16_t *halves);
int cg_image_exr_enc_limits(int *threads, int *window_bytes);
/* n_frames pictures in device memory, with cg_image_encode_png_device's conventions in every
 * respect: enqueued on `stream` (NULL: the context's) without a host wait; frame f is read at
 * d_rgba + 4 * f * frame_stride floats (frame_stride in pixels, 0: width * height; d_rgba 16-byte
 * aligned), its file goes to d_out + f * slot_bytes and its length to d_bytes[f] (8-byte aligned),
 * or CG_E_CAPACITY there when the file is longer than slot_bytes: then nothing is written to that
 * slot, and the other frames are unaffected.  Nothing is written past a file's last byte.  The
 * predicted bytes and staged streams of up to 8 frames live in grow-only scratch the context owns,
 * one set per context: calls on one context must be ordered among themselves.  n_frames == 0
 * returns CG_OK and touches nothing. */
int cg_image_encode_exr_device(cg_ctx *ctx, const float *d_rgba, int width, int height, int n_frames,
                               size_t frame_stride, const cg_exr_params *params, uint8_t *d_out, size_t slot_bytes,
                               int64_t *d_bytes, void *stream);
/* One picture in host memory through the device encoder, arguments as cg_image_encode_exr_host;
 * waits for the file. */
int cg_image_encode_exr(cg_ctx *ctx, const float *rgba, int width, int height, size_t row_stride_pixels,
                        const cg_exr_params *params, uint8_t *out, size_t cap, size_t *n);
/* Key scripts of float pictures delivered into host memory as files: cg_rt_render_sequence_png's
 * and cg_rast_draw_sequence_png's arguments and behaviour with EXR files of the scene-linear
 * picture before the clamp.  Chunks of `chunk` frames (0: 8, at most 8 -- a float frame is 16
 * bytes a pixel; the raytracer's call clamps a larger value, the rasteriser's refuses it as it
 * refuses one above 64 for PNG) are rendered as CG_PIX_RGBA_F32 by cg_rt_render_sequence_device /
 * cg_rast_draw_sequence_picture_device's route into the scratch the exposed calls own, encoded
 * behind their render into slots of cg_image_exr_bound, and exactly a chunk's file bytes are
 * copied into `out` back to back while the next chunk renders.  offsets[f] .. offsets[f + 1] is
 * frame f's file: with CG_EXR_FLOAT its samples are those floats bit for bit, with CG_EXR_HALF
 * their halves by rule 1.  If `out` (cap bytes) is short the call returns CG_E_CAPACITY: the
 * files that fit whole before the first that does not are intact, nothing is written past cap,
 * and offsets[n_frames] is the capacity a second call needs.  The rasteriser's rand() index chain
 * and `info` records equal cg_rast_draw_sequence's. */
int cg_rt_render_sequence_exr(cg_ctx *ctx, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                              const cg_exr_params *params, uint8_t *out, size_t cap, size_t *offsets, int chunk,
                              cg_stats *stats);
int cg_rast_draw_sequence_exr(cg_ctx *ctx, const cg_rast_params *ps, int n_frames, const cg_exr_params *params,
                              uint8_t *out, size_t cap, size_t *offsets, int chunk, cg_rast_seq_frame *info,
                              cg_stats *stats);

/* ---- measurement ----------------------------------------------------- */
/* Live device time of the hot kernels: while on, a start / stop HIP event
 * pair rides on each launch's own dispatch (hipExtLaunchKernel) of
 * rt_prepare_kernel, rt_tile_cert_kernel,
 * rt_lattice_units_kernel, rt_lattice_kernel, rt_lattice_lights_kernel,
 * rt_pixel_kernel, rt_big_primary_kernel, rt_shadow_hints_kernel,
 * rast_fill_kernel and rast_post_kernel, on the stream it runs on, plus
 * "rt_big_frame" (a large scene's whole frame: events recorded around it) and, for a large scene's
 * hits-only pass (cg_rt_hits_device), "rt_hits_pass" (the whole pass), "rt_hits_walk" and
 * "rt_hits_gather", the PNG encoder's png_enc_filter_kernel, png_enc_band_kernel,
 * png_enc_scan_kernel and png_enc_gather_kernel, and the EXR encoder's exr_enc_plane_kernel,
 * exr_enc_chunk_kernel, exr_enc_scan_kernel and exr_enc_gather_kernel.  cg_kernel_timing(on)
 * resets the totals (process-wide); cg_kernel_time waits for the recorded
 * launches and returns one kernel's summed launch milliseconds, its busy
 * milliseconds (the union of its launches' spans: launches that overlap on
 * two streams count once) and its launch count. */
int cg_kernel_timing(int enable);
int cg_kernel_time(const char *kernel, double *total_ms, double *busy_ms, long long *launches);

/* ---- starfield (starfield/Source/skeleton.cpp) -------------------------- */
/* n stars as (x, y, z) float triples from glibc rand() (:41-46, seed 1). */
int cg_starfield_init(float *stars, int n);
/* Update() (:82-104) for a frame time dt in ms (the reference's float(t2 - t)). */
int cg_starfield_update(float *stars, int n, float dt);
/* Draw() (:66-79): clear, project each star, PutPixelSDL white; W*H ARGB
 * into the caller-owned host buffer. */
int cg_starfield_draw(cg_ctx *ctx, const float *stars, int n, int width, int height, uint32_t *argb);
/* Resident stars: the main loop (:53-57) on the device.  cg_starfield_set uploads n (x, y, z)
 * triples as the context's stars (n == 0: an empty field), replacing an earlier set after
 * waiting for the starfield work that still reads it.  cg_starfield_get waits for the
 * context's starfield work, copies the resident state out and returns n (CG_E_CAPACITY if
 * cap < n, CG_E_NOSCENE before the first set).  They share nothing with cg_starfield_draw,
 * which may be interleaved freely. */
int cg_starfield_set(cg_ctx *ctx, const float *stars, int n);
int cg_starfield_get(cg_ctx *ctx, float *stars, int cap);
/* n_frames frames into device memory: frame f is Draw() of the stars after f updates, at
 * d_argb + f * frame_stride pixels (0 = W * H; pixels between frames are not written), and
 * update f is Update() with frame time dts[f] (host memory, consumed before the call
 * returns).  n_updates is n_frames, or n_frames - 1 to draw the last frame without advancing
 * past it (n_frames 1, n_updates 0: a plain Draw of the resident stars).  Afterwards the
 * resident stars are the state after n_updates updates.  Enqueues on `stream` (NULL: the
 * context's) and does not synchronise; calls may be queued back to back on one stream.
 * Every pixel and every z is bit-identical to cg_starfield_draw / cg_starfield_update run
 * frame by frame.  CG_E_NOSCENE before cg_starfield_set. */
int cg_starfield_run_device(cg_ctx *ctx, const float *dts, int n_updates, int n_frames, int width, int height,
                            uint32_t *d_argb, size_t frame_stride, void *stream);
/* Update() x n_updates on the resident stars, no drawing; enqueues like the call above. */
int cg_starfield_advance_device(cg_ctx *ctx, const float *dts, int n_updates, void *stream);
/* The same frames into caller-owned host memory (pageable or pinned), rendered `chunk` frames
 * at a time (0 = 8; at most 64): chunk j + 1 renders while chunk j downloads on a second
 * stream.  Returns once every frame is in host memory. */
int cg_starfield_run(cg_ctx *ctx, const float *dts, int n_updates, int n_frames, int width, int height,
                     uint32_t *argb, size_t frame_stride, int chunk, cg_stats *stats);
/* Host-only: how a run of n_frames frames is cut.  *frames_per_launch: the most frames one
 * kernel launch covers; *frames_per_block: the consecutive frames one thread draws (either
 * may be NULL).  Returns the number of launches, or CG_E_INVALID for negative arguments. */
int cg_starfield_plan(int n_stars, int n_frames, int *frames_per_launch, int *frames_per_block);

#ifdef __cplusplus
}
#endif
#endif /* CG_RENDER_H */
