// cg_host.h -- every host function that one .hip file of the library defines and another
// calls, declared once: the definition includes this header too, so a changed parameter fails
// to compile or link instead of running wrong.  Default arguments are written here only.
// struct cg_ctx stays opaque (cg_ctx.h, for the cg_api_*.hip files and cg_ctx.hip alone):
// kernel files reach the context through the ctx_* accessors.
#pragma once

#include <string>
#include <vector>

#include "cg_internal.h"
#include "cg_own.h"

#define CG_TRY(ctx, call, what)                       \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) return ctx_fail((ctx), e_, (what)); \
    } while (0)

namespace cg {

struct SceneBounds;   // cg_rt_grid.h; the rest: cg_rast_dev.h
struct BloomLayout;   // cg_bloom.h
struct RastArgs; struct RastHdr; struct RastSeq; struct RastTexMaps; struct RastLast; struct RastFrame; struct RowRec;

// The context's starfield state, used by cg_starfield.hip.  x and y never change; z alternates
// between two buffers, because a launch's blocks replay from the state before it while its
// last block stores the state after it.
struct StarState {
    int n = -1;                  // resident stars; -1: none set
    int cap = 0;                 // stars the buffers hold
    int cur = 0;                 // z[cur] is the resident state once everything enqueued has run
    // cg_starfield_run (host output): chunks render into two device slots and download on
    // `xfer` while the next chunk renders
    Stream xfer;
    DevBuf xy, z[2];             // float2 and float per star
    Event last;                  // after the latest enqueued starfield work
    bool pending = false;        // `last` has been recorded
    Event rdone[2], cdone[2];
    DevBuf slot[2];              // uint32_t pixels
    size_t slot_px = 0;
};

// ---- the context (cg_ctx.hip) ----
// ctx_buf slots: the context's grow-only scratch buffers by name.  Three ranges: the named
// fields, the compact rasteriser route's own buffers (cg_rast_big.hip names them kBufBig0 + k)
// and the buffers calls' (cg_rast_buffers.hip).
enum {
    kBufTris = 0, kBufHdr, kBufSpan, kBufPix, kBufArgb, kBufDepth, kBufShadow, kBufCount, kBufRecs, kBufGeo,
    kBufPc, kBufTl, kBufRnd, kBufJt,     // colour modes 1-2 (cg_rast_colour.hip)
    kBufStars, kBufStarFrame,            // cg_starfield.hip
    kBufTexel, kBufImage, kBufSeq,
    kBufRastHdr,                         // cg_rast_draw_exposed*: a chunk's CG_PIX_RGBA_F32 frames
    kBufJpegEnc, kBufJpegEncIo,          // cg_jpeg_enc.hip: a chunk's coefficients and intervals; the host form's frame
    kBufFieldsEnd,
    kBufBig0 = 22, kBufBigEnd = kBufBig0 + 15,
    kBufOwner = 40, kBufClipPre, kBufScreen, kBufLow, kBufHigh, kBufClipId, kBufTriId, kBufPos, kBufPick, kBufOwnerEnd
};
void *ctx_buf(cg_ctx *c, int which, size_t bytes, hipError_t *e);
// cg_png_enc.hip's two: 0 a chunk's filtered rows and staged bands, 1 the host form's frame and file
void *ctx_png_buf(cg_ctx *c, int which, size_t bytes, hipError_t *e);
// cg_exr_enc.hip's two: 0 a chunk's predicted bytes and staged streams, 1 the host form's frame and file
void *ctx_exr_buf(cg_ctx *c, int which, size_t bytes, hipError_t *e);
// cg_exr_enc.hip: *out = *in, or the defaults for NULL; false if a field is invalid
bool exr_resolve_params(const cg_exr_params *in, cg_exr_params *out);
int ctx_device(const cg_ctx *c);
hipStream_t ctx_stream(const cg_ctx *c);
void ctx_events(cg_ctx *c, hipEvent_t *a, hipEvent_t *b);
void ctx_set_error(cg_ctx *c, const std::string &e);
int ctx_invalid(cg_ctx *c, const char *what);
int ctx_fail(cg_ctx *c, hipError_t e, const char *what);
// cg_rt_frame_columns over the context's scene (the full width without one)
void ctx_rt_columns(const cg_ctx *c, const cg_rt_camera *cam, int *c0, int *c1);
StarState *ctx_star(cg_ctx *c);
// The route a frame of list capacity `cap` takes on this context: its forced route, else its route
// limit, else cg_rast_route -- but compact for a colour mode 1-2 frame (`colour`) whose list the dense
// colour fill's LDS counters cannot hold (kRastDenseColourList).
int ctx_rast_route(cg_ctx *c, long long cap, bool colour);
// cg_rast_set_route(ctx, 1) holds: the A/B hook's compact frames are colour mode 0 only
bool ctx_rast_forced_compact(cg_ctx *c);
RastLast *ctx_rast_last(cg_ctx *c);
RastFrame *ctx_rast_frame(cg_ctx *c);
// A buffers call is running the frame (cg_rast_draw_buffers*, cg_rast_pick): colour modes 1-2
// also run the ordered z-buffer's fill for the state words, which they otherwise never make.
bool ctx_rast_want_owner(cg_ctx *c);
// the device texture maps and which textures are renderable (bit k: texture k)
int rast_tex_maps(cg_ctx *c, RastTexMaps *m);

// ---- raytracer kernels' launches and host helpers ----
// cg_rt.hip
hipError_t launch_rt_scene(const cg_tri *, int, RtGeo *, RtShade *, hipStream_t);
hipError_t launch_rt_prepare(const cg_tri *, const RtGeo *, int, const RtFrameCams &, int, RtTri *, hipStream_t,
                             const RtFrame *, const RtSphere *, unsigned long long *, unsigned long long *,
                             LatFlatten * = nullptr, LatPublish * = nullptr, unsigned long long ** = nullptr,
                             const RtFrameRec * = nullptr);
size_t rt_sup_units(const RtFrame &);
bool rt_use_lattice(const RtFrame &);
int rt_lattice_kind(const RtFrame &);
size_t rt_lattice_tiles(const RtFrame &);
size_t rt_lattice_unit_bytes(const RtFrame &, int);
hipError_t launch_rt_lattice_units(const RtFrame &, const RtTri *, const RtShade *, const RtSphere *,
                                   const unsigned long long *, const RtFrameCams &, int, unsigned long long *,
                                   hipStream_t, const RtFrameRec * = nullptr);
hipError_t launch_rt_lattice_frames(const RtFrame &, const RtTri *, const RtShade *, const RtSphere *,
                                    const unsigned long long *, const unsigned long long *, const RtFrameCams &,
                                    int, size_t, uint32_t *, hipStream_t, uint32_t *, const LatOrder *,
                                    const LatReady * = nullptr, const unsigned long long * = nullptr,
                                    const RtFrameRec * = nullptr);
hipError_t launch_rt_pixels(const RtFrame &, const RtTri *, const RtShade *, const RtSphere *,
                            const unsigned long long *, unsigned long long *, uint32_t *, hipStream_t,
                            const unsigned long long * = nullptr);
hipError_t launch_rt_pack_rgb24(const uint32_t *, int, int, int, int, uint8_t *, hipStream_t);
hipError_t launch_rt_pack_radiance(const float *, size_t, float, uint32_t *, hipStream_t);
hipError_t launch_rt_assemble(const uint8_t *, const RtBlocks &, int, uint32_t *, size_t, hipStream_t);
hipError_t launch_rt_unstripe(const uint32_t *, int, int, int, int, int, int, uint32_t *, hipStream_t);
hipError_t launch_rt_probe_closest(const RtFrame &, const cg_tri *, const RtSphere *, const cg_vec4 *,
                                   const cg_vec4 *, int, cg_isect *, int *, hipStream_t);
hipError_t launch_rt_probe_direct_light(const RtFrame &, const RtTri *, const RtShade *, const RtSphere *,
                                        const cg_isect *, int, cg_vec3 *, hipStream_t);
// cg_rt_big.hip
hipError_t launch_rt_big(const RtFrame &, RtTri *, const RtShade *, const RtSphere *, const RtGrid &, void *,
                         uint32_t *, hipStream_t, const RtGeo *, const cg_tri *, int, const BigCaps &,
                         unsigned long long *, int, const RtHits * = nullptr);
bool rt_big_shadow_lists(const RtFrame &);
int rt_big_mode(const RtFrame &);
bool rt_grid_build(const cg_tri *, int, RtGrid &, std::vector<int> &, std::vector<int> &, size_t);
size_t rt_big_scratch_bytes(const RtFrame &, const BigCaps &, bool hits = false);
// cg_rt_brute.hip, cg_rt_hits.hip
hipError_t rt_render_brute(const RtFrame &, const cg_tri *, int, const RtSphere *, int, int, uint32_t *, hipStream_t);
hipError_t launch_rt_hits_small(const RtFrame &, const cg_tri *, const RtSphere *, const RtHits &, hipStream_t);
hipError_t launch_rt_pick(const RtFrame &, const cg_tri *, const RtSphere *, cg_vec4, cg_vec4, void *, cg_isect *, int *,
                          hipStream_t);
size_t rt_pick_scratch_bytes();
void rt_pixel_ray(const cg_rt_camera *, int, int, int, cg_vec4 *, cg_vec4 *);
// cg_scene.hip
SceneBounds rt_scene_bounds(const cg_tri *tris, int n_tris);
void rt_scene_box_from(const SceneBounds &b, int n_tris, const cg_sphere *spheres, int n_spheres, double lo[3],
                       double hi[3]);
void rt_hit_box_from(const SceneBounds &b, const cg_sphere *spheres, int n_spheres, float blo[3], float bhi[3]);
float rt_normal_bound(const SceneBounds &b, int n_spheres);
void rt_box_columns(const double lo[3], const double hi[3], const cg_rt_camera *cam, int *col0, int *col1);
// cg_hdr.hip
hipError_t launch_hdr_histogram(const float *, int, size_t, int, size_t, uint32_t *, cg_hdr_stats *, hipStream_t);
hipError_t launch_hdr_exposure(const uint32_t *, int, const cg_hdr_exposure_params &, const float *, float *,
                               hipStream_t);
hipError_t launch_rt_tonemap_pack(const float *, size_t, int, size_t, const float *, int, float, uint32_t *, size_t,
                                  hipStream_t);
hipError_t launch_rast_tonemap_pack(const float *, size_t, int, size_t, const float *, int, float, uint32_t *, size_t,
                                    hipStream_t);
// cg_bloom.hip: a chunk's pyramids (B_k into d_planes, n_frames * L.total pixels; U_k into d_pyr), and the composite
hipError_t launch_bloom_pyramid(const float *d_rgba, const BloomLayout &L, int n_frames, size_t sstride,
                                const float *d_scales, const cg_hdr_bloom_params &p, float *d_planes, float *d_pyr,
                                size_t pstride, hipStream_t st);
hipError_t launch_bloom_pack(const float *d_rgba, const float *d_pyr, const BloomLayout &L, int n_frames,
                             size_t sstride, size_t pstride, const float *d_scales, const cg_hdr_bloom_params &p,
                             int rule, int op, float white2, uint32_t *d_argb, size_t dstride, hipStream_t st);
// cg_api_rt.hip: cg_rt_render_frames_device, plus per-frame completion signals for cg_dist
int rt_render_frames(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                     const cg_rt_shard *shard, void *d_out, size_t frame_stride, int pix_format, void *stream,
                     uint32_t *d_done, uint32_t *target, const int *group_starts, int ngroups, int light_stride);

// ---- rasteriser ----
// cg_geometry.hip, cg_rast.hip
hipError_t launch_rast_clip(const cg_rast_params &prm, const cg_rtri *d_room, int n_room, const cg_rtri *d_boxes,
                            int n_boxes, cg_rtri *d_stage, int *d_counts, cg_vec4 *d_light, int *d_first,
                            hipStream_t st);
void launch_rast_post_direct(const RastArgs &A, const float4 *state, const int32_t *shadow, uint32_t *d_argb,
                             hipStream_t st, int pix = CG_PIX_ARGB8888);
int rast_make_args(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light,
                   const cg_vec4 *d_light, int tex_mask, RastArgs *out);
int rast_render_device(cg_ctx *ctx, const cg_rtri *d_tris, int n, const cg_rast_params *p,
                       cg_vec4 light, uint32_t *d_argb, float *d_depth, int32_t *d_shadow,
                       hipStream_t st, cg_stats *stats, int tex_mask);
int rast_draw_device(cg_ctx *c, const cg_rtri *d_room, int n_room, const cg_rtri *d_boxes, int n_boxes,
                     const cg_rast_params *p, uint32_t *d_argb, float *d_depth, int32_t *d_shadow,
                     hipStream_t st, cg_stats *stats, int **n_out, int tex_mask, const RastSeq *seq = nullptr,
                     int pix = CG_PIX_ARGB8888);
// cg_rast_big.hip
void rast_big_blocks(int *batch, int *chunk);
int rast_big_render(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light, uint32_t *d_argb,
                    float *d_depth, int32_t *d_shadow, hipStream_t st, cg_stats *stats, int tex_mask);
int rast_big_draw(cg_ctx *c, const cg_rtri *d_room, int n_room, const cg_rtri *d_boxes, int n_boxes,
                  const cg_rast_params *p, uint32_t *d_argb, float *d_depth, int32_t *d_shadow, hipStream_t st,
                  cg_stats *stats, int **n_out, int tex_mask, const RastSeq *seq, int pix = CG_PIX_ARGB8888);
// cg_rast_colour.hip
int rast_rand_stream(cg_ctx *c, int rnd_buf, int jt_buf, uint64_t offset, long long S, hipStream_t st, int32_t **out);
int rast_colour_fill(cg_ctx *c, const RastArgs &A, const cg_rast_params *p, const RowRec *recs, const int *count,
                     const RastHdr *hdr, const int *n_dev, int max_recs, float4 *state, float *d_depth,
                     int32_t *shadow, hipStream_t st, long long *n_shaded);
int rast_seq_colour_fill(cg_ctx *c, const RastArgs &A, const cg_rast_params *p, const RowRec *recs, const int *count,
                         const RastHdr *hdr, const int *n_dev, int max_recs, float4 *state, float *d_depth,
                         int32_t *shadow, hipStream_t st, const RastSeq &q);
int rast_seq_tables(cg_ctx *c, long long nb, long long *have, uint32_t **tables);
int rast_seq_chain_mode0(cg_ctx *c, hipStream_t st, const RastSeq &q);
int rast_seq_chain_exact(cg_ctx *c, hipStream_t st, const RastSeq &q, const long long *total);
int rast_rand_probe(cg_ctx *c, uint32_t *tables, int nb, const uint64_t *d_off, int n, int32_t *d_out, hipStream_t st);
long long rast_rand_chunks(long long nvals);
// cg_rast_buffers.hip
int rast_buffers_device(cg_ctx *c, const cg_rast_buffers *d, int n_room, hipStream_t st);
int rast_pick_device(cg_ctx *c, int n_room, int x, int y, hipStream_t st, int *out8);
int rast_frame_state_bytes(cg_ctx *c);

}  // namespace cg
