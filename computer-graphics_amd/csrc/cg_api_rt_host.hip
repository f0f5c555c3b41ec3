// cg_api_rt_host.hip -- raytracer frames delivered into host memory (cg_rt_render*, the HostFill
// threads) and the exposure chain's entry points with bloom (cg_hdr_*, cg_rt_render_exposed*).  Host
// code only.
#include <chrono>
#include <cstdlib>

#include "cg_bloom.h"
#include "cg_ctx.h"
#include "cg_hdr.h"

// Host-memory form of a CG_PIX_RGBA_F32 frame: one frame call into the context's scratch frame,
// then a download.
extern "C" int cg_rt_render_radiance(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                                     float *rgba, cg_stats *stats)
{
    if (!c || !rgba || !cam || cam->width <= 0 || cam->height <= 0) return CG_E_INVALID;
    if (c->n_tris < 0) {
        c->err = "render before cg_rt_set_scene";
        return CG_E_NOSCENE;
    }
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t bytes = (size_t)cam->width * cam->height * 16;
    CG_TRY(c, c->frame.ensure(bytes), "alloc frame");
    CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
    cg_rt_shard whole{0, 1, cam->height, 0, cam->height, 0, 0};   // a band of exactly the frame's rows
    if (int rc = cg_rt_render_frames_device(c, lights, n_lights, cam, 1, &whole, c->frame.p, 0, CG_PIX_RGBA_F32,
                                            c->stream))
        return rc;
    CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
    CG_TRY(c, hipMemcpyAsync(rgba, c->frame.p, bytes, hipMemcpyDeviceToHost, c->stream), "download frame");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rt frame");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = c->n_tris;
        stats->n_spans = 0;
    }
    return CG_OK;
}

// Host-buffer delivery of frames (cg_rt_render, cg_rt_render_frames): only the
// columns the camera can see anything in (cg_rt_frame_columns, from the
// scene's box) cross PCIe; the columns outside are certainly
// PutPixelSDL(0, 0, 0) = 0x80000000 (no ray there can hit anything,
// skeleton.cpp:160-166) and the host stores them itself while the GPU renders
// and copies.  C2: columns 384-1551, 61 % of the bytes.  CG_DRAW_WINDOW=0:
// whole rows (A/B runs).
static bool draw_window_on()
{
    static const bool on = [] {
        const char *e = std::getenv("CG_DRAW_WINDOW");
        return !(e && e[0] == '0');
    }();
    return on;
}
// [c0, c1) of frame f's download; false: whole rows
static bool draw_window(const cg_ctx *c, const cg_rt_camera *cam, int &c0, int &c1)
{
    c0 = 0;
    c1 = cam->width;
    if (!draw_window_on()) return false;
    ctx_rt_columns(c, cam, &c0, &c1);
    if (c1 <= c0) c0 = c1 = 0;   // nothing visible: a black frame, nothing to copy
    return c0 > 0 || c1 < cam->width;
}
// frames of rows x W pixels (row pitch W): columns outside [c0, c1) black, on
// the context's fill threads (CG_DRAW_THREADS, default min(8, cores / 2));
// returns at once, HostFill::wait() before the frames are complete
static HostFill *host_black_outside(cg_ctx *c, std::vector<HostFill::Frame> frames, int W, int rows, int c0, int c1)
{
    if (!c->hfill) {
        const char *e = std::getenv("CG_DRAW_THREADS");
        const int hw = (int)std::thread::hardware_concurrency();
        const int n = e && *e ? std::atoi(e) : std::min(8, std::max(1, hw / 2));
        c->hfill.reset(new HostFill(std::max(0, std::min(n, 64))));
    }
    c->hfill->run(std::move(frames), W, rows, c0, c1);
    return c->hfill.get();
}
// D2H of frames [nf frames of W x H at src (pitch W, frame stride px)] into
// dst (frame stride `stride`): the window's columns only (one pitched copy
// when the frames are contiguous on both sides), or everything.
static hipError_t download_frames(uint32_t *dst, size_t stride, const uint32_t *src, int W, int H, int nf, int c0,
                                  int c1, bool window, hipStream_t st, size_t sstride = 0)
{
    // sstride: the source's frame stride in pixels (0 = W * H; more when the frames' rows pad to stripes)
    const size_t px = sstride ? sstride : (size_t)W * H;
    if (sstride && sstride != (size_t)W * H) {
        for (int f = 0; f < nf; ++f) {
            const hipError_t e = window
                ? (c1 <= c0 ? hipSuccess
                            : hipMemcpy2DAsync(dst + (size_t)f * stride + c0, (size_t)W * 4, src + (size_t)f * px + c0,
                                               (size_t)W * 4, (size_t)(c1 - c0) * 4, H, hipMemcpyDeviceToHost, st))
                : hipMemcpyAsync(dst + (size_t)f * stride, src + (size_t)f * px, (size_t)W * H * 4,
                                 hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    if (!window) {
        if (stride == px) return hipMemcpyAsync(dst, src, (size_t)nf * px * 4, hipMemcpyDeviceToHost, st);
        for (int f = 0; f < nf; ++f) {
            const hipError_t e = hipMemcpyAsync(dst + (size_t)f * stride, src + (size_t)f * px, px * 4,
                                                hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    if (c1 <= c0) return hipSuccess;
    if (stride == px)
        return hipMemcpy2DAsync(dst + c0, (size_t)W * 4, src + c0, (size_t)W * 4, (size_t)(c1 - c0) * 4,
                                (size_t)nf * H, hipMemcpyDeviceToHost, st);
    for (int f = 0; f < nf; ++f) {
        const hipError_t e = hipMemcpy2DAsync(dst + (size_t)f * stride + c0, (size_t)W * 4, src + (size_t)f * px + c0,
                                              (size_t)W * 4, (size_t)(c1 - c0) * 4, H, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- auto-exposure and tone mapping (kernels: cg_hdr.hip; arithmetic: cg_hdr.h) ----
extern "C" int cg_hdr_histogram_device(cg_ctx *c, const float *d_pixels, int channels, size_t n_pixels, int n_frames,
                                       size_t frame_stride, uint32_t *d_hist, cg_hdr_stats *d_stats, void *stream)
{
    if (!c || n_frames < 0 || (channels != 3 && channels != 4) || n_pixels >= ((size_t)1 << 32)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const size_t stride = frame_stride ? frame_stride : n_pixels;
    if (!d_hist || ((uintptr_t)d_hist & 15) || ((uintptr_t)d_stats & 3) || (n_pixels && !d_pixels) ||
        ((uintptr_t)d_pixels & (channels == 4 ? 15 : 3)) || stride < n_pixels)
        return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_hdr_histogram(d_pixels, channels, n_pixels, n_frames, stride, d_hist, d_stats,
                                   stream ? (hipStream_t)stream : c->stream),
           "histogram launch");
    return CG_OK;
}

extern "C" int cg_hdr_exposure_device(cg_ctx *c, const uint32_t *d_hist, int n_frames,
                                      const cg_hdr_exposure_params *params, const float *d_prev, float *d_scales,
                                      void *stream)
{
    if (!c || n_frames < 0 || !hdr_params_ok(params)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    if (!d_hist || ((uintptr_t)d_hist & 15) || !d_scales || ((uintptr_t)d_scales & 3) || ((uintptr_t)d_prev & 3))
        return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_hdr_exposure(d_hist, n_frames, *params, d_prev, d_scales, stream ? (hipStream_t)stream : c->stream),
           "exposure launch");
    return CG_OK;
}

extern "C" int cg_rt_tonemap_pack_device(cg_ctx *c, const float *d_rgba, size_t n_pixels, int n_frames,
                                         size_t src_stride, const float *d_scales, int op, float white2,
                                         uint32_t *d_argb, size_t dst_stride, void *stream)
{
    if (!c || n_frames < 0 || !hdr_tone_ok(op, white2) || n_pixels >= ((size_t)1 << 32)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const size_t ss = src_stride ? src_stride : n_pixels, ds = dst_stride ? dst_stride : n_pixels;
    if (!d_scales || ((uintptr_t)d_scales & 3) || (n_pixels && (!d_rgba || !d_argb)) || ((uintptr_t)d_rgba & 15) ||
        ((uintptr_t)d_argb & 3) || ss < n_pixels || ds < n_pixels)
        return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_rt_tonemap_pack(d_rgba, n_pixels, n_frames, ss, d_scales, op, white2, d_argb, ds,
                                     stream ? (hipStream_t)stream : c->stream),
           "tonemap pack launch");
    return CG_OK;
}

constexpr int kHdrChunkFrames = 8;   // frames of cg_rt_render_exposed_device's scratch

// ---- bloom (kernels: cg_bloom.hip; arithmetic: cg_bloom.h) ----
// what both device bloom calls check of a frame set: size, strides (0: the plane) and alignment
static bool bloom_frames_ok(int W, int H, const cg_hdr_bloom_params *bloom, BloomLayout *L, const float *d_rgba,
                            size_t *sstride, const float *d_pyr, size_t *pstride, const float *d_scales)
{
    if (!bloom_params_ok(bloom) || !bloom_layout(W, H, bloom->levels, L) || (size_t)W * H >= ((size_t)1 << 32))
        return false;
    if (!*sstride) *sstride = (size_t)W * H;
    if (!*pstride) *pstride = L->total;
    return d_rgba && !((uintptr_t)d_rgba & 15) && d_pyr && !((uintptr_t)d_pyr & 15) && d_scales &&
           !((uintptr_t)d_scales & 3) && *sstride >= (size_t)W * H && *pstride >= L->total;
}

extern "C" int cg_hdr_bloom_device(cg_ctx *c, const float *d_rgba, int width, int height, int n_frames,
                                   size_t src_stride, const float *d_scales, const cg_hdr_bloom_params *bloom,
                                   float *d_pyr, size_t pyr_stride, void *stream)
{
    if (!c || n_frames < 0 || !bloom_params_ok(bloom) || width <= 0 || height <= 0) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    BloomLayout L;
    if (!bloom_frames_ok(width, height, bloom, &L, d_rgba, &src_stride, d_pyr, &pyr_stride, d_scales)) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // the unblurred planes of kHdrChunkFrames frames at a time
    CG_TRY(c, c->bloom_planes.ensure((size_t)std::min(n_frames, kHdrChunkFrames) * L.total * 16), "alloc bloom planes");
    for (int f0 = 0; f0 < n_frames; f0 += kHdrChunkFrames)
        CG_TRY(c, launch_bloom_pyramid(d_rgba + (size_t)f0 * src_stride * 4, L, std::min(kHdrChunkFrames, n_frames - f0),
                                       src_stride, d_scales + f0, *bloom, (float *)c->bloom_planes.p,
                                       d_pyr + (size_t)f0 * pyr_stride * 4, pyr_stride, st),
               "bloom launch");
    return CG_OK;
}

extern "C" int cg_hdr_bloom_pack_device(cg_ctx *c, const float *d_rgba, const float *d_pyr, int width, int height,
                                        int n_frames, size_t src_stride, size_t pyr_stride, const float *d_scales,
                                        const cg_hdr_bloom_params *bloom, int rule, int op, float white2,
                                        uint32_t *d_argb, size_t dst_stride, void *stream)
{
    if (!c || n_frames < 0 || !bloom_params_ok(bloom) || !bloom_rule_ok(rule) || !hdr_tone_ok(op, white2) ||
        width <= 0 || height <= 0)
        return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    BloomLayout L;
    if (!bloom_frames_ok(width, height, bloom, &L, d_rgba, &src_stride, d_pyr, &pyr_stride, d_scales)) return CG_E_INVALID;
    const size_t ds = dst_stride ? dst_stride : (size_t)width * height;
    if (!d_argb || ((uintptr_t)d_argb & 3) || ds < (size_t)width * height) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_bloom_pack(d_rgba, d_pyr, L, n_frames, src_stride, pyr_stride, d_scales, *bloom, rule, op, white2,
                                d_argb, ds, stream ? (hipStream_t)stream : c->stream),
           "bloom pack launch");
    return CG_OK;
}

// what both forms of cg_rt_render_exposed check before anything is enqueued
static int rt_exposed_check(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                            const cg_hdr_exposure_params *params, int op, float white2, size_t frame_stride,
                            const cg_hdr_bloom_params *bloom)
{
    if (!c || n_frames < 0 || (n_frames && !cams) || !hdr_params_ok(params) || !hdr_tone_ok(op, white2) ||
        (bloom && !bloom_params_ok(bloom)) ||
        n_lights < 0 || n_lights > kMaxLights || (n_lights && !lights))
        return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const int W = cams[0].width, H = cams[0].height;
    if (W <= 0 || H <= 0 || (size_t)W * H >= ((size_t)1 << 32)) return CG_E_INVALID;
    for (int f = 1; f < n_frames; ++f)
        if (cams[f].width != W || cams[f].height != H) return CG_E_INVALID;
    if (frame_stride && frame_stride < (size_t)W * H) return CG_E_INVALID;
    if (c->n_tris < 0) {
        c->err = "render before cg_rt_set_scene";
        return CG_E_NOSCENE;
    }
    return CG_OK;
}

// Frames f0 .. f0 + nf - 1 (nf <= kHdrChunkFrames) of an exposed call: rendered as CG_PIX_RGBA_F32
// into the context's scratch, then histogram, exposure (previous scale *d_prev) and pack, all on st.
// With bloom: the chunk's pyramids into scratch after the exposure, and the composite for the pack.
static int rt_exposed_chunk(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int f0, int nf,
                            int per_frame_lights, const cg_hdr_exposure_params &params, const float *d_prev, int op,
                            float white2, const cg_hdr_bloom_params *bloom, uint32_t *d_argb, size_t stride,
                            float *d_scales, hipStream_t st)
{
    const int H = cams[0].height;
    const size_t px = (size_t)cams[0].width * H;
    CG_TRY(c, c->hdr_rgba.ensure(kHdrChunkFrames * px * 16), "alloc exposure frames");
    CG_TRY(c, c->hdr_hist.ensure(kHdrChunkFrames * CG_HDR_BINS * sizeof(uint32_t)), "alloc exposure histograms");
    cg_rt_shard whole{0, 1, H, 0, H, 0, 0};   // a band of exactly the frame's rows
    const int rc = per_frame_lights
        ? cg_rt_render_sequence_device(c, lights + (size_t)f0 * n_lights, n_lights, cams + f0, nf, &whole,
                                       c->hdr_rgba.p, px, CG_PIX_RGBA_F32, st)
        : cg_rt_render_frames_device(c, lights, n_lights, cams + f0, nf, &whole, c->hdr_rgba.p, px, CG_PIX_RGBA_F32, st);
    if (rc) return rc;
    const float *rgba = (const float *)c->hdr_rgba.p;
    uint32_t *hist = (uint32_t *)c->hdr_hist.p;
    CG_TRY(c, launch_hdr_histogram(rgba, 4, px, nf, px, hist, nullptr, st), "histogram launch");
    CG_TRY(c, launch_hdr_exposure(hist, nf, params, d_prev, d_scales, st), "exposure launch");
    if (bloom) {
        BloomLayout L;
        if (!bloom_layout(cams[0].width, H, bloom->levels, &L)) return CG_E_INVALID;
        CG_TRY(c, c->bloom_planes.ensure(kHdrChunkFrames * L.total * 16), "alloc bloom planes");
        CG_TRY(c, c->bloom_pyr.ensure(kHdrChunkFrames * L.total * 16), "alloc bloom pyramids");
        float *pyr = (float *)c->bloom_pyr.p;
        CG_TRY(c, launch_bloom_pyramid(rgba, L, nf, px, d_scales, *bloom, (float *)c->bloom_planes.p, pyr, L.total, st),
               "bloom launch");
        CG_TRY(c, launch_bloom_pack(rgba, pyr, L, nf, px, L.total, d_scales, *bloom, CG_BLOOM_RULE_RT, op, white2, d_argb,
                                    stride, st),
               "bloom pack launch");
        return CG_OK;
    }
    CG_TRY(c, launch_rt_tonemap_pack(rgba, px, nf, px, d_scales, op, white2, d_argb, stride, st), "tonemap pack launch");
    return CG_OK;
}

extern "C" int cg_rt_render_exposed_bloom_device(cg_ctx *c, const cg_light *lights, int n_lights,
                                                 const cg_rt_camera *cams, int n_frames, int per_frame_lights,
                                                 const cg_hdr_exposure_params *params, const float *d_prev, int op,
                                                 float white2, const cg_hdr_bloom_params *bloom, uint32_t *d_argb,
                                                 size_t frame_stride, float *d_scales, void *stream)
{
    if (int rc = rt_exposed_check(c, lights, n_lights, cams, n_frames, params, op, white2, frame_stride, bloom)) return rc;
    if (n_frames == 0) return CG_OK;
    if (!d_argb || ((uintptr_t)d_argb & 3) || !d_scales || ((uintptr_t)d_scales & 3) || ((uintptr_t)d_prev & 3))
        return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t stride = frame_stride ? frame_stride : (size_t)cams[0].width * cams[0].height;
    for (int f0 = 0; f0 < n_frames; f0 += kHdrChunkFrames) {
        const int nf = std::min(kHdrChunkFrames, n_frames - f0);
        if (int rc = rt_exposed_chunk(c, lights, n_lights, cams, f0, nf, per_frame_lights, *params,
                                      f0 ? d_scales + f0 - 1 : d_prev, op, white2, bloom, d_argb + (size_t)f0 * stride,
                                      stride, d_scales + f0, st))
            return rc;
    }
    return CG_OK;
}

extern "C" int cg_rt_render_exposed_device(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                           int n_frames, int per_frame_lights, const cg_hdr_exposure_params *params,
                                           const float *d_prev, int op, float white2, uint32_t *d_argb,
                                           size_t frame_stride, float *d_scales, void *stream)
{
    return cg_rt_render_exposed_bloom_device(c, lights, n_lights, cams, n_frames, per_frame_lights, params, d_prev, op,
                                             white2, nullptr, d_argb, frame_stride, d_scales, stream);
}

// Host-memory form: the device form's chunks into context scratch, each chunk's frames downloaded
// after its render; the scales (and the caller's previous scale) live in one device array,
// [0] the previous scale, [1 + f] frame f's.
extern "C" int cg_rt_render_exposed_bloom(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                          int n_frames, int per_frame_lights, const cg_hdr_exposure_params *params,
                                          const float *prev, int op, float white2, const cg_hdr_bloom_params *bloom,
                                          uint32_t *argb, size_t frame_stride, float *scales, cg_stats *stats)
{
    if (int rc = rt_exposed_check(c, lights, n_lights, cams, n_frames, params, op, white2, frame_stride, bloom)) return rc;
    if (n_frames == 0) return CG_OK;
    if (!argb || !scales) return CG_E_INVALID;
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t px = (size_t)cams[0].width * cams[0].height;
    const size_t stride = frame_stride ? frame_stride : px;
    CG_TRY(c, c->hdr_argb.ensure(kHdrChunkFrames * px * sizeof(uint32_t)), "alloc exposed frames");
    CG_TRY(c, c->hdr_scales.ensure(((size_t)n_frames + 1) * sizeof(float)), "alloc scales");
    float *d_s = (float *)c->hdr_scales.p;
    uint32_t *d_a = (uint32_t *)c->hdr_argb.p;
    if (prev) CG_TRY(c, hipMemcpyAsync(d_s, prev, sizeof(float), hipMemcpyHostToDevice, c->stream), "upload scale");
    float ms_sum = 0.f;
    for (int f0 = 0; f0 < n_frames; f0 += kHdrChunkFrames) {
        const int nf = std::min(kHdrChunkFrames, n_frames - f0);
        CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
        if (int rc = rt_exposed_chunk(c, lights, n_lights, cams, f0, nf, per_frame_lights, *params,
                                      f0 || prev ? d_s + f0 : nullptr, op, white2, bloom, d_a, px, d_s + 1 + f0,
                                      c->stream))
            return rc;
        CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
        CG_TRY(c, download_frames(argb + (size_t)f0 * stride, stride, d_a, cams[0].width, cams[0].height, nf, 0,
                                  cams[0].width, false, c->stream),
               "download frames");
        CG_TRY(c, hipStreamSynchronize(c->stream), "exposed frames");
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        ms_sum += ms;
    }
    CG_TRY(c, hipMemcpy(scales, d_s + 1, (size_t)n_frames * sizeof(float), hipMemcpyDeviceToHost), "download scales");
    if (stats) {
        stats->kernel_ms = ms_sum;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = c->n_tris;
        stats->n_spans = 0;
    }
    return CG_OK;
}

extern "C" int cg_rt_render_exposed(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                    int n_frames, int per_frame_lights, const cg_hdr_exposure_params *params,
                                    const float *prev, int op, float white2, uint32_t *argb, size_t frame_stride,
                                    float *scales, cg_stats *stats)
{
    return cg_rt_render_exposed_bloom(c, lights, n_lights, cams, n_frames, per_frame_lights, params, prev, op, white2,
                                      nullptr, argb, frame_stride, scales, stats);
}

extern "C" int cg_rt_render(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                            uint32_t *argb, cg_stats *stats)
{
    if (!c || !argb) return CG_E_INVALID;
    auto t0 = std::chrono::steady_clock::now();
    RtFrame F;
    int rc = fill_frame(c, lights, n_lights, cam, nullptr, c->stream, F);
    if (rc) return rc;
    size_t bytes = (size_t)F.rows_out * F.W * sizeof(uint32_t);
    CG_TRY(c, c->frame.ensure(bytes), "alloc frame");
    CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
    rc = rt_enqueue(c, F, (uint32_t *)c->frame.p, c->stream);
    if (rc) return rc;
    CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
    int c0, c1;
    const bool window = draw_window(c, cam, c0, c1);
    // the black columns beside the render and the copy
    HostFill *hf = window ? host_black_outside(c, {{argb}}, F.W, F.H, c0, c1) : nullptr;
    const hipError_t e = download_frames(argb, (size_t)F.W * F.H, (const uint32_t *)c->frame.p, F.W, F.H, 1, c0, c1,
                                         window, c->stream);
    if (hf) hf->wait();
    CG_TRY(c, e, "download frame");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rt frame");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = c->n_tris;
        stats->n_spans = 0;
    }
    return CG_OK;
}

// n_frames frames into host memory: chunks of `chunk` frames render through
// rt_render_frames into two device slots on the context's stream; each
// chunk's download runs on `xfer` while the next chunk renders.  The download
// of chunk j is issued after chunk j + 1's render is enqueued: a pageable
// destination makes hipMemcpyAsync stage through the runtime's pinned buffers
// and return only when the copy is done, so issued in the other order the
// host would hold back the next render.
static int rt_render_frames_host(cg_ctx *c, const cg_light *lights, int n_lights, int light_stride,
                                 const cg_rt_camera *cams, int n_frames, uint32_t *argb, size_t frame_stride, int chunk,
                                 cg_stats *stats);
extern "C" int cg_rt_render_frames(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                   int n_frames, uint32_t *argb, size_t frame_stride, int chunk, cg_stats *stats)
{
    return rt_render_frames_host(c, lights, n_lights, 0, cams, n_frames, argb, frame_stride, chunk, stats);
}
extern "C" int cg_rt_render_sequence(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                     int n_frames, uint32_t *argb, size_t frame_stride, int chunk, cg_stats *stats)
{
    if (n_lights < 0 || n_lights > kMaxLights || (n_lights && !lights)) return CG_E_INVALID;
    return rt_render_frames_host(c, lights, n_lights, std::max(n_lights, 1), cams, n_frames, argb, frame_stride, chunk,
                                 stats);
}
// light_stride: 0 (common lights), else frame f's lights at lights + f * n_lights
static int rt_render_frames_host(cg_ctx *c, const cg_light *lights, int n_lights, int light_stride,
                                 const cg_rt_camera *cams, int n_frames, uint32_t *argb, size_t frame_stride, int chunk,
                                 cg_stats *stats)
{
    if (!c || !argb || n_frames < 0 || (n_frames && !cams) || chunk < 0) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const int W = cams[0].width, H = cams[0].height;
    if (W <= 0 || H <= 0) return CG_E_INVALID;
    for (int f = 1; f < n_frames; ++f)   // the slots hold chunks of W x H frames
        if (cams[f].width != W || cams[f].height != H) return CG_E_INVALID;
    const size_t px = (size_t)W * H;
    const size_t stride = frame_stride ? frame_stride : px;
    if (stride < px) return CG_E_INVALID;
    const int ch = chunk ? std::min(chunk, 64) : 8;
    CG_TRY(c, c->xfer.ensure(hipStreamNonBlocking), "copy stream");
    for (int k = 0; k < 2; ++k) {
        CG_TRY(c, c->ev_rdone[k].ensure(), "copy event");
        CG_TRY(c, c->ev_cdone[k].ensure(), "copy event");
    }
    // Every return below, error or not, leaves nothing of this call running:
    // earlier chunks' downloads may still be writing into argb (asynchronous
    // when it is pinned), and the stream may wait on their events.
    struct Drain {
        cg_ctx *c;
        ~Drain()
        {
            if (c->hfill) c->hfill->wait();   // the host's black columns
            (void)hipStreamSynchronize(c->xfer);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain_on_exit{c};
    // a slot's frames: the whole frame's rows in device memory (H padded to its 8-row stripes)
    const size_t spx = (size_t)cg_rt_shard_rows(H, nullptr) * W;
    for (int k = 0; k < 2; ++k) CG_TRY(c, c->hslot[k].ensure((size_t)ch * spx * sizeof(uint32_t)), "alloc frame slots");
    const int nchunks = (n_frames + ch - 1) / ch;
    auto download = [&](int j) -> int {
        const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        CG_TRY(c, hipStreamWaitEvent(c->xfer, c->ev_rdone[s], 0), "copy wait");
        // the chunk's union window (cg_rt_render's delivery, above)
        int a = W, b = 0;
        bool window = true;
        for (int f = f0; f < f0 + nf && window; ++f) {
            int x0, x1;
            window = draw_window(c, &cams[f], x0, x1);
            if (x1 > x0) {
                a = std::min(a, x0);
                b = std::max(b, x1);
            }
        }
        if (a >= b) a = b = 0;
        if (window) {   // the fill threads beside the copy (a pageable copy returns only when done)
            std::vector<HostFill::Frame> fr;
            for (int f = f0; f < f0 + nf; ++f) fr.push_back({argb + (size_t)f * stride});
            host_black_outside(c, std::move(fr), W, H, a, b);
        }
        CG_TRY(c, download_frames(argb + (size_t)f0 * stride, stride, (const uint32_t *)c->hslot[s].p, W, H, nf, a, b,
                                  window, c->xfer, spx), "download frames");
        CG_TRY(c, hipEventRecord(c->ev_cdone[s], c->xfer), "copy event");
        return CG_OK;
    };
    CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
    for (int j = 0; j < nchunks; ++j) {
        const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        if (j >= 2) CG_TRY(c, hipStreamWaitEvent(c->stream, c->ev_cdone[s], 0), "slot wait");   // chunk j - 2 downloaded
        int rc = rt_render_frames(c, lights && light_stride ? lights + (size_t)f0 * n_lights : lights, n_lights,
                                  cams + f0, nf, nullptr, c->hslot[s].p, spx, CG_PIX_ARGB8888, c->stream, nullptr, nullptr,
                                  nullptr, 0, light_stride);
        if (rc) return rc;
        CG_TRY(c, hipEventRecord(c->ev_rdone[s], c->stream), "render event");
        if (j >= 1 && (rc = download(j - 1))) return rc;
    }
    CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
    if (int rc = download(nchunks - 1)) return rc;
    CG_TRY(c, hipStreamSynchronize(c->xfer), "download frames");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rt frames");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = c->n_tris;
        stats->n_spans = 0;
        stats->n_shaded = -1;
    }
    return CG_OK;
}

// ---- frames delivered compressed (kernels: cg_jpeg_enc.hip) ----
int JpegDelivery::begin()
{
    slot_bytes = (size_t)W * H;   // a frame's device slot: a file this long is rare and is encoded again alone
    if (png) slot_bytes = (size_t)cg_image_png_bound(W, H, pprm.colour);   // exact frames: no file is longer
    if (exr) slot_bytes = (size_t)cg_image_exr_bound(W, H, eprm.channels, eprm.type);
    CG_TRY(c, c->xfer.ensure(hipStreamNonBlocking), "copy stream");
    for (int k = 0; k < 2; ++k) {
        CG_TRY(c, c->jpeg_rdone[k].ensure(), "copy event");
        CG_TRY(c, c->jpeg_cdone[k].ensure(), "copy event");
        CG_TRY(c, c->jpeg_out[k].ensure(256 * (((size_t)ch * 8 + 255) / 256) + (size_t)ch * slot_bytes), "alloc file slots");
    }
    CG_TRY(c, c->jpeg_len_host.ensure(2 * (size_t)ch * 8), "alloc host lengths");
    offsets[0] = 0;
    full = false;
    return CG_OK;
}

int JpegDelivery::slot_wait(int j)
{
    if (j >= 2) CG_TRY(c, hipStreamWaitEvent(c->stream, c->jpeg_cdone[j & 1], 0), "slot wait");
    return CG_OK;
}

int JpegDelivery::encode(int j, const void *d_frames_v, size_t frame_stride)
{
    const uint32_t *d_frames = (const uint32_t *)d_frames_v;
    const int s = j & 1, nf = std::min(ch, n_frames - j * ch);
    frames[s] = d_frames_v;
    fstride[s] = frame_stride;
    uint8_t *base = (uint8_t *)c->jpeg_out[s].p;
    const size_t lens_b = 256 * (((size_t)ch * 8 + 255) / 256);
    if (exr) {
        if (int rc = cg_image_encode_exr_device(c, (const float *)d_frames_v, W, H, nf, frame_stride, &eprm, base + lens_b, slot_bytes,
                                                (int64_t *)base, c->stream))
            return rc;
    } else if (int rc = png ? cg_image_encode_png_device(c, d_frames, W, H, nf, frame_stride, &pprm, base + lens_b, slot_bytes,
                                                  (int64_t *)base, c->stream)
                     : cg_image_encode_jpeg_device(c, d_frames, W, H, nf, frame_stride, &prm, base + lens_b, slot_bytes,
                                                   (int64_t *)base, c->stream))
        return rc;
    CG_TRY(c, hipEventRecord(c->jpeg_rdone[s], c->stream), "encode event");
    return CG_OK;
}

int JpegDelivery::deliver(int j)
{
    const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
    const uint8_t *base = (const uint8_t *)c->jpeg_out[s].p;
    const size_t lens_b = 256 * (((size_t)ch * 8 + 255) / 256);
    int64_t *h_len = (int64_t *)c->jpeg_len_host.p + (size_t)s * ch;
    CG_TRY(c, hipStreamWaitEvent(c->xfer, c->jpeg_rdone[s], 0), "copy wait");
    CG_TRY(c, hipMemcpyAsync(h_len, base, (size_t)nf * 8, hipMemcpyDeviceToHost, c->xfer), "d2h lengths");
    CG_TRY(c, hipStreamSynchronize(c->xfer), "jpeg lengths");
    for (int f = 0; f < nf; ++f) {
        int64_t len = h_len[f];
        const uint8_t *src = base + lens_b + (size_t)f * slot_bytes;
        const bool again = len == CG_E_CAPACITY && !png && !exr;
        if (again) {   // longer than W * H bytes: alone, into a slot no file can exceed, behind what the stream holds
            const size_t bound = (size_t)cg_image_jpeg_bound(W, H, prm.subsampling);
            CG_TRY(c, c->jpeg_big.ensure(256 + bound), "alloc file slot");
            uint8_t *big = (uint8_t *)c->jpeg_big.p;
            if (int rc = cg_image_encode_jpeg_device(c, (const uint32_t *)frames[s] + (size_t)f * fstride[s], W, H, 1, 0, &prm, big + 256, bound,
                                                     (int64_t *)big, c->stream))
                return rc;
            CG_TRY(c, hipMemcpyAsync(&len, big, 8, hipMemcpyDeviceToHost, c->stream), "d2h length");
            CG_TRY(c, hipStreamSynchronize(c->stream), "jpeg frame");
            src = big + 256;
        }
        if (len < 0) return ctx_invalid(c, "jpeg delivery: a file longer than its bound");
        const size_t at = offsets[f0 + f];
        offsets[f0 + f + 1] = at + (size_t)len;
        if (at + (size_t)len > cap) full = true;
        if (full) continue;
        if (again) CG_TRY(c, hipMemcpy(out + at, src, (size_t)len, hipMemcpyDeviceToHost), "download file");
        else CG_TRY(c, hipMemcpyAsync(out + at, src, (size_t)len, hipMemcpyDeviceToHost, c->xfer), "download file");
    }
    CG_TRY(c, hipEventRecord(c->jpeg_cdone[s], c->xfer), "copy event");
    return CG_OK;
}

int JpegDelivery::finish()
{
    CG_TRY(c, hipStreamSynchronize(c->xfer), "download files");
    CG_TRY(c, hipStreamSynchronize(c->stream), "frames");
    return offsets[n_frames] > cap ? CG_E_CAPACITY : CG_OK;
}

static bool jpeg_params_ok(const cg_jpeg_params *p)
{
    return p && p->quality >= 1 && p->quality <= 100 && (p->subsampling == CG_JPEG_444 || p->subsampling == CG_JPEG_420);
}

static bool png_params_ok(const cg_png_params *p)
{
    return p && (p->colour == CG_PNG_RGB || p->colour == CG_PNG_RGBA) &&
           (p->filter == CG_PNG_FILTER_ADAPTIVE || (p->filter >= 0 && p->filter <= 4));
}

// cg_rt_render_sequence's chunks (rt_render_frames_host above), each encoded on the context's stream
// behind its render; chunk j's files are copied while chunk j + 1 renders.  JPEG files under jp, or
// PNG files under pp, or EXR files under ep: then a chunk is at most 8 frames, rendered as
// CG_PIX_RGBA_F32 by the device sequence call into the exposed calls' float scratch -- one set is
// enough, since a chunk's encoding stands on the stream before the next chunk's render.
static int rt_sequence_files(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                             const cg_jpeg_params *jp, const cg_png_params *pp, const cg_exr_params *ep, uint8_t *out,
                             size_t cap, size_t *offsets, int chunk, cg_stats *stats)
{
    if (!c || !offsets || n_frames < 0 || (n_frames && !cams) || chunk < 0 || (!out && cap) ||
        (ep ? false : pp ? !png_params_ok(pp) : !jpeg_params_ok(jp)) || n_lights < 0 || n_lights > kMaxLights || (n_lights && !lights))
        return CG_E_INVALID;
    offsets[0] = 0;
    if (n_frames == 0) return CG_OK;
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const int W = cams[0].width, H = cams[0].height;
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return CG_E_INVALID;
    for (int f = 1; f < n_frames; ++f)
        if (cams[f].width != W || cams[f].height != H) return CG_E_INVALID;
    const int ch = std::min(chunk ? std::min(chunk, ep ? kHdrChunkFrames : 64) : 8, n_frames);
    struct Drain {
        cg_ctx *c;
        ~Drain()
        {
            (void)hipStreamSynchronize(c->xfer);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain_on_exit{c};
    JpegDelivery D{c, W, H, n_frames, ch, jp ? *jp : cg_jpeg_params{}, out, cap, offsets};
    if (pp) D.png = true, D.pprm = *pp;
    if (ep) D.exr = true, D.eprm = *ep;
    if (int rc = D.begin()) return rc;
    const size_t spx = (size_t)cg_rt_shard_rows(H, nullptr) * W, px = (size_t)W * H;
    if (ep) CG_TRY(c, c->hdr_rgba.ensure(kHdrChunkFrames * px * 16), "alloc picture frames");
    else
        for (int k = 0; k < 2; ++k) CG_TRY(c, c->hslot[k].ensure((size_t)ch * spx * sizeof(uint32_t)), "alloc frame slots");
    cg_rt_shard whole{0, 1, H, 0, H, 0, 0};   // a band of exactly the frame's rows
    const int nchunks = (n_frames + ch - 1) / ch;
    const int light_stride = std::max(n_lights, 1);
    CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
    for (int j = 0; j < nchunks; ++j) {
        const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        int rc = D.slot_wait(j);
        if (rc) return rc;
        if (ep) {
            rc = cg_rt_render_sequence_device(c, lights ? lights + (size_t)f0 * n_lights : lights, n_lights, cams + f0, nf,
                                              &whole, c->hdr_rgba.p, px, CG_PIX_RGBA_F32, c->stream);
            if (rc) return rc;
            if ((rc = D.encode(j, c->hdr_rgba.p, px))) return rc;
            if (j >= 1 && (rc = D.deliver(j - 1))) return rc;
            continue;
        }
        rc = rt_render_frames(c, lights ? lights + (size_t)f0 * n_lights : lights, n_lights, cams + f0, nf, nullptr,
                              c->hslot[s].p, spx, CG_PIX_ARGB8888, c->stream, nullptr, nullptr, nullptr, 0, light_stride);
        if (rc) return rc;
        if ((rc = D.encode(j, c->hslot[s].p, spx))) return rc;
        if (j >= 1 && (rc = D.deliver(j - 1))) return rc;
    }
    CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
    if (int rc = D.deliver(nchunks - 1)) return rc;
    const int rc = D.finish();
    if (rc != CG_OK && rc != CG_E_CAPACITY) return rc;
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = c->n_tris;
        stats->n_spans = 0;
        stats->n_shaded = -1;
    }
    return rc;
}

extern "C" int cg_rt_render_sequence_jpeg(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                          int n_frames, const cg_jpeg_params *params, uint8_t *out, size_t cap,
                                          size_t *offsets, int chunk, cg_stats *stats)
{
    return rt_sequence_files(c, lights, n_lights, cams, n_frames, params, nullptr, nullptr, out, cap, offsets, chunk, stats);
}

extern "C" int cg_rt_render_sequence_png(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                         int n_frames, const cg_png_params *params, uint8_t *out, size_t cap,
                                         size_t *offsets, int chunk, cg_stats *stats)
{
    if (!params) return CG_E_INVALID;
    return rt_sequence_files(c, lights, n_lights, cams, n_frames, nullptr, params, nullptr, out, cap, offsets, chunk, stats);
}

extern "C" int cg_rt_render_sequence_exr(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams,
                                         int n_frames, const cg_exr_params *params, uint8_t *out, size_t cap,
                                         size_t *offsets, int chunk, cg_stats *stats)
{
    cg_exr_params prm;
    if (!exr_resolve_params(params, &prm)) return CG_E_INVALID;
    return rt_sequence_files(c, lights, n_lights, cams, n_frames, nullptr, nullptr, &prm, out, cap, offsets, chunk, stats);
}
