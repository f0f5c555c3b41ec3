// cg_starfield.hip -- the starfield program (starfield/Source/skeleton.cpp): 1000
// stars from glibc rand() (:41-46), projected and plotted white every frame
// (Draw :66-79, PutPixelSDL SDLauxiliary.h:149-161), drifting in z (Update :82-104).
// Stars are (x, y, z) float triples; host-side init/update, device draw.
// Resident stars (cg_starfield_set) run whole stretches of the main loop (:53-57) on the
// device: cg_starfield_run_device / _advance_device / _run, further down.
#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "cg_host.h"

using namespace cg;

// :41-46 -- (float(rand()) / float(RAND_MAX) - 0.5) * 2 is evaluated in double
extern "C" int cg_starfield_init(float *stars, int n)
{
    if (n < 0 || (n && !stars)) return CG_E_INVALID;
    if (n == 0) return CG_OK;
    int32_t *r = new (std::nothrow) int32_t[3 * (size_t)n];
    if (!r) return CG_E_INVALID;
    cg_glibc_rand(0, 3 * n, r);
    const float rmax = (float)2147483647;                 // float(RAND_MAX)
    for (int i = 0; i < n; ++i) {
        stars[3 * i + 0] = (float)(((double)((float)r[3 * i + 0] / rmax) - 0.5) * 2);
        stars[3 * i + 1] = (float)(((double)((float)r[3 * i + 1] / rmax) - 0.5) * 2);
        stars[3 * i + 2] = (float)r[3 * i + 2] / rmax;
    }
    delete[] r;
    return CG_OK;
}

// Update (:82-104) for a frame time dt (ms; the reference's float(t2 - t))
extern "C" int cg_starfield_update(float *stars, int n, float dt)
{
    if (n < 0 || (n && !stars)) return CG_E_INVALID;
    for (int i = 0; i < n; ++i) {
        float z = stars[3 * i + 2];
        if (z <= 0) z += 1;
        if (z > 1) z -= 1;
        stars[3 * i + 2] = (float)((double)z - (0.0005 * (double)dt));
    }
    return CG_OK;
}

namespace cg {

__global__ void star_clear_kernel(uint32_t *argb, int npx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npx) argb[i] = 0u;                             // :69 memset
}

// Draw (:66-79): u = (W/2)(x/z) + W/2, v likewise; PutPixelSDL truncates to int
// (x86 cvttss2si) and skips pixels off the screen.  Coinciding stars write
// the same white pixel.
__global__ void star_draw_kernel(const float *__restrict__ stars, int n, int W, int H, uint32_t *argb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = stars[3 * i], y = stars[3 * i + 1], z = stars[3 * i + 2];
    const float u = ((float)(W / 2) * (x / z)) + (float)(W / 2);
    const float v = ((float)(H / 2) * (y / z)) + (float)(H / 2);
    const int px = f2i_x86(u), py = f2i_x86(v);
    if (px < 0 || px >= W || py < 0 || py >= H) return;   // "apa"
    argb[(size_t)py * W + px] = put_pixel(v3(1.0f, 1.0f, 1.0f));
}

}  // namespace cg

// One starfield frame into the caller's W*H ARGB buffer (Draw :66-79).
extern "C" int cg_starfield_draw(cg_ctx *c, const float *stars, int n, int width, int height, uint32_t *argb)
{
    if (!c || n < 0 || (n && !stars) || !argb || width <= 0 || height <= 0) return CG_E_INVALID;
    hipError_t e;
    const size_t npx = (size_t)width * height;
    float *d_st = (float *)ctx_buf(c, kBufStars, (size_t)(n > 0 ? n : 1) * 3 * sizeof(float), &e);
    if (!d_st) return ctx_fail(c, e, "alloc stars");
    uint32_t *d_px = (uint32_t *)ctx_buf(c, kBufStarFrame, npx * sizeof(uint32_t), &e);
    if (!d_px) return ctx_fail(c, e, "alloc starfield frame");
    hipStream_t st = ctx_stream(c);
    if (n && (e = hipMemcpyAsync(d_st, stars, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess)
        return ctx_fail(c, e, "upload stars");
    hipLaunchKernelGGL(star_clear_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, d_px, (int)npx);
    if (n) hipLaunchKernelGGL(star_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_st, n, width, height, d_px);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "starfield launch");
    if ((e = hipMemcpyAsync(argb, d_px, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return ctx_fail(c, e, "starfield frame");
    return CG_OK;
}

// ---------------------------------------------------------------------------
// Resident stars: the main loop (:53-57) on the device.

namespace cg {

// One star's Update (:91-96); d = 0.0005 * (double)dt.  The wraps are float adds, the step
// is the reference's double subtraction rounded back to float.
__device__ __forceinline__ float star_step(float z, double d)
{
    if (z <= 0) z += 1;
    if (z > 1) z -= 1;
    return (float)((double)z - d);
}

// Frames 0 .. nf - 1 of a launch, frame f = Draw of the stars after f updates, update f with
// steps.d[f] (nu = nf or nf - 1 updates in all).  Thread (star i, frame block blockIdx.y):
// replays the updates before its block's first frame in registers, then draws and updates
// through its kStarBlockFrames frames.  A z is a sequential recurrence (each update rounds and
// the wraps depend on the rounded value), so the replay is the only exact way to frame f; it
// is a handful of ALU operations a step and no memory traffic.  The last block's threads hold
// the state after the launch and store it to zout, which is not zin: the other blocks still
// replay from zin.  Coinciding stars store the same white pixel, so plain stores do.
__global__ __launch_bounds__(256) void star_run_kernel(const float2 *__restrict__ xy, const float *__restrict__ zin,
                                                       float *__restrict__ zout, int n, int nf, int nu, int W, int H,
                                                       uint32_t *__restrict__ argb, size_t stride, StarSteps steps)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f0 = (int)blockIdx.y * kStarBlockFrames;
    const int f1 = min(f0 + kStarBlockFrames, nf);
    float z = zin[i];
    // f < f0 <= nf - 1 <= nu; f0 is a multiple of the block length: one wide scalar load a block
    for (int fb = 0; fb < f0; fb += kStarBlockFrames) {
#pragma unroll
        for (int k = 0; k < kStarBlockFrames; ++k) z = star_step(z, steps.d[fb + k]);
    }
    const float2 p = xy[i];
    const float hw = (float)(W / 2), hh = (float)(H / 2);
    const uint32_t white = put_pixel(v3(1.0f, 1.0f, 1.0f));
    for (int f = f0; f < f1; ++f) {
        const float u = (hw * (p.x / z)) + hw;
        const float v = (hh * (p.y / z)) + hh;
        const int px = f2i_x86(u), py = f2i_x86(v);
        if (px >= 0 && px < W && py >= 0 && py < H) argb[(size_t)f * stride + (size_t)py * W + px] = white;
        if (f < nu) z = star_step(z, steps.d[f]);
    }
    if (f1 == nf) zout[i] = z;
}

// Update x nu with no drawing: one thread a star, in place (nobody else reads the star).
__global__ __launch_bounds__(256) void star_advance_kernel(float *__restrict__ z, int n, int nu, StarSteps steps)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = z[i];
    for (int f = 0; f < nu; ++f) v = star_step(v, steps.d[f]);
    z[i] = v;
}

}  // namespace cg

#define STAR_TRY(ctx, call, what)                                \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return ctx_fail((ctx), e_, (what)); \
    } while (0)

static void star_steps(StarSteps &s, const float *dts, int n)
{
    for (int k = 0; k < n; ++k) s.d[k] = 0.0005 * (double)dts[k];
    for (int k = n; k < kStarLaunchFrames; ++k) s.d[k] = 0.0;
}

// The checks of a run that need no device.
static int star_check_run(const cg_ctx *c, const float *dts, int n_updates, int n_frames, int width, int height)
{
    if (!c || n_updates < 0 || n_frames < 0 || (n_updates != n_frames && n_updates != n_frames - 1) || width <= 0 ||
        height <= 0 || (n_updates > 0 && !dts))
        return CG_E_INVALID;
    return CG_OK;
}

// n_frames frames at d_argb + f * stride and n_updates updates of the resident stars, enqueued
// on st: the clears first, then one launch per kStarLaunchFrames frames, each from the state
// the one before stored.  n_frames 0: updates only.
static int star_enqueue(cg_ctx *c, StarState *S, const float *dts, int n_updates, int n_frames, int W, int H,
                        uint32_t *d_argb, size_t stride, hipStream_t st)
{
    const size_t px = (size_t)W * H;
    if (n_frames > 0) {   // :68, every frame's memset ahead of the plots in stream order
        if (stride == px) {
            STAR_TRY(c, hipMemsetAsync(d_argb, 0, (size_t)n_frames * px * sizeof(uint32_t), st), "clear frames");
        } else {
            for (int f = 0; f < n_frames; ++f)
                STAR_TRY(c, hipMemsetAsync(d_argb + (size_t)f * stride, 0, px * sizeof(uint32_t), st), "clear frame");
        }
    }
    const int n = S->n;
    StarSteps steps;
    if (n > 0 && n_frames > 0) {
        for (int F0 = 0; F0 < n_frames; F0 += kStarLaunchFrames) {
            const int nf = std::min(kStarLaunchFrames, n_frames - F0), nu = std::min(nf, n_updates - F0);
            star_steps(steps, dts ? dts + F0 : nullptr, nu);
            const dim3 grid((unsigned)((n + 255) / 256), (unsigned)((nf + kStarBlockFrames - 1) / kStarBlockFrames));
            hipLaunchKernelGGL(star_run_kernel, grid, dim3(256), 0, st, (const float2 *)S->xy.p,
                               (const float *)S->z[S->cur].p, (float *)S->z[S->cur ^ 1].p, n, nf, nu, W, H,
                               d_argb + (size_t)F0 * stride, stride, steps);
            S->cur ^= 1;
        }
    } else if (n > 0) {
        for (int U0 = 0; U0 < n_updates; U0 += kStarLaunchFrames) {
            const int nu = std::min(kStarLaunchFrames, n_updates - U0);
            star_steps(steps, dts + U0, nu);
            hipLaunchKernelGGL(star_advance_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               (float *)S->z[S->cur].p, n, nu, steps);
        }
    }
    STAR_TRY(c, hipGetLastError(), "starfield launch");
    STAR_TRY(c, hipEventRecord(S->last, st), "starfield event");
    S->pending = true;
    return CG_OK;
}

extern "C" int cg_starfield_plan(int n_stars, int n_frames, int *frames_per_launch, int *frames_per_block)
{
    if (n_stars < 0 || n_frames < 0) return CG_E_INVALID;
    if (frames_per_launch) *frames_per_launch = kStarLaunchFrames;
    if (frames_per_block) *frames_per_block = kStarBlockFrames;
    return (n_frames + kStarLaunchFrames - 1) / kStarLaunchFrames;
}

extern "C" int cg_starfield_set(cg_ctx *c, const float *stars, int n)
{
    if (!c || n < 0 || (n && !stars)) return CG_E_INVALID;
    STAR_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    StarState *S = ctx_star(c);
    if (S->pending) STAR_TRY(c, hipEventSynchronize(S->last), "starfield wait");   // earlier runs read the old set
    STAR_TRY(c, S->last.ensure(), "starfield event");
    if (n > S->cap || !S->xy.p) {
        const int cap = std::max(n, 1);
        S->xy.release();
        S->z[0].release();
        S->z[1].release();
        S->cap = 0;
        S->n = -1;
        STAR_TRY(c, S->xy.ensure((size_t)cap * sizeof(float2)), "alloc stars");
        STAR_TRY(c, S->z[0].ensure((size_t)cap * sizeof(float)), "alloc stars");
        STAR_TRY(c, S->z[1].ensure((size_t)cap * sizeof(float)), "alloc stars");
        S->cap = cap;
    }
    if (n) {
        std::vector<float> xy(2 * (size_t)n), z((size_t)n);
        for (int i = 0; i < n; ++i) {
            xy[2 * (size_t)i] = stars[3 * (size_t)i];
            xy[2 * (size_t)i + 1] = stars[3 * (size_t)i + 1];
            z[i] = stars[3 * (size_t)i + 2];
        }
        hipStream_t st = ctx_stream(c);
        STAR_TRY(c, hipMemcpyAsync(S->xy.p, xy.data(), xy.size() * sizeof(float), hipMemcpyHostToDevice, st), "upload stars");
        STAR_TRY(c, hipMemcpyAsync(S->z[0].p, z.data(), z.size() * sizeof(float), hipMemcpyHostToDevice, st), "upload stars");
        STAR_TRY(c, hipStreamSynchronize(st), "upload stars");
    }
    S->cur = 0;
    S->n = n;
    return CG_OK;
}

extern "C" int cg_starfield_get(cg_ctx *c, float *stars, int cap)
{
    if (!c || cap < 0) return CG_E_INVALID;
    StarState *S = ctx_star(c);
    if (S->n < 0) return CG_E_NOSCENE;
    if (cap < S->n) return CG_E_CAPACITY;
    const int n = S->n;
    if (n == 0) return 0;
    if (!stars) return CG_E_INVALID;
    STAR_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    if (S->pending) STAR_TRY(c, hipEventSynchronize(S->last), "starfield wait");
    std::vector<float> xy(2 * (size_t)n), z((size_t)n);
    hipStream_t st = ctx_stream(c);
    STAR_TRY(c, hipMemcpyAsync(xy.data(), S->xy.p, xy.size() * sizeof(float), hipMemcpyDeviceToHost, st), "download stars");
    STAR_TRY(c, hipMemcpyAsync(z.data(), S->z[S->cur].p, z.size() * sizeof(float), hipMemcpyDeviceToHost, st),
             "download stars");
    STAR_TRY(c, hipStreamSynchronize(st), "download stars");
    for (int i = 0; i < n; ++i) {
        stars[3 * (size_t)i] = xy[2 * (size_t)i];
        stars[3 * (size_t)i + 1] = xy[2 * (size_t)i + 1];
        stars[3 * (size_t)i + 2] = z[i];
    }
    return n;
}

extern "C" int cg_starfield_run_device(cg_ctx *c, const float *dts, int n_updates, int n_frames, int width, int height,
                                       uint32_t *d_argb, size_t frame_stride, void *stream)
{
    if (int rc = star_check_run(c, dts, n_updates, n_frames, width, height)) return rc;
    const size_t px = (size_t)width * height, stride = frame_stride ? frame_stride : px;
    if (stride < px || (n_frames && !d_argb)) return CG_E_INVALID;
    StarState *S = ctx_star(c);
    if (S->n < 0) return CG_E_NOSCENE;
    if (n_frames == 0) return CG_OK;
    STAR_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    return star_enqueue(c, S, dts, n_updates, n_frames, width, height, d_argb, stride,
                        stream ? (hipStream_t)stream : ctx_stream(c));
}

extern "C" int cg_starfield_advance_device(cg_ctx *c, const float *dts, int n_updates, void *stream)
{
    if (!c || n_updates < 0 || (n_updates > 0 && !dts)) return CG_E_INVALID;
    StarState *S = ctx_star(c);
    if (S->n < 0) return CG_E_NOSCENE;
    if (n_updates == 0) return CG_OK;
    STAR_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    return star_enqueue(c, S, dts, n_updates, 0, 1, 1, nullptr, 1, stream ? (hipStream_t)stream : ctx_stream(c));
}

// The frames of cg_starfield_run_device into host memory: chunks of `chunk` frames render into
// two device slots on the context's stream and each chunk downloads on `xfer` while the next
// renders.  Chunk j's download is issued after chunk j + 1's render is enqueued, because a copy
// into pageable memory returns only when it is done.
extern "C" int cg_starfield_run(cg_ctx *c, const float *dts, int n_updates, int n_frames, int width, int height,
                                uint32_t *argb, size_t frame_stride, int chunk, cg_stats *stats)
{
    if (int rc = star_check_run(c, dts, n_updates, n_frames, width, height)) return rc;
    const size_t px = (size_t)width * height, stride = frame_stride ? frame_stride : px;
    if (stride < px || chunk < 0 || (n_frames && !argb)) return CG_E_INVALID;
    StarState *S = ctx_star(c);
    if (S->n < 0) return CG_E_NOSCENE;
    if (n_frames == 0) return CG_OK;
    auto t0 = std::chrono::steady_clock::now();
    STAR_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    const int ch = std::min(chunk ? std::min(chunk, 64) : 8, n_frames);
    hipStream_t st = ctx_stream(c);
    STAR_TRY(c, S->xfer.ensure(hipStreamNonBlocking), "copy stream");
    for (int k = 0; k < 2; ++k) {
        STAR_TRY(c, S->rdone[k].ensure(), "copy event");
        STAR_TRY(c, S->cdone[k].ensure(), "copy event");
    }
    // every return below leaves nothing of this call running
    struct Drain {
        hipStream_t a, b;
        ~Drain()
        {
            (void)hipStreamSynchronize(a);
            (void)hipStreamSynchronize(b);
        }
    } drain_on_exit{S->xfer, st};
    if (S->slot_px < (size_t)ch * px) {
        STAR_TRY(c, hipStreamSynchronize(S->xfer), "copy stream");
        STAR_TRY(c, hipStreamSynchronize(st), "starfield stream");
        for (DevBuf &b : S->slot) b.release();
        S->slot_px = 0;
        for (DevBuf &b : S->slot) STAR_TRY(c, b.ensure((size_t)ch * px * sizeof(uint32_t)), "alloc frame slots");
        S->slot_px = (size_t)ch * px;
    }
    const int nchunks = (n_frames + ch - 1) / ch;
    auto download = [&](int j) -> int {
        const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        STAR_TRY(c, hipStreamWaitEvent(S->xfer, S->rdone[s], 0), "copy wait");
        if (stride == px) {
            STAR_TRY(c, hipMemcpyAsync(argb + (size_t)f0 * stride, S->slot[s].p, (size_t)nf * px * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, S->xfer), "download frames");
        } else {
            for (int f = 0; f < nf; ++f)
                STAR_TRY(c, hipMemcpyAsync(argb + (size_t)(f0 + f) * stride, (uint32_t *)S->slot[s].p + (size_t)f * px,
                                           px * sizeof(uint32_t), hipMemcpyDeviceToHost, S->xfer), "download frames");
        }
        STAR_TRY(c, hipEventRecord(S->cdone[s], S->xfer), "copy event");
        return CG_OK;
    };
    hipEvent_t ev0, ev1;
    ctx_events(c, &ev0, &ev1);
    STAR_TRY(c, hipEventRecord(ev0, st), "event");
    for (int j = 0; j < nchunks; ++j) {
        const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        if (j >= 2) STAR_TRY(c, hipStreamWaitEvent(st, S->cdone[s], 0), "slot wait");   // chunk j - 2 downloaded
        int rc = star_enqueue(c, S, dts ? dts + f0 : nullptr, std::min(nf, n_updates - f0), nf, width, height,
                              (uint32_t *)S->slot[s].p,
                              px, st);
        if (rc) return rc;
        STAR_TRY(c, hipEventRecord(S->rdone[s], st), "render event");
        if (j >= 1 && (rc = download(j - 1))) return rc;
    }
    STAR_TRY(c, hipEventRecord(ev1, st), "event");
    if (int rc = download(nchunks - 1)) return rc;
    STAR_TRY(c, hipStreamSynchronize(S->xfer), "download frames");
    STAR_TRY(c, hipStreamSynchronize(st), "starfield frames");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = 0;
        stats->n_spans = 0;
        stats->n_shaded = -1;
    }
    return CG_OK;
}
