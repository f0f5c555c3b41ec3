// cg_hdr.hip -- the exposure chain on the device: luminance histogram and frame record,
// exposure with eye adaptation, tone-mapped pack.  The arithmetic is cg_hdr.h's, shared with the
// host-only cg_hdr_* entry points at the end of this file.
#include <algorithm>
#include <cstdlib>

#include "cg_hdr.h"
#include "cg_host.h"

namespace cg {

constexpr int kHdrThreads = 256, kHdrWaves = kHdrThreads / 64;
constexpr int kHdrPer = 8;                               // pixels a thread loads before it bins any
constexpr size_t kHdrChunk = (size_t)kHdrThreads * kHdrPer;   // pixels of one workgroup step
constexpr int kHdrMaxBlocks = 1024;                      // workgroups of a histogram launch, over all its frames
constexpr int kHdrMaxBlocksFrame = 512;                  // ... and of one frame: each adds to the frame's 256 words

// d_hist and d_stats as a histogram launch expects them: counts 0, max_bits 0, min_bits all ones
__global__ __launch_bounds__(kHdrThreads) void hdr_clear_kernel(uint32_t *__restrict__ hist, cg_hdr_stats *stats,
                                                               int n_frames)
{
    const int f = blockIdx.x;
    if (f >= n_frames) return;
    hist[(size_t)f * kHdrBins + threadIdx.x] = 0u;
    if (stats && threadIdx.x < 8) ((uint32_t *)&stats[f])[threadIdx.x] = threadIdx.x == 4 ? 0xFFFFFFFFu : 0u;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// What a lane has seen of the current frame since the last flush.
struct HdrLane {
    uint32_t counted, dark, uncovered, max_bits, min_bits;
    __device__ void reset() { counted = dark = uncovered = max_bits = 0u, min_bits = 0xFFFFFFFFu; }
};

// Luminance histogram and record of n_frames planes (cg_hdr_histogram_device).  The grid strides
// over (frame, pixel): blockIdx.y over the frames, blockIdx.x over a frame's chunks of kHdrChunk
// pixels, and a workgroup flushes after its last chunk of a frame -- once per frame it visits,
// because every flush adds to the same 256 words and adds to one word run one after the other in
// the L2.  Each wave owns a 256-bin sub-histogram in LDS.  A rendered frame puts most of a wave
// into a few bins, and LDS adds of one wave to one address run one after the other, so before the
// LDS add up to `peel` rounds merge equal bins: the lanes that share the first pending lane's bin
// are counted by a ballot and added once.  Whatever is pending after that adds lane by lane.  Dark
// and uncovered pixels and the min / max stay in registers until the flush.  Global memory sees
// integer adds only at a flush: non-zero bins, and five words a wave for the record.
template <int CH>
__global__ __launch_bounds__(kHdrThreads) void hdr_histogram_kernel(const float *__restrict__ px, size_t n_pixels,
                                                                   int n_frames, size_t frame_stride, int peel,
                                                                   uint32_t *__restrict__ hist, cg_hdr_stats *stats)
{
    __shared__ uint32_t wh[kHdrWaves][kHdrBins];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < kHdrWaves; ++w) wh[w][tid] = 0u;
    __syncthreads();
    HdrLane acc;
    acc.reset();
    const size_t chunks = (n_pixels + kHdrChunk - 1) / kHdrChunk;
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
        for (size_t c = blockIdx.x; c < chunks; c += gridDim.x) {
            const size_t base = c * kHdrChunk;
            const float *plane = px + (size_t)f * frame_stride * CH;
            float L[kHdrPer];
            bool cov[kHdrPer], in[kHdrPer];
#pragma unroll
            for (int k = 0; k < kHdrPer; ++k) {   // every load first
                const size_t p = base + (size_t)k * kHdrThreads + tid;
                in[k] = p < n_pixels;
                cov[k] = true;
                L[k] = 0.f;
                if (in[k]) {
                    if (CH == 4) {
                        const float4 v = ((const float4 *)plane)[p];
                        L[k] = hdr_luminance(v.x, v.y, v.z);
                        cov[k] = v.w > 0.0f;
                    } else {
                        const float *v = plane + p * 3;
                        L[k] = hdr_luminance(v[0], v[1], v[2]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kHdrPer; ++k) {
                const bool counted = in[k] && cov[k] && hdr_counted(L[k]);
                const uint32_t bits = hdr_bits(L[k]);
                if (in[k] && !cov[k]) ++acc.uncovered;
                if (in[k] && cov[k] && !counted) ++acc.dark;
                if (counted) {
                    ++acc.counted;
                    acc.max_bits = bits > acc.max_bits ? bits : acc.max_bits;
                    acc.min_bits = bits < acc.min_bits ? bits : acc.min_bits;
                }
                const int bin = hdr_bin_of_bits(bits);
                bool pending = counted;
                for (int r = 0; r < peel; ++r) {
                    if (pending) {
                        const int b0 = __builtin_amdgcn_readfirstlane(bin);
                        const bool same = bin == b0;
                        const unsigned long long m = __ballot(same);
                        if (same) {
                            if (lane == __ffsll(m) - 1) atomicAdd(&wh[wave][b0], (uint32_t)__popcll(m));
                            pending = false;
                        }
                    }
                }
                if (pending) atomicAdd(&wh[wave][bin], 1u);
            }
            if (c + gridDim.x >= chunks) {   // the workgroup's last chunk of frame f: flush (workgroup-uniform)
                if (stats) {
                    const uint32_t n = wave_sum(acc.counted), d = wave_sum(acc.dark), u = wave_sum(acc.uncovered);
                    const uint32_t mx = wave_max(acc.max_bits), mn = ~wave_max(~acc.min_bits);
                    if (lane == 0) {
                        uint32_t *s = (uint32_t *)&stats[f];
                        if (n) atomicAdd(s + 0, n);
                        if (d) atomicAdd(s + 1, d);
                        if (u) atomicAdd(s + 2, u);
                        if (n) atomicMax(s + 3, mx), atomicMin(s + 4, mn);
                    }
                }
                acc.reset();
                __syncthreads();
                uint32_t s = 0;
#pragma unroll
                for (int w = 0; w < kHdrWaves; ++w) s += wh[w][tid], wh[w][tid] = 0u;
                if (s) atomicAdd(&hist[(size_t)f * kHdrBins + tid], s);
                __syncthreads();
            }
        }
    }
}

// d_scales[f] = s_f (cg_hdr_exposure_device), one workgroup.  A wave takes a frame: each lane sums
// four bins, an inclusive scan over the lanes gives the running sums, the first lane at or past k
// finds the bin among its four.  The t_f of up to 256 frames wait in LDS for thread 0, which runs
// the adaptation chain in frame order.  *prev is read before anything is stored.
__global__ __launch_bounds__(kHdrThreads) void hdr_exposure_kernel(const uint32_t *__restrict__ hist, int n_frames,
                                                                  cg_hdr_exposure_params p, const float *prev,
                                                                  float *scales)
{
    __shared__ float t[kHdrThreads];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float s = prev ? *prev : 0.f;
    bool have = prev != nullptr;
    for (int f0 = 0; f0 < n_frames; f0 += kHdrThreads) {
        const int nf = n_frames - f0 < kHdrThreads ? n_frames - f0 : kHdrThreads;
        for (int i = wave; i < nf; i += kHdrWaves) {
            const uint4 h = ((const uint4 *)hist)[(size_t)(f0 + i) * (kHdrBins / 4) + lane];
            const unsigned long long own = ((unsigned long long)h.x + h.y) + ((unsigned long long)h.z + h.w);
            unsigned long long run = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long o = __shfl_up(run, d);
                if (lane >= d) run += o;
            }
            const unsigned long long total = __shfl(run, 63), k = hdr_rank(total, p.permille);
            const unsigned long long m = __ballot(run >= k);
            const int first = m ? __ffsll(m) - 1 : 0;   // m == 0 only when total == 0
            if (lane == first) {
                // the first of the lane's four bins whose running sum reaches k
                const unsigned long long r0 = (run - own) + h.x, r1 = r0 + h.y, r2 = r1 + h.z;
                const int bin = 4 * lane + (r0 >= k ? 0 : (r1 >= k ? 1 : (r2 >= k ? 2 : 3)));
                t[i] = hdr_target_scale(total, bin, p);
            }
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < nf; ++i) {
                s = have ? (f0 + i == 0 ? s : hdr_adapt(s, t[i], p.rate)) : t[i];
                have = true;
                scales[f0 + i] = s;
            }
        }
        __syncthreads();
    }
}

// d_argb = put_pixel(tone(op, c * d_scales[f])) (cg_rt_tonemap_pack_device): one pixel a lane,
// 16 bytes in, 4 out; blockIdx.y strides over the frames, whose scale is a scalar load.
__global__ __launch_bounds__(256) void rt_tonemap_pack_kernel(const float4 *__restrict__ src, size_t n, int n_frames,
                                                              size_t sstride, const float *__restrict__ scales, int op,
                                                              float white2, uint32_t *__restrict__ dst, size_t dstride)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float s = scales[f];
        const float4 v = src[(size_t)f * sstride + i];
        dst[(size_t)f * dstride + i] = hdr_pack(v.x, v.y, v.z, s, op, white2);
    }
}

// rt_tonemap_pack_kernel with the rasteriser's border and clamp rules (cg_rast_tonemap_pack_device,
// hdr_rast_pack): an uncovered pixel packs to 0, a channel that is not positive to 0 before the scale.
__global__ __launch_bounds__(256) void rast_tonemap_pack_kernel(const float4 *__restrict__ src, size_t n, int n_frames,
                                                                size_t sstride, const float *__restrict__ scales,
                                                                int op, float white2, uint32_t *__restrict__ dst,
                                                                size_t dstride)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float s = scales[f];
        const float4 v = src[(size_t)f * sstride + i];
        dst[(size_t)f * dstride + i] = hdr_rast_pack(v.x, v.y, v.z, v.w, s, op, white2);
    }
}

// CG_HDR_PEEL: merge rounds before the LDS add (0 .. 8; default 1), for scripts/hdr_rate.py
static int hdr_peel()
{
    static const int v = [] {
        const char *e = std::getenv("CG_HDR_PEEL");
        const int n = e && *e ? std::atoi(e) : 1;
        return n < 0 ? 0 : (n > 8 ? 8 : n);
    }();
    return v;
}

// CG_HDR_BLOCKS: workgroups of a histogram launch (default kHdrMaxBlocks), for scripts/hdr_rate.py
static int hdr_blocks()
{
    static const int v = [] {
        const char *e = std::getenv("CG_HDR_BLOCKS");
        const int n = e && *e ? std::atoi(e) : kHdrMaxBlocks;
        return n < 1 ? 1 : (n > 65535 ? 65535 : n);
    }();
    return v;
}

hipError_t launch_hdr_histogram(const float *d_px, int channels, size_t n_pixels, int n_frames, size_t frame_stride,
                                uint32_t *d_hist, cg_hdr_stats *d_stats, hipStream_t st)
{
    hipLaunchKernelGGL(hdr_clear_kernel, dim3(n_frames), dim3(kHdrThreads), 0, st, d_hist, d_stats, n_frames);
    if (n_pixels == 0) return hipGetLastError();
    // gridDim.y frames in flight, gridDim.x workgroups striding over a frame's chunks: a workgroup
    // flushes once per frame it visits
    const size_t chunks = (n_pixels + kHdrChunk - 1) / kHdrChunk;
    const unsigned gy = (unsigned)std::min(n_frames, hdr_blocks());
    const unsigned per_frame = std::max(1u, std::min<unsigned>(kHdrMaxBlocksFrame, hdr_blocks() / gy));
    const unsigned gx = (unsigned)std::min<size_t>(chunks, per_frame);
    if (channels == 4)
        hipLaunchKernelGGL(hdr_histogram_kernel<4>, dim3(gx, gy), dim3(kHdrThreads), 0, st, d_px, n_pixels, n_frames,
                           frame_stride, hdr_peel(), d_hist, d_stats);
    else
        hipLaunchKernelGGL(hdr_histogram_kernel<3>, dim3(gx, gy), dim3(kHdrThreads), 0, st, d_px, n_pixels, n_frames,
                           frame_stride, hdr_peel(), d_hist, d_stats);
    return hipGetLastError();
}

hipError_t launch_hdr_exposure(const uint32_t *d_hist, int n_frames, const cg_hdr_exposure_params &p,
                               const float *d_prev, float *d_scales, hipStream_t st)
{
    hipLaunchKernelGGL(hdr_exposure_kernel, dim3(1), dim3(kHdrThreads), 0, st, d_hist, n_frames, p, d_prev, d_scales);
    return hipGetLastError();
}

hipError_t launch_rt_tonemap_pack(const float *d_rgba, size_t n, int n_frames, size_t sstride, const float *d_scales,
                                  int op, float white2, uint32_t *d_argb, size_t dstride, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_tonemap_pack_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(n_frames < 65535 ? n_frames : 65535)),
                       dim3(256), 0, st, (const float4 *)d_rgba, n, n_frames, sstride, d_scales, op, white2, d_argb,
                       dstride);
    return hipGetLastError();
}

hipError_t launch_rast_tonemap_pack(const float *d_rgba, size_t n, int n_frames, size_t sstride, const float *d_scales,
                                    int op, float white2, uint32_t *d_argb, size_t dstride, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rast_tonemap_pack_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(n_frames < 65535 ? n_frames : 65535)),
                       dim3(256), 0, st, (const float4 *)d_rgba, n, n_frames, sstride, d_scales, op, white2, d_argb,
                       dstride);
    return hipGetLastError();
}

}  // namespace cg

using namespace cg;

// ---- host-only restatements (no device, no context) -----------------------
extern "C" float cg_hdr_luminance(float x, float y, float z) { return hdr_luminance(x, y, z); }
extern "C" int cg_hdr_bin(float L) { return hdr_bin(L); }
extern "C" float cg_hdr_bin_edge(int bin) { return bin < 0 || bin >= kHdrBins ? 0.0f : hdr_bin_edge(bin); }
extern "C" float cg_hdr_tone(int op, float v, float white2) { return hdr_tone(op, v, white2); }
extern "C" uint32_t cg_rast_pack_pixel(const float rgba[4], float scale, int op, float white2)
{
    return rgba ? hdr_rast_pack(rgba[0], rgba[1], rgba[2], rgba[3], scale, op, white2) : 0u;
}

extern "C" int cg_hdr_exposure(const uint32_t *hist, int n_frames, const cg_hdr_exposure_params *params,
                               const float *prev, float *scales)
{
    if (n_frames < 0 || !hdr_params_ok(params) || (n_frames && (!hist || !scales))) return CG_E_INVALID;
    float s = prev ? *prev : 0.f;
    for (int f = 0; f < n_frames; ++f) {
        const uint32_t *h = hist + (size_t)f * kHdrBins;
        uint64_t total = 0;
        for (int b = 0; b < kHdrBins; ++b) total += h[b];
        const uint64_t k = hdr_rank(total, params->permille);
        uint64_t run = 0;
        int bin = kHdrBins - 1;
        for (int b = 0; b < kHdrBins; ++b) {
            run += h[b];
            if (run >= k) {
                bin = b;
                break;
            }
        }
        const float t = hdr_target_scale(total, bin, *params);
        if (f == 0) s = prev ? s : t;
        else s = hdr_adapt(s, t, params->rate);
        scales[f] = s;
    }
    return CG_OK;
}
