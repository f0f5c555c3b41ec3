// cg_bloom.hip -- the bloom pyramid on the device: bright pass with the first box, the further
// boxes, blur with the up-add per level, and the composite in front of the tone curve.  The
// arithmetic is cg_bloom.h's, shared with the host-only cg_hdr_bloom* entry points at the end of
// this file.  A pyramid pixel is a float4 whose fourth float is +0.0f.
#include <algorithm>
#include <vector>

#include "cg_bloom.h"
#include "cg_host.h"

namespace cg {

constexpr int kBloomThreads = 256;
// Blur tile: 32 x 8 pixels a workgroup, one a lane, so a tile row is the 32 pixels (512 bytes) of
// half a wave; with the 2-pixel halo 36 x 12 pixels are staged and 32 x 12 hold the horizontal pass.
constexpr int kBloomTW = 32, kBloomTH = 8, kBloomHalo = 2;
constexpr int kBloomSW = kBloomTW + 2 * kBloomHalo, kBloomSH = kBloomTH + 2 * kBloomHalo;
static_assert(kBloomTW * kBloomTH == kBloomThreads, "one pixel a lane");

// B_1 of n_frames frames: a lane reads its 2 x 2 source pixels (clamped at the right and lower
// edge of an odd size), takes the bright pass of each at the frame's scale and stores their box.
// blockIdx.y strides over the frames, whose scale is a scalar load.
__global__ __launch_bounds__(kBloomThreads) void bloom_bright_box_kernel(const float4 *__restrict__ src, int W, int H,
                                                                        int W1, int H1, int n_frames, size_t sstride,
                                                                        const float *__restrict__ scales,
                                                                        float threshold, float cap,
                                                                        float4 *__restrict__ dst, size_t dstride)
{
    const size_t i = (size_t)blockIdx.x * kBloomThreads + threadIdx.x;
    if (i >= (size_t)W1 * H1) return;
    const int Y = (int)((unsigned)i / (unsigned)W1), X = (int)((unsigned)i - (unsigned)Y * (unsigned)W1);
    const int x0 = 2 * X, x1 = min(2 * X + 1, W - 1), y0 = 2 * Y, y1 = min(2 * Y + 1, H - 1);
    const size_t r0 = (size_t)y0 * W, r1 = (size_t)y1 * W;
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float s = scales[f];
        const float4 *p = src + (size_t)f * sstride;
        const float4 a = p[r0 + x0], b = p[r0 + x1], c = p[r1 + x0], d = p[r1 + x1];
        const Bloom3 ba = bloom_bright_pixel(a.x, a.y, a.z, a.w, s, threshold, cap);
        const Bloom3 bb = bloom_bright_pixel(b.x, b.y, b.z, b.w, s, threshold, cap);
        const Bloom3 bc = bloom_bright_pixel(c.x, c.y, c.z, c.w, s, threshold, cap);
        const Bloom3 bd = bloom_bright_pixel(d.x, d.y, d.z, d.w, s, threshold, cap);
        dst[(size_t)f * dstride + i] = make_float4(bloom_box(ba.x, bb.x, bc.x, bd.x), bloom_box(ba.y, bb.y, bc.y, bd.y),
                                                   bloom_box(ba.z, bb.z, bc.z, bd.z), 0.0f);
    }
}

// B_k from B_{k-1} (w0 x h0 at `from`, w1 x h1 at `to`, both inside a frame's planes of `stride` pixels)
__global__ __launch_bounds__(kBloomThreads) void bloom_box_kernel(float4 *__restrict__ planes, size_t from, size_t to,
                                                                 int w0, int h0, int w1, int h1, int n_frames,
                                                                 size_t stride)
{
    const size_t i = (size_t)blockIdx.x * kBloomThreads + threadIdx.x;
    if (i >= (size_t)w1 * h1) return;
    const int Y = (int)((unsigned)i / (unsigned)w1), X = (int)((unsigned)i - (unsigned)Y * (unsigned)w1);
    const int x0 = 2 * X, x1 = min(2 * X + 1, w0 - 1), y0 = 2 * Y, y1 = min(2 * Y + 1, h0 - 1);
    const size_t r0 = (size_t)y0 * w0, r1 = (size_t)y1 * w0;
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float4 *p = planes + (size_t)f * stride + from;
        const float4 a = p[r0 + x0], b = p[r0 + x1], c = p[r1 + x0], d = p[r1 + x1];
        planes[(size_t)f * stride + to + i] =
            make_float4(bloom_box(a.x, b.x, c.x, d.x), bloom_box(a.y, b.y, c.y, d.y), bloom_box(a.z, b.z, c.z, d.z), 0.0f);
    }
}

// The four taps of `up` at fine pixel (X, Y) from the coarse plane u (w x h)
__device__ __forceinline__ Bloom3 bloom_up_at(const float4 *__restrict__ u, int w, int h, int X, int Y)
{
    const int cx = bloom_up_near(X), nx = bloom_up_far(X, w), cy = bloom_up_near(Y), ny = bloom_up_far(Y, h);
    const float4 cc = u[(size_t)cy * w + cx], nc = u[(size_t)cy * w + nx];
    const float4 cn = u[(size_t)ny * w + cx], nn = u[(size_t)ny * w + nx];
    Bloom3 r;
    r.x = bloom_up(cc.x, nc.x, cn.x, nn.x);
    r.y = bloom_up(cc.y, nc.y, cn.y, nn.y);
    r.z = bloom_up(cc.z, nc.z, cn.z, nn.z);
    return r;
}

// U_k = G_k (+ up(U_{k+1}) below the coarsest level) of one level, w x h: a workgroup stages its
// B_k tile and halo in LDS with loads clamped to the level, runs the horizontal pass over the
// tile's rows and the halo's into LDS, then each lane the vertical pass of its pixel.  Clamped
// loads make a staged row or column outside the level the copy of the edge the contract names.
// `b` and `u` point at level k of frame 0's planes, `up` at level k + 1 of its pyramid (null at the
// coarsest level); blockIdx.z strides over the frames, blockIdx.y over the rows of tiles.
__global__ __launch_bounds__(kBloomThreads) void bloom_blur_up_kernel(const float4 *__restrict__ b, size_t bstride,
                                                                     int w, int h, const float4 *up, int uw, int uh,
                                                                     float4 *u, size_t ustride, int n_frames)
{
    __shared__ float4 in[kBloomSH][kBloomSW];
    __shared__ float4 hz[kBloomSH][kBloomTW];
    const int tid = threadIdx.x, lx = tid % kBloomTW, ly = tid / kBloomTW;
    const int tx0 = blockIdx.x * kBloomTW, gx = tx0 + lx;
    for (int f = blockIdx.z; f < n_frames; f += gridDim.z) {
        const float4 *src = b + (size_t)f * bstride;
        for (int ty0 = blockIdx.y * kBloomTH; ty0 < h; ty0 += gridDim.y * kBloomTH) {
            const int gy = ty0 + ly;
            for (int j = tid; j < kBloomSH * kBloomSW; j += kBloomThreads) {
                const int sy = j / kBloomSW, sx = j - sy * kBloomSW;
                const int x = min(max(tx0 + sx - kBloomHalo, 0), w - 1), y = min(max(ty0 + sy - kBloomHalo, 0), h - 1);
                in[sy][sx] = src[(size_t)y * w + x];
            }
            __syncthreads();
            for (int j = tid; j < kBloomSH * kBloomTW; j += kBloomThreads) {
                const int sy = j / kBloomTW, sx = j - sy * kBloomTW;
                const float4 m2 = in[sy][sx], m1 = in[sy][sx + 1], c = in[sy][sx + 2], p1 = in[sy][sx + 3], p2 = in[sy][sx + 4];
                hz[sy][sx] = make_float4(bloom_blur(m2.x, m1.x, c.x, p1.x, p2.x), bloom_blur(m2.y, m1.y, c.y, p1.y, p2.y),
                                         bloom_blur(m2.z, m1.z, c.z, p1.z, p2.z), 0.0f);
            }
            __syncthreads();
            if (gx < w && gy < h) {
                const float4 m2 = hz[ly][lx], m1 = hz[ly + 1][lx], c = hz[ly + 2][lx], p1 = hz[ly + 3][lx], p2 = hz[ly + 4][lx];
                float4 g = make_float4(bloom_blur(m2.x, m1.x, c.x, p1.x, p2.x), bloom_blur(m2.y, m1.y, c.y, p1.y, p2.y),
                                       bloom_blur(m2.z, m1.z, c.z, p1.z, p2.z), 0.0f);
                if (up) {
                    const Bloom3 a = bloom_up_at(up + (size_t)f * ustride, uw, uh, gx, gy);
                    g.x = g.x + a.x, g.y = g.y + a.y, g.z = g.z + a.z;
                }
                u[(size_t)f * ustride + (size_t)gy * w + gx] = g;
            }
            __syncthreads();   // the next tile stages into the same LDS
        }
    }
}

// d_argb of the composite (cg_hdr_bloom_pack_device): rt_tonemap_pack_kernel's shape plus the four
// U_1 taps of the pixel; rule and tone operator are uniform.
__global__ __launch_bounds__(kBloomThreads) void bloom_pack_kernel(const float4 *__restrict__ src,
                                                                  const float4 *__restrict__ pyr, int W, int H, int W1,
                                                                  int H1, int n_frames, size_t sstride, size_t pstride,
                                                                  const float *__restrict__ scales, float intensity,
                                                                  int rule, int op, float white2,
                                                                  uint32_t *__restrict__ dst, size_t dstride)
{
    const size_t i = (size_t)blockIdx.x * kBloomThreads + threadIdx.x;
    if (i >= (size_t)W * H) return;
    const int y = (int)((unsigned)i / (unsigned)W), x = (int)((unsigned)i - (unsigned)y * (unsigned)W);
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float s = scales[f];
        const float4 v = src[(size_t)f * sstride + i];
        const Bloom3 g = bloom_up_at(pyr + (size_t)f * pstride, W1, H1, x, y);
        dst[(size_t)f * dstride + i] = bloom_pack(v.x, v.y, v.z, v.w, g, s, intensity, rule, op, white2);
    }
}

static unsigned frames_dim(int n_frames) { return (unsigned)(n_frames < 65535 ? n_frames : 65535); }

// The whole pyramid of n_frames frames: B_1 .. B_levels into d_planes (a frame's at f * L.total
// pixels, laid out as its pyramid), then U_levels .. U_1 into d_pyr.
hipError_t launch_bloom_pyramid(const float *d_rgba, const BloomLayout &L, int n_frames, size_t sstride,
                                const float *d_scales, const cg_hdr_bloom_params &p, float *d_planes, float *d_pyr,
                                size_t pstride, hipStream_t st)
{
    float4 *B = (float4 *)d_planes, *U = (float4 *)d_pyr;
    const unsigned fy = frames_dim(n_frames);
    auto blocks = [](size_t n) { return (unsigned)((n + kBloomThreads - 1) / kBloomThreads); };
    hipLaunchKernelGGL(bloom_bright_box_kernel, dim3(blocks((size_t)L.w[1] * L.h[1]), fy), dim3(kBloomThreads), 0, st,
                       (const float4 *)d_rgba, L.w[0], L.h[0], L.w[1], L.h[1], n_frames, sstride, d_scales, p.threshold,
                       p.cap, B, L.total);
    for (int k = 2; k <= L.levels; ++k)
        hipLaunchKernelGGL(bloom_box_kernel, dim3(blocks((size_t)L.w[k] * L.h[k]), fy), dim3(kBloomThreads), 0, st, B,
                           L.off[k - 1], L.off[k], L.w[k - 1], L.h[k - 1], L.w[k], L.h[k], n_frames, L.total);
    for (int k = L.levels; k >= 1; --k) {
        const bool top = k == L.levels;
        const dim3 grid((unsigned)((L.w[k] + kBloomTW - 1) / kBloomTW),
                        (unsigned)std::min((L.h[k] + kBloomTH - 1) / kBloomTH, 65535), fy);
        hipLaunchKernelGGL(bloom_blur_up_kernel, grid, dim3(kBloomThreads), 0, st, (const float4 *)B + L.off[k], L.total,
                           L.w[k], L.h[k], top ? (const float4 *)nullptr : (const float4 *)U + L.off[k + 1],
                           top ? 0 : L.w[k + 1], top ? 0 : L.h[k + 1], U + L.off[k], pstride, n_frames);
    }
    return hipGetLastError();
}

hipError_t launch_bloom_pack(const float *d_rgba, const float *d_pyr, const BloomLayout &L, int n_frames,
                             size_t sstride, size_t pstride, const float *d_scales, const cg_hdr_bloom_params &p,
                             int rule, int op, float white2, uint32_t *d_argb, size_t dstride, hipStream_t st)
{
    const size_t n = (size_t)L.w[0] * L.h[0];
    hipLaunchKernelGGL(bloom_pack_kernel, dim3((unsigned)((n + kBloomThreads - 1) / kBloomThreads), frames_dim(n_frames)),
                       dim3(kBloomThreads), 0, st, (const float4 *)d_rgba, (const float4 *)d_pyr, L.w[0], L.h[0], L.w[1],
                       L.h[1], n_frames, sstride, pstride, d_scales, p.intensity, rule, op, white2, d_argb, dstride);
    return hipGetLastError();
}

}  // namespace cg

using namespace cg;

// ---- host-only restatements (no device, no context) -----------------------
extern "C" int cg_hdr_bloom_layout(int width, int height, int levels, int *widths, int *heights, size_t *offsets,
                                   size_t *total)
{
    BloomLayout L;
    if (!bloom_layout(width, height, levels, &L)) return CG_E_INVALID;
    for (int k = 1; k <= levels; ++k) {
        if (widths) widths[k - 1] = L.w[k];
        if (heights) heights[k - 1] = L.h[k];
        if (offsets) offsets[k - 1] = L.off[k];
    }
    if (total) *total = L.total;
    return levels;
}

namespace {
// a plane of three-channel pixels on the host
struct HostPlane {
    int w = 0, h = 0;
    std::vector<Bloom3> px;
    HostPlane(int w_, int h_) : w(w_), h(h_), px((size_t)w_ * h_) {}
    const Bloom3 &at(int x, int y) const { return px[(size_t)y * w + x]; }
    // indices clamped to the plane
    const Bloom3 &clamped(int x, int y) const { return at(std::min(std::max(x, 0), w - 1), std::min(std::max(y, 0), h - 1)); }
};
HostPlane host_box(const HostPlane &p)
{
    HostPlane o((p.w + 1) / 2, (p.h + 1) / 2);
    for (int Y = 0; Y < o.h; ++Y)
        for (int X = 0; X < o.w; ++X) {
            const int x0 = 2 * X, x1 = std::min(2 * X + 1, p.w - 1), y0 = 2 * Y, y1 = std::min(2 * Y + 1, p.h - 1);
            const Bloom3 &a = p.at(x0, y0), &b = p.at(x1, y0), &c = p.at(x0, y1), &d = p.at(x1, y1);
            o.px[(size_t)Y * o.w + X] = Bloom3{bloom_box(a.x, b.x, c.x, d.x), bloom_box(a.y, b.y, c.y, d.y),
                                               bloom_box(a.z, b.z, c.z, d.z)};
        }
    return o;
}
HostPlane host_blur(const HostPlane &p, int dx, int dy)
{
    HostPlane o(p.w, p.h);
    for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < p.w; ++x) {
            const Bloom3 &m2 = p.clamped(x - 2 * dx, y - 2 * dy), &m1 = p.clamped(x - dx, y - dy), &c = p.at(x, y);
            const Bloom3 &p1 = p.clamped(x + dx, y + dy), &p2 = p.clamped(x + 2 * dx, y + 2 * dy);
            o.px[(size_t)y * p.w + x] = Bloom3{bloom_blur(m2.x, m1.x, c.x, p1.x, p2.x), bloom_blur(m2.y, m1.y, c.y, p1.y, p2.y),
                                               bloom_blur(m2.z, m1.z, c.z, p1.z, p2.z)};
        }
    return o;
}
// up(u) at fine pixel (X, Y), u a plane of float4 pixels w x h
Bloom3 host_up_at(const float *u, int w, int h, int X, int Y)
{
    const int cx = bloom_up_near(X), nx = bloom_up_far(X, w), cy = bloom_up_near(Y), ny = bloom_up_far(Y, h);
    const float *cc = u + ((size_t)cy * w + cx) * 4, *nc = u + ((size_t)cy * w + nx) * 4;
    const float *cn = u + ((size_t)ny * w + cx) * 4, *nn = u + ((size_t)ny * w + nx) * 4;
    return Bloom3{bloom_up(cc[0], nc[0], cn[0], nn[0]), bloom_up(cc[1], nc[1], cn[1], nn[1]),
                  bloom_up(cc[2], nc[2], cn[2], nn[2])};
}
}  // namespace

extern "C" int cg_hdr_bloom(const float *rgba, int width, int height, float scale, const cg_hdr_bloom_params *bloom,
                            float *pyr)
{
    BloomLayout L;
    if (!rgba || !pyr || !bloom_params_ok(bloom) || !bloom_layout(width, height, bloom->levels, &L)) return CG_E_INVALID;
    HostPlane bright(width, height);
    for (size_t i = 0; i < bright.px.size(); ++i) {
        const float *v = rgba + i * 4;
        bright.px[i] = bloom_bright_pixel(v[0], v[1], v[2], v[3], scale, bloom->threshold, bloom->cap);
    }
    std::vector<HostPlane> G;   // G[k - 1] = G_k
    HostPlane prev = std::move(bright);
    for (int k = 1; k <= L.levels; ++k) {
        HostPlane B = host_box(prev);
        G.push_back(host_blur(host_blur(B, 1, 0), 0, 1));
        prev = std::move(B);
    }
    for (int k = L.levels; k >= 1; --k) {
        const HostPlane &g = G[k - 1];
        float *u = pyr + L.off[k] * 4;
        for (int y = 0; y < g.h; ++y)
            for (int x = 0; x < g.w; ++x) {
                Bloom3 r = g.at(x, y);
                if (k < L.levels) {
                    const Bloom3 a = host_up_at(pyr + L.off[k + 1] * 4, L.w[k + 1], L.h[k + 1], x, y);
                    r.x = r.x + a.x, r.y = r.y + a.y, r.z = r.z + a.z;
                }
                float *o = u + ((size_t)y * g.w + x) * 4;
                o[0] = r.x, o[1] = r.y, o[2] = r.z, o[3] = 0.0f;
            }
    }
    return CG_OK;
}

extern "C" int cg_hdr_bloom_pack(const float *rgba, const float *pyr, int width, int height, float scale,
                                 const cg_hdr_bloom_params *bloom, int rule, int op, float white2, uint32_t *argb)
{
    BloomLayout L;
    if (!rgba || !pyr || !argb || !bloom_params_ok(bloom) || !bloom_rule_ok(rule) || !hdr_tone_ok(op, white2) ||
        !bloom_layout(width, height, bloom->levels, &L))
        return CG_E_INVALID;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const float *v = rgba + i * 4;
            const Bloom3 g = host_up_at(pyr, L.w[1], L.h[1], x, y);
            argb[i] = bloom_pack(v[0], v[1], v[2], v[3], g, scale, bloom->intensity, rule, op, white2);
        }
    return CG_OK;
}
