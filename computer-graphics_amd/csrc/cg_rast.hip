// cg_rast.hip -- rasteriser fill + post-pass for gfx950 (MI355X).
//
// Reference: rasteriser/Source/skeleton.cpp, texture mode 0 / colour mode 0.
// Launches per frame (after rast_geometry_kernel, cg_geometry.hip, when the
// geometry runs on the device), all order-exact (no atomics touch colour/depth):
//   1. rast_setup_kernel   (one workgroup per clipped triangle)
//        VertexShader (:510-522) x3, then ComputePolygonRows (:433-498):
//        every edge sample of Interpolate (:524-551) is reduced into its row
//        with a 64-bit LDS min/max whose key is (x, sample sequence), which
//        reproduces the reference's `<=` / `>=` "later sample wins ties"
//        updates exactly; each visible row becomes a RastSpan holding what
//        DrawPolygonRows' Interpolate needs.
//   2. rast_rows_kernel    (one wave per screen row)
//        64-byte RowRec per triangle covering the row, in triangle order
//        (ballot + popcount compaction).
//   3. rast_fill_kernel    (one wave per 64-pixel row segment)
//        walks its row's records in triangle order -- the reference's ordered
//        z-buffer (`>=` for colour, `>` for shadow marks, :574/:668) with
//        depth/shadow/shade state held in registers; PixelShader +
//        calculateIllumination (:559-586, :664-688), deferred to the winner.
//   4. rast_post_kernel    (one thread per pixel)
//        the in-place raster-order post-pass (:283-307): a pixel's up/left
//        neighbours are seen darkened and down/right ones not, which is
//        recomputed per pixel from the shadow buffer, then antiAliasing
//        (:1736-1753) and PutPixelSDL.  Border pixels stay 0x00000000.
//        rast_post_f32_kernel (CG_PIX_RGBA_F32, cg_rast_draw_picture*): the same
//        text storing the float value PutPixelSDL would have been given.
#include <float.h>
#include <limits.h>

#include "cg_host.h"
#include "cg_rast_dev.h"

namespace cg {

constexpr int kSetupPreChunks = 16;  // input triangles counted in one round trip: < 64 * 16

__device__ void rast_setup_one(const cg_rtri &T, const RastArgs &A, RastSpan *__restrict__ spans,
                               RastHdr *__restrict__ hdr, int *__restrict__ first_tri, int t,
                               unsigned long long *lkey, unsigned long long *rkey, unsigned long long &fkey);

// One workgroup per clipped triangle (grid-stride).  With the device
// geometry (stage != null) the clipped list is compacted here: the count
// prefix of the n_in input triangles (LDS) locates clipped triangle t among
// the staged survivors, the workgroup copies it to tris[t] for the later
// kernels, and workgroup 0 stores the total at n_dev.
__global__ __launch_bounds__(kSetupThreads) void rast_setup_kernel(
    cg_rtri *__restrict__ tris, RastArgs A, int *__restrict__ n_dev, RastSpan *__restrict__ spans,
    RastHdr *__restrict__ hdr, int *__restrict__ first_tri, const cg_rtri *__restrict__ stage,
    const int *__restrict__ counts, int n_in)
{
    extern __shared__ unsigned long long s_keys[];          // [2 * H]: left | right keys per row; then [n_in + 1] ints
    __shared__ unsigned long long fkey;
    __shared__ int s_carry;
    unsigned long long *lkey = s_keys, *rkey = s_keys + A.H;
    int *s_pre = (int *)(s_keys + 2 * A.H);
    int n = A.n;
    if (stage) {
        if (n_in < 64 * kSetupPreChunks) {
            // exclusive prefix of the counts: every count loaded at once (one round trip, all
            // threads), each wave scans its 64-count chunks, then thread 0 offsets the chunks
            __shared__ int s_tot[kSetupPreChunks];
            constexpr int kQ = kSetupPreChunks / (kSetupThreads / 64);
            const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
            int cnt[kQ];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const int i = (q * (kSetupThreads / 64) + w) * 64 + lane;
                cnt[q] = i < n_in ? counts[i] : 0;
            }
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const int ch = q * (kSetupThreads / 64) + w, i = ch * 64 + lane;
                int x = cnt[q];
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(x, o);
                    if (lane >= o) x += y;
                }
                if (i <= n_in) s_pre[i] = x - cnt[q];   // exclusive within the chunk (s_pre[n_in]: its total)
                if (lane == 63) s_tot[ch] = x;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int a = 0;
                for (int ch = 0; ch * 64 <= n_in; ++ch) {
                    const int t = s_tot[ch];
                    s_tot[ch] = a;
                    a += t;
                }
                s_carry = a;
            }
            __syncthreads();
            for (int i = threadIdx.x; i <= n_in; i += kSetupThreads) s_pre[i] += s_tot[i / 64];
        } else if (threadIdx.x < 64) {                     // wave 0: exclusive prefix of the counts
            const int lane = threadIdx.x;
            int carry = 0;
            for (int i0 = 0; i0 < n_in; i0 += 64) {
                const int c = i0 + lane < n_in ? counts[i0 + lane] : 0;
                int x = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(x, o);
                    if (lane >= o) x += y;
                }
                if (i0 + lane < n_in) s_pre[i0 + lane] = carry + x - c;
                carry += __shfl(x, 63);
            }
            if (lane == 0) {
                s_pre[n_in] = carry;
                s_carry = carry;
            }
        }
        __syncthreads();
        n = min(s_carry, A.n);
        if (blockIdx.x == 0 && threadIdx.x == 0) *n_dev = n;
    } else if (n_dev) {
        n = min(*n_dev, A.n);
    }
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        cg_rtri T;
        if (stage) {
            int lo = 0, hi = n_in - 1;                     // the input triangle whose survivors hold t
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_pre[mid] <= t) lo = mid;
                else hi = mid - 1;
            }
            T = stage[(size_t)lo * kGeomMaxLeaves + (t - s_pre[lo])];
            if (threadIdx.x == 0) tris[t] = T;
        } else {
            T = tris[t];
        }
        rast_setup_one(T, A, spans, hdr, first_tri, t, lkey, rkey, fkey);
        __syncthreads();
    }
}

__device__ void rast_setup_one(const cg_rtri &T, const RastArgs &A, RastSpan *__restrict__ spans,
                               RastHdr *__restrict__ hdr, int *__restrict__ first_tri, int t,
                               unsigned long long *lkey, unsigned long long *rkey, unsigned long long &fkey)
{
    Pix vp[3] = {vertex_shader(A, T.v0), vertex_shader(A, T.v1), vertex_shader(A, T.v2)};
    int mx = -INT_MAX, mn = INT_MAX;                        // :434-447
    for (int i = 0; i < 3; ++i) {
        if (vp[i].y > mx) mx = vp[i].y;
        if (vp[i].y < mn) mn = vp[i].y;
    }
    long long rows = (long long)mx - (long long)mn + 1;     // :448
    int ylo = mn > 0 ? mn : 0;
    int yhi = mx < A.H - 1 ? mx : A.H - 1;
    RastHdr h;
    h.ylo = ylo;
    h.yhi = yhi;
    h.fy = INT_MAX;
    h.fx = INT_MAX;
    h.t_sh = (unsigned)t | (T.color.x >= 0 ? 0u : 0x80000000u);
    h.tex = T.texture;
    h.index = T.index;
    h.pad = 0;
    if (rows <= 0 || ylo > yhi) {
        if (threadIdx.x == 0) {
            h.ylo = 1;
            h.yhi = 0;
            hdr[t] = h;
        }
        return;
    }
    const int nv = yhi - ylo + 1;
    for (int k = threadIdx.x; k < nv; k += kSetupThreads) {
        lkey[k] = ~0ull;
        rkey[k] = 0ull;
    }
    if (threadIdx.x == 0) fkey = ~0ull;
    __syncthreads();
    // the three edges' Interpolate set-up (:524-538), shared by both passes
    const Edge E0 = make_edge(vp[0], vp[1]), E1 = make_edge(vp[1], vp[2]), E2 = make_edge(vp[2], vp[0]);
    // Edge samples -> rows (:466-497).  Rows outside the screen never shade.
    for (int ei = 0; ei < 3; ++ei) {
        const Edge &e = ei == 0 ? E0 : ei == 1 ? E1 : E2;
        // Only a sample that can still win its row issues an LDS atomic: the
        // left winner is the minimum x with the latest sequence among equals,
        // so a sample whose previous same-row neighbour has a smaller x, or
        // whose next same-row neighbour has a smaller-or-equal x, cannot win
        // (mirror for the right).  Exact for any order; a near-horizontal
        // edge then issues a few atomics per wave instead of 64 on one row.
        const int lane = threadIdx.x & 63;
        for (int jb = 0; jb < e.n; jb += kSetupThreads) {
            const int j = jb + (int)threadIdx.x;
            const bool in = j < e.n;
            int y = in ? edge_y(e, j) : INT_MIN;
            const bool vis = in && y >= ylo && y <= yhi;   // also covers :485's y - min >= 0
            if (!vis) y = INT_MIN + 1 + lane;              // never equals a real row
            const int x = vis ? edge_x(e, j) : 0;
            const int yp = __shfl_up(y, 1, 64), xp = __shfl_up(x, 1, 64);
            const int yn = __shfl_down(y, 1, 64), xn = __shfl_down(x, 1, 64);
            const bool hp = lane > 0 && yp == y, hn = lane < 63 && yn == y;
            if (vis) {
                const unsigned seq = ((unsigned)ei << 30) | (unsigned)j;
                if (!(hp && xp < x) && !(hn && xn <= x)) atomicMin(&lkey[y - ylo], key_left(x, seq));
                if (!(hp && xp > x) && !(hn && xn >= x)) atomicMax(&rkey[y - ylo], key_right(x, seq));
            }
        }
    }
    __syncthreads();
    const bool shade_tri = A.want_first && T.color.x >= 0;
    for (int k = threadIdx.x; k < nv; k += kSetupThreads) {
        RastSpan s;
        unsigned long long lk = lkey[k], rk = rkey[k];
        if (lk == ~0ull) {                                  // untouched row: shades nothing
            s.lx = 1; s.rx = 0;
            s.lz = s.sz = s.lX = s.sX = s.lY = s.sY = 0.f;
        } else {
            unsigned ls = ~(unsigned)(lk & 0xffffffffu), rs = (unsigned)(rk & 0xffffffffu);
            int le = (int)(ls >> 30), lj = (int)(ls & 0x3fffffffu);
            int re = (int)(rs >> 30), rj = (int)(rs & 0x3fffffffu);
            const Edge el = le == 0 ? E0 : le == 1 ? E1 : E2;
            const Edge er = re == 0 ? E0 : re == 1 ? E1 : E2;
            int lx = edge_x(el, lj), rx = edge_x(er, rj);
            float lz, lX, lY, rz, rX, rY;
            edge_attr(el, lj, lz, lX, lY);
            edge_attr(er, rj, rz, rX, rY);
            // DrawPolygonRows' Interpolate(left, right, N = rx - lx + 1) (:502-503, :524-538)
            long long span = (long long)rx - (long long)lx;
            if (span < 0 || span > (1 << 24)) {              // reference would not survive this row
                s.lx = 1; s.rx = 0;
                s.lz = s.sz = s.lX = s.sX = s.lY = s.sY = 0.f;
            } else {
                int N = (int)span + 1;
                float den = (float)(N - 1 > 1 ? N - 1 : 1);
                float aX = lX * lz, aY = lY * lz, bX = rX * rz, bY = rY * rz;
                s.lx = lx;
                s.rx = rx;
                s.lz = lz;
                s.sz = (rz - lz) / den;
                s.lX = aX;
                s.sX = (bX - aX) / den;
                s.lY = aY;
                s.sY = (bY - aY) / den;
                if (shade_tri) {
                    // first fragment of this row that PixelShader would shade on an empty z-buffer
                    int y = ylo + k;
                    for (int i = 0; i < N - 1; ++i) {
                        int x = lx + i;
                        if (x >= A.W) break;
                        if (x < 0) continue;
                        float zi = s.lz + (s.sz * (float)i);
                        // on an empty z-buffer a fragment shades unless it is a
                        // transparent texel of texture 2/3 (:602, :624)
                        if (zi >= 0.0f && (!A.textured || rast_opaque(A, T.texture, T.index, zi,
                                                                     s.lX + (s.sX * (float)i),
                                                                     s.lY + (s.sY * (float)i)))) {
                            atomicMin(&fkey, ((unsigned long long)(unsigned)y << 32) | (unsigned)x);
                            break;
                        }
                    }
                }
            }
        }
        spans[(size_t)(ylo + k) * A.n + t] = s;              // row-major: a row's spans are contiguous
    }
    if (shade_tri) {
        __syncthreads();
        if (threadIdx.x == 0 && fkey != ~0ull) {
            h.fy = (int)(fkey >> 32);
            h.fx = (int)(fkey & 0xffffffffu);
            atomicMin(first_tri, t);
        }
    }
    if (threadIdx.x == 0) hdr[t] = h;
}


// A wave per row: the records of the row's covering triangles in triangle
// order.  The headers of a group of 64 * kRowBatches triangles are loaded in
// one round trip (beside the triangle count), then the spans of those that
// cover the row, then the ballot compaction -- two dependent round trips per
// group instead of three per 64 triangles.
constexpr int kRowBatches = 8;
__global__ __launch_bounds__(256) void rast_rows_kernel(const cg_rtri *__restrict__ tris, RastArgs A,
                                                       const int *__restrict__ n_dev,
                                                       const RastSpan *__restrict__ spans,
                                                       const RastHdr *__restrict__ hdr,
                                                       const int *__restrict__ first_tri,
                                                       RowRec *__restrict__ recs, int *__restrict__ count)
{
    int m;
    const int g = xcd_group(A.H, kXcdRows / 4, m);
    if (g < 0) return;
    const int y = g * kXcdRows + m * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (y >= A.H) return;
    const int ft = A.want_first ? *first_tri : INT_MAX;
    const int n = n_dev ? min(*n_dev, A.n) : A.n;
    int c = 0;
    for (int g0 = 0; g0 == 0 || g0 < n; g0 += 64 * kRowBatches) {
        RastHdr h[kRowBatches];
#pragma unroll
        for (int j = 0; j < kRowBatches; ++j) {   // in flight together (t < A.n: a valid header slot)
            const int t = g0 + 64 * j + lane;
            if (t < A.n) h[j] = hdr[t];
        }
        RastSpan sp[kRowBatches];
        bool keep[kRowBatches];
#pragma unroll
        for (int j = 0; j < kRowBatches; ++j) {
            const int t = g0 + 64 * j + lane;
            keep[j] = t < n && h[j].ylo <= y && y <= h[j].yhi;
            if (keep[j]) sp[j] = spans[(size_t)y * A.n + t];
        }
#pragma unroll
        for (int j = 0; j < kRowBatches; ++j) {
            const int t = g0 + 64 * j + lane;
            // fragments x in [lx, rx - 1] (:504) intersecting [0, W)
            const bool k = keep[j] && sp[j].rx > sp[j].lx && sp[j].rx - 1 >= 0 && sp[j].lx <= A.W - 1;
            const unsigned long long mk = __ballot(k);
            if (k) {
                RowRec r;
                r.lx = sp[j].lx; r.rx = sp[j].rx;
                r.lz = sp[j].lz; r.sz = sp[j].sz; r.lX = sp[j].lX; r.sX = sp[j].sX; r.lY = sp[j].lY; r.sY = sp[j].sY;
                r.t_sh = h[j].t_sh;
                r.first_x = (t == ft && h[j].fy == y) ? h[j].fx : -1;
                r.tex = h[j].tex; r.index = h[j].index;
                recs[(size_t)y * A.n + c + __popcll(mk & ((1ull << lane) - 1ull))] = r;
            }
            c += __popcll(mk);
        }
    }
    if (lane == 0) count[y] = c;
}

// TEX: texture modes 1-3 possible (A.textured): a fragment of texture 2/3
// that passes the depth test but hits a transparent texel sets the depth to 0
// and shades nothing (:619, :643, :665) -- decided in the ordered walk.
template <bool TEX>
__global__ __launch_bounds__(256) void rast_fill_kernel(RastArgs A, const RowRec *__restrict__ recs,
                                                       const int *__restrict__ count, uint32_t *__restrict__ state,
                                                       float *__restrict__ depth_out, int32_t *__restrict__ shadow_out)
{
    const int segs = (A.W + kFillPx - 1) / kFillPx;
    // wave-uniform by construction; readfirstlane lets the compiler keep the
    // record walk on the scalar unit (uniform branches)
    int m;
    const int g = xcd_group(A.H, (segs * kXcdRows + 3) / 4, m);
    if (g < 0) return;
    const int unit = m * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (row, segment) in the group
    const int lane = threadIdx.x & 63;
    const int y = g * kXcdRows + unit / segs;
    if (unit >= segs * kXcdRows || y >= A.H) return;
    const int x0 = (unit % segs) * kFillPx;
    const int x = x0 + lane;
    float depth = 0.0f;                                   // :247
    int shadow = 0, win = -1;                             // :259; record of the last shading fragment
    const int cnt = count[y];
    const RowRec *rr = recs + (size_t)y * A.n;
    // 64 records per round trip: lane q loads record base+q (coalesced), a
    // ballot keeps those with a fragment in this segment, and the set bits are
    // walked in ascending order (= triangle order) with readlane broadcasts.
    for (int base = 0; base < cnt; base += 64) {
        const int q = base + lane;
        int mlx = 0, mrx = 0, msh = 0, mtex = 0, midx = 0;
        float mlz = 0.f, msz = 0.f, mlX = 0.f, msX = 0.f, mlY = 0.f, msY = 0.f;
        if (q < cnt) {
            const RowRec &mr = rr[q];
            mlx = mr.lx; mrx = mr.rx; mlz = mr.lz; msz = mr.sz; msh = rec_shadow(mr);
            if (TEX) {
                mtex = mr.tex; midx = mr.index;
                mlX = mr.lX; msX = mr.sX; mlY = mr.lY; msY = mr.sY;
            }
        }
        const bool ov = q < cnt && !(mrx - 1 < x0 || mlx > x0 + kFillPx - 1);
        unsigned long long m = __ballot(ov);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1ull;
            const int lx = __builtin_amdgcn_readlane(mlx, b);
            const int rx = __builtin_amdgcn_readlane(mrx, b);
            const float lz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mlz), b));
            const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(msz), b));
            const int shd = __builtin_amdgcn_readlane(msh, b);
            // every readlane sits here, where the whole wave is active: lane b
            // holds the record, and a readlane under a per-lane condition below
            // would read a register the compiler may have split under EXEC
            int tex = 0, idx = 0;
            float lX = 0.f, sX = 0.f, lY = 0.f, sY = 0.f;
            if (TEX) {
                tex = __builtin_amdgcn_readlane(mtex, b);
                idx = __builtin_amdgcn_readlane(midx, b);
                lX = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mlX), b));
                sX = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(msX), b));
                lY = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mlY), b));
                sY = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(msY), b));
            }
            const int i = x - lx;
            if (!(x < A.W && i >= 0 && x < rx)) continue;          // :504, :573
            const float zinv = lz + (sz * (float)i);               // :543
            if (!shd) {
                if (zinv >= depth) {                               // :574
                    bool opaque = true;
                    if (TEX && tex >= 2)                           // opacity-tested textures
                        opaque = rast_opaque(A, tex, idx, zinv, lX + (sX * (float)i), lY + (sY * (float)i));
                    if (opaque) {
                        depth = zinv;                              // :665
                        win = base + b;
                    } else {
                        depth = 0.0f;                              // p.zinv = 0 (:619, :643), :665
                    }
                }
            } else if (zinv > depth) {                             // :668-669
                shadow = 1;
            }
        }
    }
    if (x < A.W) {
        const size_t o = (size_t)y * A.W + x;
        if (A.state16) ((uint16_t *)state)[o] = (uint16_t)((win + 1) | (shadow ? 0x8000 : 0));
        else state[o] = (uint32_t)(win + 1) | (shadow ? kStShadow : 0u);
        if (depth_out) depth_out[o] = depth;
        if (shadow_out) shadow_out[o] = shadow;
    }
}

// Post-pass (:283-307) on a 64x8 tile: the shadow marks (halo 2) go to LDS,
// then every pixel of the tile and its 1-pixel halo gets its three shade
// buffers and its darkening computed once, then each interior pixel runs
// antiAliasing (:1736-1753) on its 5 taps from LDS.  Raster order: the pixel
// itself and its up/left neighbours are seen darkened, down/right not (a
// darkening of 0 subtracts exactly nothing).  DIRECT (colour modes 1-2): the
// state is the colour fill's float4 (cg_rast_colour.hip) instead of the fill's
// record word, and the shadow marks come from the shadow plane; skip (may be
// null): a sequence frame's status word, non-zero = the frame is not drawn.
// The text is cg_rast_post_kernel.inc, once per output policy: rast_post_kernel stores PutPixelSDL's
// word, rast_post_f32_kernel (CG_PIX_RGBA_F32) the float4 it would have been given.
#define CG_RAST_POST_NAME rast_post_kernel
#define CG_RAST_POST_F32 0
#define CG_RAST_POST_OUT uint32_t
#include "cg_rast_post_kernel.inc"
#undef CG_RAST_POST_NAME
#undef CG_RAST_POST_F32
#undef CG_RAST_POST_OUT
#define CG_RAST_POST_NAME rast_post_f32_kernel
#define CG_RAST_POST_F32 1
#define CG_RAST_POST_OUT float4
#include "cg_rast_post_kernel.inc"
#undef CG_RAST_POST_NAME
#undef CG_RAST_POST_F32
#undef CG_RAST_POST_OUT

// The colour modes' post-pass over a float4 state and a shadow plane, for the compact route's
// modes 1-2 (cg_rast_big.hip): the launch below, without a status word.  pix: d_argb's pixel format
// (CG_PIX_RGBA_F32: it holds float4 pixels and the float-storing kernel runs).
void launch_rast_post_direct(const RastArgs &A, const float4 *state, const int32_t *shadow, uint32_t *d_argb,
                             hipStream_t st, int pix)
{
    if (pix == CG_PIX_RGBA_F32) {
        hipLaunchKernelGGL((rast_post_f32_kernel<true, false>), dim3(xcd_grid(A.H, (A.W + kPostTW - 1) / kPostTW)),
                           dim3(256), 0, st, A.tris, A, (const void *)state, (const RowRec *)nullptr, shadow,
                           (float4 *)d_argb, (const int32_t *)nullptr);
        return;
    }
    hipLaunchKernelGGL((rast_post_kernel<true, false>), dim3(xcd_grid(A.H, (A.W + kPostTW - 1) / kPostTW)), dim3(256), 0,
                       st, A.tris, A, (const void *)state, (const RowRec *)nullptr, shadow, d_argb,
                       (const int32_t *)nullptr);
}

// The fill + post pipeline.  Either the triangle count is known on the host
// (n_dev == nullptr, n = count) or it lives on the device (n_dev, n = capacity,
// light read from d_light).
// Staged survivors of the device clip (rast_draw_device): the setup compacts them.
struct RastStage {
    const cg_rtri *stage;   // null: d_tris is already the list
    const int *counts;
    int n_in;
};
static int rast_pipeline(cg_ctx *c, cg_rtri *d_tris, int n, int *n_dev, const cg_rast_params *p,
                         cg_vec4 light, const cg_vec4 *d_light, uint32_t *d_argb, float *d_depth,
                         int32_t *d_shadow, hipStream_t st, cg_stats *stats, bool events_open, int tex_mask,
                         RastStage sg, const RastSeq *seq = nullptr, int pix = CG_PIX_ARGB8888);

// glm::inverse for mat4 (glm/detail/type_mat4x4.inl:37-90), column-major
// m[4c + r] = m[c][r]: findU / findV's inverse(R) (skeleton.cpp:1762).
static void mat4_inverse_glm(const float *m, float *out)
{
    auto M = [m](int c, int r) { return m[4 * c + r]; };
    const float c00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3), c02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3);
    const float c03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3);
    const float c04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3), c06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3);
    const float c07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3);
    const float c08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2), c10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2);
    const float c11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2);
    const float c12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3), c14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3);
    const float c15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3);
    const float c16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2), c18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2);
    const float c19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2);
    const float c20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1), c22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1);
    const float c23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
    const float fac[6][4] = {{c00, c00, c02, c03}, {c04, c04, c06, c07}, {c08, c08, c10, c11},
                             {c12, c12, c14, c15}, {c16, c16, c18, c19}, {c20, c20, c22, c23}};
    const float vec[4][4] = {{M(1, 0), M(0, 0), M(0, 0), M(0, 0)}, {M(1, 1), M(0, 1), M(0, 1), M(0, 1)},
                             {M(1, 2), M(0, 2), M(0, 2), M(0, 2)}, {M(1, 3), M(0, 3), M(0, 3), M(0, 3)}};
    float inv[4][4];
    for (int k = 0; k < 4; ++k) {
        const float sa = (k & 1) ? -1.0f : 1.0f, sb = -sa;   // SignA (+,-,+,-), SignB (-,+,-,+)
        inv[0][k] = ((vec[1][k] * fac[0][k] - vec[2][k] * fac[1][k]) + vec[3][k] * fac[2][k]) * sa;
        inv[1][k] = ((vec[0][k] * fac[0][k] - vec[2][k] * fac[3][k]) + vec[3][k] * fac[4][k]) * sb;
        inv[2][k] = ((vec[0][k] * fac[1][k] - vec[1][k] * fac[3][k]) + vec[3][k] * fac[5][k]) * sa;
        inv[3][k] = ((vec[0][k] * fac[2][k] - vec[1][k] * fac[4][k]) + vec[2][k] * fac[5][k]) * sb;
    }
    const float d0 = M(0, 0) * inv[0][0], d1 = M(0, 1) * inv[1][0], d2 = M(0, 2) * inv[2][0],
                d3 = M(0, 3) * inv[3][0];
    const float one_over = 1.0f / ((d0 + d1) + (d2 + d3));
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) out[4 * c + r] = inv[c][r] * one_over;
}

// The kernels' frame arguments from the caller's parameters (both routes); state16 is the
// route's own decision.  Fails for a texture the frame cannot render.
int rast_make_args(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light,
                   const cg_vec4 *d_light, int tex_mask, RastArgs *out)
{
    const int W = p->width, H = p->height;
    RastArgs A;
    A.W = W;
    A.H = H;
    A.n = n;
    A.focal = p->focal;
    A.light[0] = light.x; A.light[1] = light.y; A.light[2] = light.z;
    A.lp[0] = p->light_power.x; A.lp[1] = p->light_power.y; A.lp[2] = p->light_power.z;
    A.ind_first = p->indirect_first;
    A.want_first = p->colour_mode == 0 && p->indirect_first != 0.2f * 1;   // the :585 rewrite is mode 0 only
    A.d_light = d_light;
    // texture modes 1-3: the maps, cameraPos and, when yaw != 0, inverse(R)
    const int loaded = rast_tex_maps(c, &A.tx);
    if (tex_mask & 16) return ctx_invalid(c, "texture selector outside 0-3 (TestModelH.h:21)");
    if (tex_mask & ~loaded & 0xe)
        return ctx_invalid(c, "a triangle carries a texture whose maps are not loaded (cg_rast_set_textures)");
    if ((tex_mask & 2) && (size_t)(H - 1) * kMarbleN + (W - 1) >= (size_t)kMarbleN * kMarbleN)
        return ctx_invalid(c, "marble: normalMap_marble[y * 2000 + x] would index past the map");
    A.textured = (tex_mask & 0xe) != 0;
    A.use_inv = p->yaw != 0.0f;
    A.state16 = 0;
    A.tris = d_tris;
    A.cam[0] = p->camera.x; A.cam[1] = p->camera.y; A.cam[2] = p->camera.z; A.cam[3] = p->camera.w;
    mat4_inverse_glm(p->R, A.Rinv);
    *out = A;
    return CG_OK;
}

int rast_render_device(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light,
                       uint32_t *d_argb, float *d_depth, int32_t *d_shadow, hipStream_t st,
                       cg_stats *stats, int tex_mask)
{
    if (ctx_rast_route(c, n, p->colour_mode != 0) == CG_RAST_ROUTE_COMPACT)
        return rast_big_render(c, d_tris, n, p, light, d_argb, d_depth, d_shadow, st, stats, tex_mask);
    return rast_pipeline(c, const_cast<cg_rtri *>(d_tris), n, nullptr, p, light, nullptr, d_argb, d_depth, d_shadow,
                         st, stats, false, tex_mask, RastStage{nullptr, nullptr, 0});
}

// Whole rasteriser Draw on the device: geometry (shadow volumes + clip) then
// fill + post.  room/boxes are device pointers (cg_rast_set_scene).  seq: the
// frame belongs to a sequence (cg_rast_draw_sequence_device).  pix: the pixel
// format of d_argb -- CG_PIX_RGBA_F32: W * H float4, stored by the post-pass's
// float kernels; every other launch of the frame is the same.
int rast_draw_device(cg_ctx *c, const cg_rtri *d_room, int n_room, const cg_rtri *d_boxes, int n_boxes,
                     const cg_rast_params *p, uint32_t *d_argb, float *d_depth, int32_t *d_shadow,
                     hipStream_t st, cg_stats *stats, int **n_out, int tex_mask, const RastSeq *seq, int pix)
{
    if (p->width <= 2 || p->height <= 2 || p->height > kRastMaxRows || p->focal == 0.0f) return CG_E_INVALID;
    if (pix != CG_PIX_ARGB8888 && pix != CG_PIX_RGBA_F32) return CG_E_INVALID;
    const long long n_in_ll = (long long)n_room + 7ll * n_boxes;
    // a sequence's frames all take the route the call chose (its lanes and tables follow it)
    const int route = seq ? seq->route : ctx_rast_route(c, kGeomMaxLeaves * n_in_ll, p->colour_mode != 0);
    if (route == CG_RAST_ROUTE_COMPACT)
        return rast_big_draw(c, d_room, n_room, d_boxes, n_boxes, p, d_argb, d_depth, d_shadow, st, stats, n_out,
                             tex_mask, seq, pix);
    if (n_in_ll > kRastDenseInputs)
        return ctx_invalid(c, "dense route: more than 4096 input triangles (the setup's LDS prefix); "
                              "use the compact route (cg_rast_set_route)");
    const int n_in = (int)n_in_ll;
    // planes 1-4 and 6 can each split a triangle in two; plane 5 never does
    const int cap = n_in > 0 ? 32 * n_in : 1;
    hipError_t e;
    // the clipped list, then each input triangle's staged survivors (32 each)
    cg_rtri *tris = (cg_rtri *)ctx_buf(c, kBufTris, ((size_t)cap + 32 * (size_t)n_in) * sizeof(cg_rtri), &e);
    if (!tris) return ctx_fail(c, e, "alloc clipped triangles");
    int *geo = (int *)ctx_buf(c, kBufGeo, 64 + 4 * (size_t)n_in, &e);   // [0] count, [4..7] light, [16..] counts
    if (!geo) return ctx_fail(c, e, "alloc geometry header");
    int *misc = (int *)ctx_buf(c, kBufCount, ((size_t)p->height + 16) * sizeof(int), &e);   // count[H] | first_tri
    if (!misc) return ctx_fail(c, e, "alloc counts");
    hipEvent_t e0, e1;
    ctx_events(c, &e0, &e1);
    if (stats && (e = hipEventRecord(e0, st)) != hipSuccess) return ctx_fail(c, e, "event");
    if ((e = launch_rast_clip(*p, d_room, n_room, d_boxes, n_boxes, tris + cap, geo + 16, (cg_vec4 *)(geo + 4),
                              misc + p->height, st)) != hipSuccess)
        return ctx_fail(c, e, "rast_clip launch");
    if (n_out) *n_out = geo;
    return rast_pipeline(c, tris, cap, geo, p, cg_vec4{0, 0, 0, 1}, (const cg_vec4 *)(geo + 4), d_argb, d_depth,
                         d_shadow, st, stats, true, tex_mask, RastStage{tris + cap, geo + 16, n_in}, seq, pix);
}

static int rast_pipeline(cg_ctx *c, cg_rtri *d_tris, int n, int *n_dev, const cg_rast_params *p,
                         cg_vec4 light, const cg_vec4 *d_light, uint32_t *d_argb, float *d_depth,
                         int32_t *d_shadow, hipStream_t st, cg_stats *stats, bool events_open, int tex_mask,
                         RastStage sg, const RastSeq *seq, int pix)
{
    if (p->width <= 2 || p->height <= 2 || p->height > kRastMaxRows) return CG_E_INVALID;
    const int W = p->width, H = p->height;
    const size_t npx = (size_t)W * H;
    const int nn = n > 0 ? n : 1;
    if (p->colour_mode != 0 && nn > kRastDenseColourList)   // reached only on a forced dense route or a route limit
        return ctx_invalid(c, "dense route: colour modes 1-2 count fragments per list slot in LDS, at most 20480 "
                              "slots (32 an input triangle); the automatic route takes the compact route there");
    hipError_t e;
    RastSpan *spans = (RastSpan *)ctx_buf(c, kBufSpan, (size_t)nn * H * sizeof(RastSpan), &e);
    if (!spans) return ctx_fail(c, e, "alloc spans");
    RastHdr *hdr = (RastHdr *)ctx_buf(c, kBufHdr, (size_t)nn * sizeof(RastHdr), &e);
    if (!hdr) return ctx_fail(c, e, "alloc hdr");
    // fill -> post state: 4 B/pixel in colour mode 0, the colour fill's 16 B in modes 1-2
    void *state = ctx_buf(c, kBufPix, npx * (p->colour_mode == 0 ? sizeof(uint32_t) : sizeof(float4)), &e);
    if (!state) return ctx_fail(c, e, "alloc state");
    int *misc = (int *)ctx_buf(c, kBufCount, ((size_t)H + 16) * sizeof(int), &e);   // count[H] | first_tri
    if (!misc) return ctx_fail(c, e, "alloc counts");
    int *count = misc, *first_tri = misc + H;
    RowRec *recs = (RowRec *)ctx_buf(c, kBufRecs, (size_t)H * nn * sizeof(RowRec), &e);
    if (!recs) return ctx_fail(c, e, "alloc row records");
    int32_t *shadow = d_shadow;   // mode 0 carries the marks in the state; modes 1-2 need the plane
    if (!shadow && p->colour_mode != 0) {
        shadow = (int32_t *)ctx_buf(c, kBufShadow, npx * sizeof(int32_t), &e);
        if (!shadow) return ctx_fail(c, e, "alloc shadow");
    }
    RastArgs A;
    if (const int rc = rast_make_args(c, d_tris, n, p, light, d_light, tex_mask, &A)) return rc;
    A.state16 = p->colour_mode == 0 && nn < 32768;
    hipEvent_t e0, e1;
    ctx_events(c, &e0, &e1);
    if (stats && !events_open && (e = hipEventRecord(e0, st)) != hipSuccess) return ctx_fail(c, e, "event");
    // the device clip initialises the first-fragment minimum (rast_clip_kernel)
    if (A.want_first && !(sg.stage && sg.n_in > 0) && (e = hipMemsetAsync(first_tri, 0x7f, sizeof(int), st)) != hipSuccess)
        return ctx_fail(c, e, "memset");
    if (n > 0) {
        const int grid = n < 1024 ? n : 1024;                // LDS 16 B per row: several workgroups per CU
        hipLaunchKernelGGL(rast_setup_kernel, dim3(grid), dim3(kSetupThreads),
                           2 * (size_t)H * 8 + ((size_t)sg.n_in + 1) * 4, st, d_tris, A, n_dev, spans, hdr, first_tri,
                           sg.stage, sg.counts, sg.n_in);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_setup launch");
    }
    hipLaunchKernelGGL(rast_rows_kernel, dim3(xcd_grid(H, kXcdRows / 4)), dim3(256), 0, st, d_tris, A, n_dev, spans, hdr,
                       first_tri, recs, count);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_rows launch");
    const int post_grid = xcd_grid(H, (W + kPostTW - 1) / kPostTW);
    void *words = state;   // the ordered z-buffer's state words (RastFrame)
    if (p->colour_mode != 0) {
        long long ns = -1;
        const int rc = seq ? rast_seq_colour_fill(c, A, p, recs, count, hdr, n_dev, nn, (float4 *)state, d_depth,
                                                  shadow, st, *seq)
                           : rast_colour_fill(c, A, p, recs, count, hdr, n_dev, nn, (float4 *)state, d_depth, shadow,
                                              st, &ns);
        if (rc) return rc;
        if (stats) stats->n_shaded = ns;
        if (!d_argb) {
            // null: a buffers call that asks for no picture
        } else if (pix == CG_PIX_RGBA_F32)
            hipLaunchKernelGGL((rast_post_f32_kernel<true, false>), dim3(post_grid), dim3(256), 0, st, d_tris, A,
                               (const void *)state, (const RowRec *)recs, shadow, (float4 *)d_argb,
                               seq ? (const int32_t *)&seq->info->status : (const int32_t *)nullptr);
        else
            hipLaunchKernelGGL((rast_post_kernel<true, false>), dim3(post_grid), dim3(256), 0, st, d_tris, A,
                               (const void *)state, (const RowRec *)recs, shadow, d_argb,
                               seq ? (const int32_t *)&seq->info->status : (const int32_t *)nullptr);
        if (ctx_rast_want_owner(c)) {
            // the owner of a pixel is the ordered z-buffer's last writer whatever the colour mode
            // (modes 1-2 ignore textures, :604): the mode-0 fill's walk into words of its own
            words = ctx_buf(c, kBufOwner, npx * sizeof(uint32_t), &e);
            if (!words) return ctx_fail(c, e, "alloc owner state");
            A.state16 = nn < 32768;
            const int fgrid = xcd_grid(H, ((W + kFillPx - 1) / kFillPx * kXcdRows + 3) / 4);
            hipLaunchKernelGGL(rast_fill_kernel<false>, dim3(fgrid), dim3(256), 0, st, A, (const RowRec *)recs,
                               (const int *)count, (uint32_t *)words, (float *)nullptr, (int32_t *)nullptr);
        }
    } else {
        const int fgrid = xcd_grid(H, ((W + kFillPx - 1) / kFillPx * kXcdRows + 3) / 4);
        {
            const int kt_id = KT_RAST_FILL;
            if (A.textured)
                kt_launch(kt_id, rast_fill_kernel<true>, dim3(fgrid), dim3(256), 0, st, A, recs, count,
                                   (uint32_t *)state, d_depth, d_shadow);
            else
                kt_launch(kt_id, rast_fill_kernel<false>, dim3(fgrid), dim3(256), 0, st, A, recs, count,
                                   (uint32_t *)state, d_depth, d_shadow);
        }
        const int kt_id = KT_RAST_POST;
        if (!d_argb) {
            // a buffers call that asks for no picture
        } else if (pix == CG_PIX_RGBA_F32) {
            if (A.textured)
                kt_launch(kt_id, (rast_post_f32_kernel<false, true>), dim3(post_grid), dim3(256), 0, st, d_tris, A,
                          (const void *)state, (const RowRec *)recs, (const int32_t *)nullptr, (float4 *)d_argb,
                          (const int32_t *)nullptr);
            else
                kt_launch(kt_id, (rast_post_f32_kernel<false, false>), dim3(post_grid), dim3(256), 0, st, d_tris, A,
                          (const void *)state, (const RowRec *)recs, (const int32_t *)nullptr, (float4 *)d_argb,
                          (const int32_t *)nullptr);
        } else if (A.textured)
            kt_launch(kt_id, (rast_post_kernel<false, true>), dim3(post_grid), dim3(256), 0, st, d_tris, A,
                               (const void *)state, (const RowRec *)recs, (const int32_t *)nullptr, d_argb,
                               (const int32_t *)nullptr);
        else
            kt_launch(kt_id, (rast_post_kernel<false, false>), dim3(post_grid), dim3(256), 0, st, d_tris, A,
                               (const void *)state, (const RowRec *)recs, (const int32_t *)nullptr, d_argb,
                               (const int32_t *)nullptr);
        if (stats) stats->n_shaded = -1;
        if (seq) {
            const int rc = rast_seq_chain_mode0(c, st, *seq);
            if (rc) return rc;
        }
    }
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_post launch");
    if (stats && (e = hipEventRecord(e1, st)) != hipSuccess) return ctx_fail(c, e, "event");
    if (stats) {
        stats->n_tris = n_dev ? -1 : n;
        stats->n_spans = 0;
    }
    *ctx_rast_last(c) = RastLast{CG_RAST_ROUTE_DENSE, n_dev ? -1ll : (long long)n, 0, -1, n_dev, count, H, st};
    RastFrame &fr = *ctx_rast_frame(c);
    fr = RastFrame{};
    fr.valid = p->colour_mode == 0 || words != state;
    fr.route = CG_RAST_ROUTE_DENSE;
    fr.mode = p->colour_mode;
    fr.A = A;
    fr.words = words;
    fr.direct = p->colour_mode != 0 ? (const float4 *)state : nullptr;
    fr.recs = recs;
    fr.rec_cap = (unsigned long long)H * (unsigned long long)nn;
    fr.counts = sg.stage ? sg.counts : nullptr;
    fr.n_in = sg.n_in;
    fr.st = st;
    return CG_OK;
}

}  // namespace cg
