// cg_rast_big.hip -- the rasteriser's compact route for large scenes (gfx950).
//
// The dense pipeline (cg_rast.hip) sizes its spans and row records at
// capacity x H and tests every header slot on every row.  This route renders
// the same Draw with scratch and work that follow what the frame covers; every
// plane is bit-identical to the dense route's (the arithmetic below is the
// dense kernels', only the addressing differs).
//
// Launches per frame, all order-exact (no atomic decides an order):
//   1. rast_clip_kernel (cg_geometry.hip, unchanged) stages each input
//      triangle's survivors; big_scan (reduce / top / apply) turns counts[n_in]
//      into offsets and rast_big_gather_kernel copies the survivors into list
//      order.  The host reads the total: the clipped list is sized by it.
//   2. rast_big_range_kernel: a triangle's visible rows from its three
//      VertexShader results (the setup's ylo / yhi); big_scan gives its span
//      offset; the host reads the span total.  rast_big_setup_kernel is
//      rast_setup_kernel's ComputePolygonRows body storing the spans at
//      span_off[t] + (y - ylo), with each span's (triangle, row) beside it.
//   3. Row lists: a stable counting sort of the spans by row.  The spans lie in
//      triangle order, so a row's records in span order are in triangle order.
//      A wave takes a chunk of kBigChunk consecutive spans and walks it
//      kBigBatch at a time with one counter per row in LDS; within a batch the
//      lanes of equal row rank themselves with ballots.  Pass 1 counts
//      (hist[chunk][row]); a scan over the chunks of each row and a scan over the
//      rows give every chunk its base in every row; the host reads the record
//      total and the longest row; pass 2 repeats the walk and stores each RowRec
//      at row_off[y] + base + rank.
//   4. rast_big_fill_kernel / rast_big_post_kernel: rast_fill_kernel / the
//      mode-0 rast_post_kernel reading recs + row_off[y].
// Colour modes 1-2 (every shaded fragment draws three rand() values, in the
// reference's fragment order: triangle by triangle, row by row, left to right)
// replace 4 by an order the layout already holds -- the spans lie in (triangle,
// row) order:
//   5. rast_big_segs_kernel: the kFillPx-pixel fill segments each span's visible
//      extent overlaps (cg_rast_span_segments; 0 for shadow volumes, which never
//      shade); big_scan gives seg_off[span]; the host reads the total N, and the
//      row-list write pass leaves seg_off[span] beside every record.
//   6. rast_big_colour_kernel<false>: the fill's walk, one wave per (row,
//      segment), with the ordered z-buffer alone; the fragments of each record
//      that pass it go to c[seg_off[span] + segment - the span's first]: one
//      writer an entry.  big_scan over c numbers them: entries lie in (triangle,
//      row, x) order, so fbase[entry] is the frame-wide number of the entry's
//      first shaded fragment and fbase[N] is S, which the host reads.
//   7. the generator of cg_rast_colour.hip makes exactly 3 S values;
//      rast_big_colour_kernel<true> repeats the walk, numbers a passing fragment
//      fbase[entry] + the passing lanes below it, and shades each pixel's last
//      winner as rast_fill_rand_kernel does; the dense rast_post_kernel<true,
//      false> finishes the frame.
// Every store is bounded by its buffer's capacity; no kernel waits on another.
#include <algorithm>

#include "cg_host.h"
#include "cg_rast_dev.h"

namespace cg {

typedef unsigned long long u64;

// Block sizes of the row-list passes (cg_rast_row_blocks): a wave ranks
// kBigBatch spans per ballot round and owns kBigChunk consecutive spans.
constexpr int kBigBatch = 64;
constexpr int kBigChunk = 2048;
static_assert(kBigChunk % kBigBatch == 0, "a chunk is whole batches");
constexpr int kRowBits = 12;
static_assert((1 << kRowBits) >= kRastMaxRows, "a row index fits the ballot rounds");

void rast_big_blocks(int *batch, int *chunk)
{
    *batch = kBigBatch;
    *chunk = kBigChunk;
}

// ---- device-wide exclusive scan: int counts -> 64-bit offsets, out[N] = total ----
constexpr int kScanThreads = 256, kScanItems = 16, kScanBlock = kScanThreads * kScanItems;

// exclusive prefix of one value per thread over the workgroup (256 threads); total: their sum
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64 *s_w, u64 &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    u64 base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) {
        if (k < w) base += s_w[k];
        total += s_w[k];
    }
    __syncthreads();   // s_w is free for the next call
    return base + x - v;
}

__global__ __launch_bounds__(kScanThreads) void rast_big_scan_reduce_kernel(const int *__restrict__ in, long long N,
                                                                            u64 *__restrict__ bsum)
{
    __shared__ u64 s_w[kScanThreads / 64];
    const long long i0 = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems;
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (i0 + k < N) s += (u64)(unsigned)max(in[i0 + k], 0);
    u64 total;
    (void)block_excl_scan(s, s_w, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: the block sums become their exclusive prefix, *total the grand total
__global__ __launch_bounds__(kScanThreads) void rast_big_scan_top_kernel(u64 *__restrict__ bsum, int nb,
                                                                         u64 *__restrict__ total_out)
{
    __shared__ u64 s_w[kScanThreads / 64];
    u64 carry = 0;
    for (int b0 = 0; b0 < nb; b0 += kScanThreads) {
        const int b = b0 + (int)threadIdx.x;
        const u64 v = b < nb ? bsum[b] : 0;
        u64 total;
        const u64 ex = block_excl_scan(v, s_w, total);
        if (b < nb) bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(kScanThreads) void rast_big_scan_apply_kernel(const int *__restrict__ in, long long N,
                                                                           const u64 *__restrict__ bsum,
                                                                           u64 *__restrict__ out)
{
    __shared__ u64 s_w[kScanThreads / 64];
    const long long i0 = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems;
    int v[kScanItems];
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = i0 + k < N ? max(in[i0 + k], 0) : 0;
        s += (u64)(unsigned)v[k];
    }
    u64 total;
    u64 run = bsum[blockIdx.x] + block_excl_scan(s, s_w, total);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (i0 + k < N) out[i0 + k] = run;
        run += (u64)(unsigned)v[k];
    }
}

// ---- 1. clipped list: the staged survivors in list order ----
__global__ __launch_bounds__(256) void rast_big_gather_kernel(const cg_rtri *__restrict__ stage,
                                                             const int *__restrict__ counts,
                                                             const u64 *__restrict__ pre, int n_in,
                                                             cg_rtri *__restrict__ tris, int n)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long i = idx / kGeomMaxLeaves;
    const int k = (int)(idx % kGeomMaxLeaves);
    if (i >= n_in || k >= min(counts[i], kGeomMaxLeaves)) return;
    const u64 o = pre[i] + (u64)k;
    if (o < (u64)n) tris[o] = stage[(size_t)i * kGeomMaxLeaves + k];
}

// ---- 2. span setup ----
// rows a triangle's spans take: the setup's ylo / yhi (:434-448)
__device__ __forceinline__ void tri_rows(const RastArgs &A, const Pix *vp, int &ylo, int &yhi, long long &rows)
{
    int mx = -INT_MAX, mn = INT_MAX;                        // :434-447
    for (int i = 0; i < 3; ++i) {
        if (vp[i].y > mx) mx = vp[i].y;
        if (vp[i].y < mn) mn = vp[i].y;
    }
    rows = (long long)mx - (long long)mn + 1;               // :448
    ylo = mn > 0 ? mn : 0;
    yhi = mx < A.H - 1 ? mx : A.H - 1;
}

__global__ __launch_bounds__(256) void rast_big_range_kernel(const cg_rtri *__restrict__ tris, RastArgs A, int n,
                                                            int *__restrict__ nrows)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const cg_rtri T = tris[t];
    const Pix vp[3] = {vertex_shader(A, T.v0), vertex_shader(A, T.v1), vertex_shader(A, T.v2)};
    int ylo, yhi;
    long long rows;
    tri_rows(A, vp, ylo, yhi, rows);
    nrows[t] = (rows <= 0 || ylo > yhi) ? 0 : yhi - ylo + 1;
}

// rast_setup_one (cg_rast.hip) with the spans of triangle t at spans[so ..], their (t, y) beside them
__device__ void big_setup_one(const cg_rtri &T, const RastArgs &A, RastSpan *__restrict__ spans,
                              uint2 *__restrict__ span_ty, u64 so, u64 span_cap, RastHdr *__restrict__ hdr,
                              int *__restrict__ first_tri, int t, unsigned long long *lkey,
                              unsigned long long *rkey, unsigned long long &fkey)
{
    Pix vp[3] = {vertex_shader(A, T.v0), vertex_shader(A, T.v1), vertex_shader(A, T.v2)};
    int ylo, yhi;
    long long rows;
    tri_rows(A, vp, ylo, yhi, rows);
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
    // Edge samples -> rows (:466-497), as rast_setup_one reduces them
    for (int ei = 0; ei < 3; ++ei) {
        const Edge &e = ei == 0 ? E0 : ei == 1 ? E1 : E2;
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
        if (so + (u64)k < span_cap) {                       // a triangle's spans are contiguous, rows ascending
            spans[so + (u64)k] = s;
            span_ty[so + (u64)k] = make_uint2((unsigned)t, (unsigned)(ylo + k));
        }
    }
    if (shade_tri) {
        __syncthreads();
        if (threadIdx.x == 0 && fkey != ~0ull) {
            h.fy = (int)(fkey >> 32);
            h.fx = (int)(fkey & 0xffffffffu);
            atomicMin(first_tri, t);                         // a minimum: the same whatever the order
        }
    }
    if (threadIdx.x == 0) hdr[t] = h;
}

// One workgroup per clipped triangle (grid-stride); LDS: the left | right keys of H rows.
__global__ __launch_bounds__(kSetupThreads) void rast_big_setup_kernel(
    const cg_rtri *__restrict__ tris, RastArgs A, int n, const u64 *__restrict__ span_off, u64 span_cap,
    RastSpan *__restrict__ spans, uint2 *__restrict__ span_ty, RastHdr *__restrict__ hdr,
    int *__restrict__ first_tri)
{
    extern __shared__ unsigned long long s_keys[];          // [2 * H]
    __shared__ unsigned long long fkey;
    unsigned long long *lkey = s_keys, *rkey = s_keys + A.H;
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        const cg_rtri T = tris[t];
        big_setup_one(T, A, spans, span_ty, span_off[t], span_cap, hdr, first_tri, t, lkey, rkey, fkey);
        __syncthreads();
    }
}

// ---- 3. row lists ----
// Lane's span of the batch at s (none past s1): whether it gives a record
// (fragments x in [lx, rx - 1] (:504) intersecting [0, W), as rast_rows_kernel
// keeps them), its row, and `eq`, the batch's record lanes of the same row.
__device__ __forceinline__ bool batch_rank(const RastArgs &A, const RastSpan *__restrict__ spans,
                                           const uint2 *__restrict__ span_ty, u64 s, u64 s1, RastSpan &sp,
                                           uint2 &ty, unsigned long long &eq)
{
    bool k = false;
    ty = make_uint2(0u, 0u);
    if (s < s1) {
        sp = spans[s];
        ty = span_ty[s];
        k = ty.x < (unsigned)A.n && ty.y < (unsigned)A.H && sp.rx > sp.lx && sp.rx - 1 >= 0 && sp.lx <= A.W - 1;
    }
    eq = __ballot(k);
#pragma unroll
    for (int b = 0; b < kRowBits; ++b) {
        const bool bit = (ty.y >> b) & 1u;
        const unsigned long long bb = __ballot(bit);
        eq &= bit ? bb : ~bb;
    }
    return k;
}

// One wave per chunk of kBigChunk spans.  WRITE = false: hist[chunk][y] = the
// chunk's records of row y.  WRITE = true: hist holds the chunk's base in each
// row (rast_big_colscan_kernel) and the records are stored; ENT (colour modes
// 1-2): with seg_off[span], the record's first entry of c, beside each.
template <bool WRITE, bool ENT>
__global__ __launch_bounds__(64) void rast_big_rows_kernel(RastArgs A, const RastSpan *__restrict__ spans,
                                                          const uint2 *__restrict__ span_ty, u64 n_spans,
                                                          int *__restrict__ hist, const RastHdr *__restrict__ hdr,
                                                          const int *__restrict__ first_tri,
                                                          const u64 *__restrict__ row_off, RowRec *__restrict__ recs,
                                                          u64 rec_cap, const u64 *__restrict__ seg_off,
                                                          u64 *__restrict__ rec_ent)
{
    extern __shared__ int s_cnt[];                          // [H]
    const int lane = threadIdx.x;
    int *hrow = hist + (size_t)blockIdx.x * A.H;
    for (int y = lane; y < A.H; y += 64) s_cnt[y] = WRITE ? hrow[y] : 0;
    __syncthreads();
    const int ft = (WRITE && A.want_first) ? *first_tri : INT_MAX;
    const u64 s0 = (u64)blockIdx.x * kBigChunk, s1 = min(s0 + (u64)kBigChunk, n_spans);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (u64 b = s0; b < s1; b += kBigBatch) {
        RastSpan sp;
        uint2 ty;
        unsigned long long eq;
        const bool k = batch_rank(A, spans, span_ty, b + lane, s1, sp, ty, eq);
        if (k) {
            const int rank = __popcll(eq & below);
            const int base = s_cnt[ty.y];                   // every lane reads before the row's last lane adds
            if (((eq >> lane) >> 1) == 0ull) s_cnt[ty.y] = base + rank + 1;
            if (WRITE) {
                const RastHdr h = hdr[ty.x];
                RowRec r;
                r.lx = sp.lx; r.rx = sp.rx;
                r.lz = sp.lz; r.sz = sp.sz; r.lX = sp.lX; r.sX = sp.sX; r.lY = sp.lY; r.sY = sp.sY;
                r.t_sh = h.t_sh;
                r.first_x = ((int)ty.x == ft && h.fy == (int)ty.y) ? h.fx : -1;
                r.tex = h.tex; r.index = h.index;
                const u64 o = row_off[ty.y] + (u64)(unsigned)(base + rank);
                if (o < rec_cap) recs[o] = r;
                if (ENT && o < rec_cap) rec_ent[o] = seg_off[b + lane];
            }
        }
    }
    if (!WRITE) {
        __syncthreads();
        for (int y = lane; y < A.H; y += 64) hrow[y] = s_cnt[y];
    }
}

// A thread per row: hist[.][y] becomes its exclusive prefix over the chunks, count[y] the row's records.
__global__ __launch_bounds__(64) void rast_big_colscan_kernel(int *__restrict__ hist, long long chunks, int H,
                                                             int *__restrict__ count)
{
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= H) return;
    int run = 0;
#pragma unroll 8
    for (long long c = 0; c < chunks; ++c) {
        const size_t o = (size_t)c * H + y;
        const int v = hist[o];
        hist[o] = run;
        run += v;
    }
    count[y] = run;
}

// One workgroup: row_off[y] = records before row y, row_off[H] the total, row_off[H + 1] the longest row.
__global__ __launch_bounds__(kScanThreads) void rast_big_rowoff_kernel(const int *__restrict__ count, int H,
                                                                       u64 *__restrict__ row_off)
{
    __shared__ u64 s_w[kScanThreads / 64];
    __shared__ int s_max[kScanThreads / 64];
    u64 carry = 0;
    int mx = 0;
    for (int y0 = 0; y0 < H; y0 += kScanThreads) {
        const int y = y0 + (int)threadIdx.x;
        const int v = y < H ? max(count[y], 0) : 0;
        mx = max(mx, v);
        u64 total;
        const u64 ex = block_excl_scan((u64)(unsigned)v, s_w, total);
        if (y < H) row_off[y] = carry + ex;
        carry += total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kScanThreads / 64; ++k) mx = max(mx, s_max[k]);
        row_off[H] = carry;
        row_off[H + 1] = (u64)(unsigned)mx;
    }
}

// ---- 4. fill and post: rast_fill_kernel / rast_post_kernel<false, TEX> on recs + row_off[y] ----
template <bool TEX>
__global__ __launch_bounds__(256) void rast_big_fill_kernel(RastArgs A, const RowRec *__restrict__ recs,
                                                           const u64 *__restrict__ row_off,
                                                           const int *__restrict__ count, u64 rec_cap,
                                                           uint32_t *__restrict__ state,
                                                           float *__restrict__ depth_out,
                                                           int32_t *__restrict__ shadow_out)
{
    const int segs = (A.W + kFillPx - 1) / kFillPx;
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
    const u64 ro = min(row_off[y], rec_cap);
    const int cnt = (int)min((u64)(unsigned)max(count[y], 0), rec_cap - ro);
    const RowRec *rr = recs + ro;
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
        unsigned long long mk = __ballot(ov);
        while (mk) {
            const int b = __builtin_ctzll(mk);
            mk &= mk - 1ull;
            // every readlane sits here, where the whole wave is active (see rast_fill_kernel)
            const int lx = __builtin_amdgcn_readlane(mlx, b);
            const int rx = __builtin_amdgcn_readlane(mrx, b);
            const float lz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mlz), b));
            const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(msz), b));
            const int shd = __builtin_amdgcn_readlane(msh, b);
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

// The text is cg_rast_big_post_kernel.inc, once per output policy (as cg_rast.hip's post-pass):
// rast_big_post_kernel stores PutPixelSDL's word, rast_big_post_f32_kernel (CG_PIX_RGBA_F32) the
// float4 it would have been given.
#define CG_RAST_POST_NAME rast_big_post_kernel
#define CG_RAST_POST_F32 0
#define CG_RAST_POST_OUT uint32_t
#include "cg_rast_big_post_kernel.inc"
#undef CG_RAST_POST_NAME
#undef CG_RAST_POST_F32
#undef CG_RAST_POST_OUT
#define CG_RAST_POST_NAME rast_big_post_f32_kernel
#define CG_RAST_POST_F32 1
#define CG_RAST_POST_OUT float4
#include "cg_rast_big_post_kernel.inc"
#undef CG_RAST_POST_NAME
#undef CG_RAST_POST_F32
#undef CG_RAST_POST_OUT

// ---- 5-7. colour modes 1-2 ----
// nseg[s]: the entries of c that span s takes, one per fill segment its visible extent overlaps
__global__ __launch_bounds__(256) void rast_big_segs_kernel(RastArgs A, const RastSpan *__restrict__ spans,
                                                           const uint2 *__restrict__ span_ty, u64 n_spans,
                                                           const RastHdr *__restrict__ hdr, int *__restrict__ nseg)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_spans) return;
    const uint2 ty = span_ty[s];
    int k = 0, first;
    if (ty.x < (unsigned)A.n && ty.y < (unsigned)A.H && (hdr[ty.x].t_sh >> 31) == 0u)   // as batch_rank keeps them
        k = rast_span_segments(spans[s].lx, spans[s].rx, A.W, &first);
    nseg[s] = k;
}

// rast_big_fill_kernel's walk with the ordered z-buffer of rast_count_kernel / rast_fill_rand_kernel.
// SHADE = false: c[entry] = the fragments of the record that pass in this segment (lane q keeps
// the count of record base + q and stores it after the batch).  SHADE = true: a passing fragment
// takes the number fbase[entry] + the passing lanes below it, and each pixel's last winner is
// shaded with its three values into the kStateDirect state.
template <bool SHADE>
__global__ __launch_bounds__(256) void rast_big_colour_kernel(RastArgs A0, const RowRec *__restrict__ recs,
                                                             const u64 *__restrict__ row_off,
                                                             const int *__restrict__ count, u64 rec_cap,
                                                             const u64 *__restrict__ rec_ent, u64 n_ent,
                                                             int *__restrict__ c, const u64 *__restrict__ fbase,
                                                             const int32_t *__restrict__ rnd, long long n_shaded,
                                                             int mode, float4 *__restrict__ state,
                                                             float *__restrict__ depth_out,
                                                             int32_t *__restrict__ shadow_out)
{
    const RastArgs A = SHADE ? with_device_light(A0) : A0;
    const int segs = (A.W + kFillPx - 1) / kFillPx;
    int m;
    const int g = xcd_group(A.H, (segs * kXcdRows + 3) / 4, m);
    if (g < 0) return;
    const int unit = m * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (row, segment) in the group
    const int lane = threadIdx.x & 63;
    const int y = g * kXcdRows + unit / segs;
    if (unit >= segs * kXcdRows || y >= A.H) return;
    const int seg = unit % segs, x0 = seg * kFillPx;
    const int x = x0 + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    float depth = 0.0f;                                   // :247
    int shadow = 0, win = -1;                             // :259; record of the last shading fragment
    long long widx = 0;                                   // its number among the frame's shaded fragments
    const u64 ro = min(row_off[y], rec_cap);
    const int cnt = (int)min((u64)(unsigned)max(count[y], 0), rec_cap - ro);
    const RowRec *rr = recs + ro;
    for (int base = 0; base < cnt; base += 64) {
        const int q = base + lane;
        int mlx = 0, mrx = 0, msh = 0;
        float mlz = 0.f, msz = 0.f;
        u64 ment = 0;
        if (q < cnt) {
            const RowRec &mr = rr[q];
            mlx = mr.lx; mrx = mr.rx; mlz = mr.lz; msz = mr.sz; msh = rec_shadow(mr);
            ment = rec_ent[ro + q];
        }
        const bool ov = q < cnt && !(mrx - 1 < x0 || mlx > x0 + kFillPx - 1);
        // the record's entry for this segment: seg_off[span] + (segment - the span's first)
        int first;
        const int ns = rast_span_segments(mlx, mrx, A.W, &first);
        const u64 ent = ment + (u64)(unsigned)(seg - first);
        const bool own = ov && !msh && seg >= first && seg - first < ns && ent < n_ent;
        int mine = 0;                                     // SHADE = false: the passes of record base + lane
        long long mfb = 0;
        if (SHADE && own) mfb = (long long)fbase[ent];
        unsigned long long mk = __ballot(SHADE ? ov : own);   // shadow triangles never shade
        while (mk) {
            const int b = __builtin_ctzll(mk);
            mk &= mk - 1ull;
            // every readlane sits here, where the whole wave is active (see rast_fill_kernel)
            const int lx = __builtin_amdgcn_readlane(mlx, b);
            const int rx = __builtin_amdgcn_readlane(mrx, b);
            const float lz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mlz), b));
            const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(msz), b));
            const int shd = SHADE ? __builtin_amdgcn_readlane(msh, b) : 0;
            long long fb = 0;
            if (SHADE)
                fb = (long long)(((u64)(unsigned)__builtin_amdgcn_readlane((int)((u64)mfb >> 32), b) << 32) |
                                 (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)mfb, b));
            const int i = x - lx;
            const bool in = x < A.W && i >= 0 && x < rx;             // :504, :573
            const float zinv = lz + (sz * (float)i);                 // :543
            if (!shd) {
                const bool pass = in && zinv >= depth;               // :574
                const unsigned long long pm = __ballot(pass);
                if (pass) {
                    depth = zinv;                                    // :665
                    win = base + b;
                    widx = fb + __popcll(pm & below);
                }
                if (!SHADE && lane == b) mine = __popcll(pm);
            } else if (in && zinv > depth) {                         // :668-669
                shadow = 1;
            }
        }
        if (!SHADE && own) c[ent] = mine;
    }
    if (!SHADE || x >= A.W) return;
    float4 st = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
    if (win >= 0 && widx >= 0 && widx < n_shaded) {
        const RowRec r = rr[win];
        const int i = x - r.lx;
        const float X = r.lX + (r.sX * (float)i);                    // :547-548 numerators
        const float Y = r.lY + (r.sY * (float)i);
        const cg_vec4 tn = A.tris[rec_t(r)].normal;
        const vec3 D = illum_D(A, depth, X, Y, v3(tn.x, tn.y, tn.z));
        const float r0 = rand_unit(rnd[3 * widx]), r1 = rand_unit(rnd[3 * widx + 1]), r2 = rand_unit(rnd[3 * widx + 2]);
        const vec3 rc = mode == 1 ? v3(r0, r1, r2) : v3(r0 - 0.2f, 1.0f, r2 - 0.2f);   // :652 / :660
        const float ind = A.ind_first;                               // modes 1-2 never rewrite it
        const vec3 sc = rc * (D + v3(ind, ind, ind));
        st = make_float4(__int_as_float(kStateDirect), sc.x, sc.y, sc.z);
    }
    const size_t o = (size_t)y * A.W + x;
    state[o] = st;
    if (depth_out) depth_out[o] = depth;
    shadow_out[o] = shadow;
}

// ---- host ----
namespace {

// ctx_buf slots of this route's own buffers (cg_ctx::rbig[which - kBufBig0])
enum { kBigTris = kBufBig0, kBigPre, kBigNrows, kBigSpanOff, kBigSpanTy, kBigHist, kBigRowOff, kBigScan,
       // colour modes 1-2 only: segments per span, their offsets, each record's first entry, the
       // entries' fragment counts, their prefix, the rand() stream and its jump table
       kBigNseg, kBigSegOff, kBigRecEnt, kBigEnt, kBigFbase, kBigRnd, kBigJt };

// The refusal of a colour mode 1-2 frame that cg_rast_set_route(ctx, 1) forced here: the hook is a
// colour-mode-0 A/B switch (modes 1-2 reach this route on the automatic choice only).
const char *const kForcedColour =
    "compact route: colour modes 1-2 are not built for it (their count, scan, generator "
    "and chain kernels read the dense layout); colour mode 0 only";

// a few bytes the host needs before it can size the next buffer: the documented waits
int big_read(cg_ctx *c, hipStream_t st, void *dst, const void *src, size_t bytes, const char *what)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? CG_OK : ctx_fail(c, e, what);
}

// out[i] = in[0] + .. + in[i - 1] (negative counts as 0), out[N] the total
int big_scan(cg_ctx *c, hipStream_t st, const int *in, long long N, u64 *out)
{
    hipError_t e;
    if (N <= 0) {
        e = hipMemsetAsync(out, 0, sizeof(u64), st);
        return e == hipSuccess ? CG_OK : ctx_fail(c, e, "memset");
    }
    const long long nb = (N + kScanBlock - 1) / kScanBlock;
    u64 *bsum = (u64 *)ctx_buf(c, kBigScan, (size_t)nb * sizeof(u64), &e);
    if (!bsum) return ctx_fail(c, e, "alloc scan sums");
    hipLaunchKernelGGL(rast_big_scan_reduce_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, st, in, N, bsum);
    hipLaunchKernelGGL(rast_big_scan_top_kernel, dim3(1), dim3(kScanThreads), 0, st, bsum, (int)nb, out + N);
    hipLaunchKernelGGL(rast_big_scan_apply_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, st, in, N,
                       (const u64 *)bsum, out);
    e = hipGetLastError();
    return e == hipSuccess ? CG_OK : ctx_fail(c, e, "rast_big_scan launch");
}

// Colour modes 1-2 from the row records on: count, scan, (host: in a sequence the call index,
// then S), generator, number and shade, post.  seq: the frame's record is written too.
int big_colour(cg_ctx *c, const RastArgs &A, const cg_rast_params *p, const RowRec *recs, const u64 *row_off,
               const int *count, u64 n_recs, const u64 *rec_ent, u64 n_ent, float4 *state, uint32_t *d_argb,
               float *d_depth, int32_t *d_shadow, hipStream_t st, const RastSeq *seq, long long *n_shaded, int pix)
{
    hipError_t e;
    const size_t npx = (size_t)A.W * A.H, ne = n_ent > 0 ? (size_t)n_ent : 1;
    int32_t *shadow = d_shadow;   // the post-pass reads the marks from the plane
    if (!shadow && !(shadow = (int32_t *)ctx_buf(c, kBufShadow, npx * sizeof(int32_t), &e))) return ctx_fail(c, e, "alloc shadow");
    int *ent = (int *)ctx_buf(c, kBigEnt, ne * sizeof(int), &e);
    if (!ent) return ctx_fail(c, e, "alloc entry counts");
    u64 *fbase = (u64 *)ctx_buf(c, kBigFbase, (ne + 1) * sizeof(u64), &e);
    if (!fbase) return ctx_fail(c, e, "alloc fragment numbers");
    const int fgrid = xcd_grid(A.H, ((A.W + kFillPx - 1) / kFillPx * kXcdRows + 3) / 4);
    {
        KtScope kt(KT_RAST_BIG_COUNT, st);
        // every entry has one writer; cleared all the same: a hole would be a wrong count, not a stray one
        if ((e = hipMemsetAsync(ent, 0, ne * sizeof(int), st)) != hipSuccess) return ctx_fail(c, e, "memset");
        if (n_ent > 0)
            hipLaunchKernelGGL(rast_big_colour_kernel<false>, dim3(fgrid), dim3(256), 0, st, A, recs, row_off, count,
                               n_recs, rec_ent, n_ent, ent, (const u64 *)nullptr, (const int32_t *)nullptr, 0ll, 0,
                               (float4 *)nullptr, (float *)nullptr, (int32_t *)nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_count launch");
        if (const int rc = big_scan(c, st, ent, (long long)n_ent, fbase)) return rc;
    }
    uint64_t offset = seq ? seq->start : p->rand_offset;
    if (seq && !seq->first)   // what the previous frame's step left in this frame's record
        if (const int rc = big_read(c, st, &offset, &seq->info->rand_offset, sizeof(offset), "call index")) return rc;
    u64 S = 0;
    if (const int rc = big_read(c, st, &S, fbase + n_ent, sizeof(u64), "shaded-fragment count")) return rc;
    *n_shaded = (long long)S;
    int32_t *rnd = nullptr;
    {
        KtScope kt(KT_RAST_BIG_RAND, st);
        if (const int rc = rast_rand_stream(c, kBigRnd, kBigJt, offset, (long long)S, st, &rnd)) return rc;
    }
    {
        KtScope kt(KT_RAST_BIG_SHADE, st);
        hipLaunchKernelGGL(rast_big_colour_kernel<true>, dim3(fgrid), dim3(256), 0, st, A, recs, row_off, count, n_recs,
                           rec_ent, n_ent, (int *)nullptr, (const u64 *)fbase, (const int32_t *)rnd, (long long)S,
                           p->colour_mode, state, d_depth, shadow);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_shade launch");
    }
    if (d_argb) {   // null: a buffers call that asks for no picture
        KtScope kt(KT_RAST_BIG_POST, st);
        launch_rast_post_direct(A, state, shadow, d_argb, st, pix);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_post launch");
    }
    if (seq) {
        const int rc = rast_seq_chain_exact(c, st, *seq, (const long long *)(fbase + n_ent));
        if (rc) return rc;
    }
    // the generator's jump table was uploaded from host memory that a later frame may grow
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return ctx_fail(c, e, "colour frame");
    return CG_OK;
}

// Span setup, row lists, fill and post over a clipped list whose length the host knows.
// clip_ran: rast_clip_kernel initialised the first-fragment minimum on this stream.  pix: d_argb's
// pixel format (CG_PIX_RGBA_F32: float4 pixels from the post-pass's float kernels).
int big_pipeline(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light,
                 const cg_vec4 *d_light, uint32_t *d_argb, float *d_depth, int32_t *d_shadow, hipStream_t st,
                 cg_stats *stats, bool events_open, bool clip_ran, int tex_mask, const RastSeq *seq,
                 int pix = CG_PIX_ARGB8888)
{
    if (p->width <= 2 || p->height <= 2 || p->height > kRastMaxRows) return CG_E_INVALID;
    if (p->colour_mode != 0 && ctx_rast_forced_compact(c)) return ctx_invalid(c, kForcedColour);
    const int W = p->width, H = p->height;
    const size_t npx = (size_t)W * H;
    hipError_t e;
    RastArgs A;
    if (const int rc = rast_make_args(c, d_tris, n, p, light, d_light, tex_mask, &A)) return rc;
    int *misc = (int *)ctx_buf(c, kBufCount, ((size_t)H + 16) * sizeof(int), &e);   // count[H] | first_tri
    if (!misc) return ctx_fail(c, e, "alloc counts");
    int *count = misc, *first_tri = misc + H;
    const size_t nn = n > 0 ? (size_t)n : 1;
    RastHdr *hdr = (RastHdr *)ctx_buf(c, kBufHdr, nn * sizeof(RastHdr), &e);
    if (!hdr) return ctx_fail(c, e, "alloc hdr");
    int *nrows = (int *)ctx_buf(c, kBigNrows, nn * sizeof(int), &e);
    if (!nrows) return ctx_fail(c, e, "alloc row counts");
    u64 *span_off = (u64 *)ctx_buf(c, kBigSpanOff, (nn + 1) * sizeof(u64), &e);
    if (!span_off) return ctx_fail(c, e, "alloc span offsets");
    u64 *row_off = (u64 *)ctx_buf(c, kBigRowOff, ((size_t)H + 2) * sizeof(u64), &e);
    if (!row_off) return ctx_fail(c, e, "alloc row offsets");
    const bool colour = p->colour_mode != 0;
    // fill -> post state: 4 B/pixel in colour mode 0, the colour walk's 16 B in modes 1-2
    void *state = ctx_buf(c, kBufPix, npx * (colour ? sizeof(float4) : sizeof(uint32_t)), &e);
    if (!state) return ctx_fail(c, e, "alloc state");
    hipEvent_t e0, e1;
    ctx_events(c, &e0, &e1);
    if (stats && !events_open && (e = hipEventRecord(e0, st)) != hipSuccess) return ctx_fail(c, e, "event");
    if (A.want_first && !clip_ran && (e = hipMemsetAsync(first_tri, 0x7f, sizeof(int), st)) != hipSuccess)
        return ctx_fail(c, e, "memset");
    // -- span setup: rows per triangle, their offsets, the spans
    u64 n_spans = 0;
    if (n > 0) {
        {
            KtScope kt(KT_RAST_BIG_SETUP, st);
            hipLaunchKernelGGL(rast_big_range_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_tris, A, n,
                               nrows);
            if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_range launch");
            if (const int rc = big_scan(c, st, nrows, n, span_off)) return rc;
        }
        if (const int rc = big_read(c, st, &n_spans, span_off + n, sizeof(u64), "span total")) return rc;
    }
    const size_t ns = n_spans > 0 ? (size_t)n_spans : 1;
    RastSpan *spans = (RastSpan *)ctx_buf(c, kBufSpan, ns * sizeof(RastSpan), &e);
    if (!spans) return ctx_fail(c, e, "alloc spans");
    uint2 *span_ty = (uint2 *)ctx_buf(c, kBigSpanTy, ns * sizeof(uint2), &e);
    if (!span_ty) return ctx_fail(c, e, "alloc span keys");
    const long long chunks = (long long)((n_spans + kBigChunk - 1) / kBigChunk);
    int *hist = (int *)ctx_buf(c, kBigHist, (size_t)std::max(chunks, 1ll) * H * sizeof(int), &e);
    if (!hist) return ctx_fail(c, e, "alloc row histogram");
    if (n > 0) {
        KtScope kt(KT_RAST_BIG_SETUP, st);
        const int grid = n < 8192 ? n : 8192;
        hipLaunchKernelGGL(rast_big_setup_kernel, dim3(grid), dim3(kSetupThreads), 2 * (size_t)H * 8, st, d_tris, A, n,
                           (const u64 *)span_off, n_spans, spans, span_ty, hdr, first_tri);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_setup launch");
    }
    // -- colour modes 1-2: the entries of c each span takes, their offsets
    u64 *seg_off = nullptr, n_ent = 0;
    if (colour) {
        int *nseg = (int *)ctx_buf(c, kBigNseg, ns * sizeof(int), &e);
        if (!nseg) return ctx_fail(c, e, "alloc span segments");
        seg_off = (u64 *)ctx_buf(c, kBigSegOff, (ns + 1) * sizeof(u64), &e);
        if (!seg_off) return ctx_fail(c, e, "alloc segment offsets");
        {
            KtScope kt(KT_RAST_BIG_COUNT, st);
            if (n_spans > 0)
                hipLaunchKernelGGL(rast_big_segs_kernel, dim3((unsigned)((n_spans + 255) / 256)), dim3(256), 0, st, A,
                                   (const RastSpan *)spans, (const uint2 *)span_ty, n_spans, (const RastHdr *)hdr, nseg);
            if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_segs launch");
            if (const int rc = big_scan(c, st, nseg, (long long)n_spans, seg_off)) return rc;
        }
        if (const int rc = big_read(c, st, &n_ent, seg_off + n_spans, sizeof(u64), "segment total")) return rc;
    }
    // -- row lists: count, scan, (host: totals), write
    u64 tot[2] = {0, 0};   // records, the longest row
    {
        KtScope kt(KT_RAST_BIG_ROWS, st);
        if (chunks > 0)
            hipLaunchKernelGGL((rast_big_rows_kernel<false, false>), dim3((unsigned)chunks), dim3(64),
                               (size_t)H * sizeof(int), st, A, (const RastSpan *)spans, (const uint2 *)span_ty, n_spans,
                               hist, (const RastHdr *)hdr, (const int *)first_tri, (const u64 *)row_off,
                               (RowRec *)nullptr, (u64)0, (const u64 *)nullptr, (u64 *)nullptr);
        hipLaunchKernelGGL(rast_big_colscan_kernel, dim3((H + 63) / 64), dim3(64), 0, st, hist, chunks, H, count);
        hipLaunchKernelGGL(rast_big_rowoff_kernel, dim3(1), dim3(kScanThreads), 0, st, (const int *)count, H, row_off);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_rows launch");
    }
    if (const int rc = big_read(c, st, tot, row_off + H, sizeof(tot), "record total")) return rc;
    const u64 n_recs = tot[0];
    RowRec *recs = (RowRec *)ctx_buf(c, kBufRecs, (size_t)std::max<u64>(n_recs, 1) * sizeof(RowRec), &e);
    if (!recs) return ctx_fail(c, e, "alloc row records");
    A.state16 = !colour && tot[1] < 32768;
    u64 *rec_ent = nullptr;
    if (colour && !(rec_ent = (u64 *)ctx_buf(c, kBigRecEnt, (size_t)std::max<u64>(n_recs, 1) * sizeof(u64), &e)))
        return ctx_fail(c, e, "alloc record entries");
    if (chunks > 0 && n_recs > 0) {
        KtScope kt(KT_RAST_BIG_ROWS, st);
        if (colour)
            hipLaunchKernelGGL((rast_big_rows_kernel<true, true>), dim3((unsigned)chunks), dim3(64),
                               (size_t)H * sizeof(int), st, A, (const RastSpan *)spans, (const uint2 *)span_ty, n_spans,
                               hist, (const RastHdr *)hdr, (const int *)first_tri, (const u64 *)row_off, recs, n_recs,
                               (const u64 *)seg_off, rec_ent);
        else
            hipLaunchKernelGGL((rast_big_rows_kernel<true, false>), dim3((unsigned)chunks), dim3(64),
                               (size_t)H * sizeof(int), st, A, (const RastSpan *)spans, (const uint2 *)span_ty, n_spans,
                               hist, (const RastHdr *)hdr, (const int *)first_tri, (const u64 *)row_off, recs, n_recs,
                               (const u64 *)nullptr, (u64 *)nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_rows launch");
    }
    long long n_shaded = -1;
    void *words = state;   // the ordered z-buffer's state words (RastFrame)
    if (colour) {
        const int rc = big_colour(c, A, p, recs, row_off, count, n_recs, rec_ent, n_ent, (float4 *)state, d_argb, d_depth,
                                  d_shadow, st, seq, &n_shaded, pix);
        if (rc) return rc;
        if (ctx_rast_want_owner(c)) {
            // the owner of a pixel is the ordered z-buffer's last writer whatever the colour mode
            // (modes 1-2 ignore textures, :604): the mode-0 fill's walk into words of its own
            words = ctx_buf(c, kBufOwner, npx * sizeof(uint32_t), &e);
            if (!words) return ctx_fail(c, e, "alloc owner state");
            A.state16 = tot[1] < 32768;
            const int fgrid = xcd_grid(H, ((W + kFillPx - 1) / kFillPx * kXcdRows + 3) / 4);
            hipLaunchKernelGGL(rast_big_fill_kernel<false>, dim3(fgrid), dim3(256), 0, st, A, (const RowRec *)recs,
                               (const u64 *)row_off, (const int *)count, n_recs, (uint32_t *)words, (float *)nullptr,
                               (int32_t *)nullptr);
            if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_fill launch");
        }
    } else {
        // -- fill and post
        {
            KtScope kt(KT_RAST_BIG_FILL, st);
            const int fgrid = xcd_grid(H, ((W + kFillPx - 1) / kFillPx * kXcdRows + 3) / 4);
            if (A.textured)
                hipLaunchKernelGGL(rast_big_fill_kernel<true>, dim3(fgrid), dim3(256), 0, st, A, (const RowRec *)recs,
                                   (const u64 *)row_off, (const int *)count, n_recs, (uint32_t *)state, d_depth, d_shadow);
            else
                hipLaunchKernelGGL(rast_big_fill_kernel<false>, dim3(fgrid), dim3(256), 0, st, A, (const RowRec *)recs,
                                   (const u64 *)row_off, (const int *)count, n_recs, (uint32_t *)state, d_depth, d_shadow);
            if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_fill launch");
        }
        if (d_argb) {   // null: a buffers call that asks for no picture
            KtScope kt(KT_RAST_BIG_POST, st);
            const int post_grid = xcd_grid(H, (W + kPostTW - 1) / kPostTW);
            if (pix == CG_PIX_RGBA_F32 && A.textured)
                hipLaunchKernelGGL(rast_big_post_f32_kernel<true>, dim3(post_grid), dim3(256), 0, st, d_tris, A,
                                   (const void *)state, (const RowRec *)recs, (const u64 *)row_off, n_recs,
                                   (float4 *)d_argb);
            else if (pix == CG_PIX_RGBA_F32)
                hipLaunchKernelGGL(rast_big_post_f32_kernel<false>, dim3(post_grid), dim3(256), 0, st, d_tris, A,
                                   (const void *)state, (const RowRec *)recs, (const u64 *)row_off, n_recs,
                                   (float4 *)d_argb);
            else if (A.textured)
                hipLaunchKernelGGL(rast_big_post_kernel<true>, dim3(post_grid), dim3(256), 0, st, d_tris, A,
                                   (const void *)state, (const RowRec *)recs, (const u64 *)row_off, n_recs, d_argb);
            else
                hipLaunchKernelGGL(rast_big_post_kernel<false>, dim3(post_grid), dim3(256), 0, st, d_tris, A,
                                   (const void *)state, (const RowRec *)recs, (const u64 *)row_off, n_recs, d_argb);
            if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_post launch");
        }
        if (seq) {
            const int rc = rast_seq_chain_mode0(c, st, *seq);
            if (rc) return rc;
        }
    }
    if (stats && (e = hipEventRecord(e1, st)) != hipSuccess) return ctx_fail(c, e, "event");
    if (stats) {
        stats->n_tris = n;
        stats->n_spans = 0;   // as the dense route reports it; the frame's spans: cg_rast_scratch_info
        stats->n_shaded = n_shaded;
    }
    *ctx_rast_last(c) = RastLast{CG_RAST_ROUTE_COMPACT, (long long)n, (long long)n_spans, (long long)n_recs, nullptr,
                                 nullptr, H, st};
    RastFrame &fr = *ctx_rast_frame(c);
    fr = RastFrame{};
    fr.valid = !colour || words != state;
    fr.route = CG_RAST_ROUTE_COMPACT;
    fr.mode = p->colour_mode;
    fr.A = A;
    fr.words = words;
    fr.direct = colour ? (const float4 *)state : nullptr;
    fr.recs = recs;
    fr.row_off = row_off;
    fr.rec_cap = n_recs;
    fr.st = st;
    return CG_OK;
}

}  // namespace

int rast_big_render(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light, uint32_t *d_argb,
                    float *d_depth, int32_t *d_shadow, hipStream_t st, cg_stats *stats, int tex_mask)
{
    return big_pipeline(c, d_tris, n, p, light, nullptr, d_argb, d_depth, d_shadow, st, stats, false, false, tex_mask,
                        nullptr);
}

// Whole Draw: clip on the device, the survivors compacted by a scan of their counts, then the
// pipeline above over a list of exactly the clipped length.  *n_out: a device word that holds it.
int rast_big_draw(cg_ctx *c, const cg_rtri *d_room, int n_room, const cg_rtri *d_boxes, int n_boxes,
                  const cg_rast_params *p, uint32_t *d_argb, float *d_depth, int32_t *d_shadow, hipStream_t st,
                  cg_stats *stats, int **n_out, int tex_mask, const RastSeq *seq, int pix)
{
    if (p->width <= 2 || p->height <= 2 || p->height > kRastMaxRows || p->focal == 0.0f) return CG_E_INVALID;
    if (p->colour_mode != 0 && ctx_rast_forced_compact(c)) return ctx_invalid(c, kForcedColour);
    const long long n_in_ll = (long long)n_room + 7ll * n_boxes;
    if (n_in_ll > kRastMaxInputs) return ctx_invalid(c, "more than 4194304 input triangles");
    const int n_in = (int)n_in_ll;
    const size_t ni = n_in > 0 ? (size_t)n_in : 1;
    hipError_t e;
    // each input triangle's staged survivors (32 each)
    cg_rtri *stage = (cg_rtri *)ctx_buf(c, kBufTris, ni * kGeomMaxLeaves * sizeof(cg_rtri), &e);
    if (!stage) return ctx_fail(c, e, "alloc clip staging");
    int *geo = (int *)ctx_buf(c, kBufGeo, 64 + 4 * ni, &e);   // [4..7] light, [16..] counts
    if (!geo) return ctx_fail(c, e, "alloc geometry header");
    int *misc = (int *)ctx_buf(c, kBufCount, ((size_t)p->height + 16) * sizeof(int), &e);   // count[H] | first_tri
    if (!misc) return ctx_fail(c, e, "alloc counts");
    u64 *pre = (u64 *)ctx_buf(c, kBigPre, (ni + 1) * sizeof(u64), &e);
    if (!pre) return ctx_fail(c, e, "alloc clip offsets");
    hipEvent_t e0, e1;
    ctx_events(c, &e0, &e1);
    if (stats && (e = hipEventRecord(e0, st)) != hipSuccess) return ctx_fail(c, e, "event");
    {
        KtScope kt(KT_RAST_BIG_CLIP, st);
        if ((e = launch_rast_clip(*p, d_room, n_room, d_boxes, n_boxes, stage, geo + 16, (cg_vec4 *)(geo + 4),
                                  misc + p->height, st)) != hipSuccess)
            return ctx_fail(c, e, "rast_clip launch");
        if (const int rc = big_scan(c, st, geo + 16, n_in, pre)) return rc;
    }
    u64 total = 0;
    if (const int rc = big_read(c, st, &total, pre + n_in, sizeof(u64), "clipped count")) return rc;
    if (total > (u64)kGeomMaxLeaves * (u64)ni) return ctx_invalid(c, "clipped count past the clip's capacity");
    const int n = (int)total;
    cg_rtri *tris = (cg_rtri *)ctx_buf(c, kBigTris, (size_t)std::max(n, 1) * sizeof(cg_rtri), &e);
    if (!tris) return ctx_fail(c, e, "alloc clipped triangles");
    if (n > 0) {
        KtScope kt(KT_RAST_BIG_CLIP, st);
        const long long threads = (long long)n_in * kGeomMaxLeaves;
        hipLaunchKernelGGL(rast_big_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st,
                           (const cg_rtri *)stage, (const int *)(geo + 16), (const u64 *)pre, n_in, tris, n);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_big_gather launch");
    }
    if (n_out) *n_out = (int *)(pre + n_in);   // little-endian: the count's low word
    const int rc = big_pipeline(c, tris, n, p, cg_vec4{0, 0, 0, 1}, (const cg_vec4 *)(geo + 4), d_argb, d_depth, d_shadow,
                                st, stats, true, n_in > 0, tex_mask, seq, pix);
    if (rc == CG_OK) {   // clipped triangle -> input triangle: the counts and the prefix the gather used
        RastFrame &fr = *ctx_rast_frame(c);
        fr.counts = geo + 16;
        fr.pre = pre;
        fr.n_in = n_in;
    }
    return rc;
}

}  // namespace cg
