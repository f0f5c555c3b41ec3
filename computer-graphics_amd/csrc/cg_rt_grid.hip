// cg_rt_grid.hip -- the scene grid and the scene bounds of cg_rt_set_scene_device, built on the
// device from triangles that live there (gfx950).  The host builder (rt_grid_build,
// cg_rt_big.hip) is the checker: both share cg_rt_grid.h, and the grid is the same bit for bit.
//
//   bounds   rt_grid_bounds_kernel + rt_grid_bounds_final_kernel: per-axis vertex min / max and
//            the largest |normal component|; the host reads seven floats (wait 1) and sizes the
//            grid with its own cbrt / ceil (rt_grid_dims)
//   ranges   rt_grid_ranges_kernel: a thread per triangle, its cell range (packed) and the cell
//            count of its bounding box; a 64-bit exclusive scan gives every triangle's first
//            candidate and the candidate total B, which the host reads (wait 2)
//   count    rt_grid_count_kernel: a thread per candidate (triangle, cell) pair -- no loop over a
//            triangle's cells, so a large triangle is many threads, not a long thread -- runs
//            tri_meets_cell in FP64, counts per cell with integer atomics and keeps the wave's
//            verdicts as one 64-bit word
//   offsets  a scan over the cells gives start[cells + 1] and the entry total E; cells longer
//            than kSortSmall are listed; the host reads E and that list's length (wait 3)
//   fill     rt_grid_fill_kernel: a thread per candidate again, the accepted ones take a slot of
//            their cell's segment from a per-cell cursor (any order)
//   order    every segment is sorted ascending, the host builder's order, which makes the result
//            independent of scheduling: rt_grid_sort_small_kernel (a thread per cell, at most
//            kSortSmall entries) and rt_grid_sort_long_kernel (a workgroup per listed cell: a
//            bitonic network in LDS up to kSortLds entries, in global memory beyond)
//
// Every store is guarded by its buffer's capacity and every loop by a count the host knows (n,
// the cell count, B, E, or a constant).  Integer atomics only: the counts do not depend on order.
#include <algorithm>
#include <cstring>

#include "cg_rt_grid.h"

namespace cg {

namespace {
constexpr int kGridThreads = 256;
constexpr int kScanTile = 1024;      // elements per scan workgroup: 256 threads x 4
constexpr int kBoundsBlocks = 1024;  // partial results of the bounds pass
constexpr int kSortSmall = 16;       // segments up to here: one thread, insertion sort
constexpr int kSortLds = 4096;       // segments up to here: bitonic network in LDS (16 KB)

// a triangle's cell range in one word: c0 and c1 per axis, 10 bits each (res <= 512)
__host__ __device__ inline uint64_t pack_range(const int c0[3], const int c1[3])
{
    return (uint64_t)c0[0] | (uint64_t)c0[1] << 10 | (uint64_t)c0[2] << 20 | (uint64_t)c1[0] << 30 |
           (uint64_t)c1[1] << 40 | (uint64_t)c1[2] << 50;
}

__global__ __launch_bounds__(kGridThreads) void rt_grid_bounds_kernel(const cg_tri *__restrict__ tris, int n,
                                                                      float *__restrict__ part)
{
    __shared__ float s[7][kGridThreads];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, nb = 0.f;
    const int stride = (int)gridDim.x * kGridThreads;
    for (int i = (int)blockIdx.x * kGridThreads + (int)threadIdx.x; i < n; i += stride) {
        const cg_tri t = tris[i];
        const float vx[3][3] = {{t.v0.x, t.v0.y, t.v0.z}, {t.v1.x, t.v1.y, t.v1.z}, {t.v2.x, t.v2.y, t.v2.z}};
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int a = 0; a < 3; ++a) {   // fminf / fmaxf ignore a NaN, as std::min(acc, x) does
                mn[a] = fminf(mn[a], vx[v][a]);
                mx[a] = fmaxf(mx[a], vx[v][a]);
            }
        const float q[3] = {t.normal.x, t.normal.y, t.normal.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) nb = isfinite(q[a]) ? fmaxf(nb, fabsf(q[a])) : INFINITY;
    }
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s[a][tid] = mn[a];
        s[3 + a][tid] = mx[a];
    }
    s[6][tid] = nb;
    __syncthreads();
    for (int d = kGridThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[a][tid] = fminf(s[a][tid], s[a][tid + d]);
                s[3 + a][tid] = fmaxf(s[3 + a][tid], s[3 + a][tid + d]);
            }
            s[6][tid] = fmaxf(s[6][tid], s[6][tid + d]);
        }
        __syncthreads();
    }
    if (tid < 7) part[(int)blockIdx.x * 8 + tid] = s[tid][0];
}

// One finishing block over the nb partial results (nb <= kBoundsBlocks).
__global__ __launch_bounds__(kGridThreads) void rt_grid_bounds_final_kernel(const float *__restrict__ part, int nb,
                                                                            float *__restrict__ out)
{
    __shared__ float s[7][kGridThreads];
    const int tid = (int)threadIdx.x;
    float acc[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.f};
    for (int b = tid; b < nb; b += kGridThreads) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const float x = part[b * 8 + k];
            acc[k] = k < 3 ? fminf(acc[k], x) : fmaxf(acc[k], x);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k][tid] = acc[k];
    __syncthreads();
    for (int d = kGridThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int k = 0; k < 7; ++k)
                s[k][tid] = k < 3 ? fminf(s[k][tid], s[k][tid + d]) : fmaxf(s[k][tid], s[k][tid + d]);
        }
        __syncthreads();
    }
    if (tid < 7) out[tid] = s[tid][0];
}

__global__ __launch_bounds__(kGridThreads) void rt_grid_ranges_kernel(const cg_tri *__restrict__ tris, int n, GridDims d,
                                                                      uint64_t *__restrict__ rng,
                                                                      uint64_t *__restrict__ cnt)
{
    const int i = (int)blockIdx.x * kGridThreads + (int)threadIdx.x;
    if (i >= n) return;
    const cg_tri t = tris[i];
    const double gh = d.h, eps = 1e-4 * gh;
    int c0[3], c1[3];
    grid_tri_range(t, d.lo, d.res, gh, eps, c0, c1);
    rng[i] = pack_range(c0, c1);
    // c1 < c0 on an axis (a triangle without a finite component there): no cells, as the host's loop
    uint64_t m = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) m *= c1[a] >= c0[a] ? (uint64_t)(c1[a] - c0[a] + 1) : 0ull;
    cnt[i] = m;
}

template <typename T>
__global__ __launch_bounds__(kGridThreads) void rt_grid_scan_sums_kernel(const T *__restrict__ in, uint64_t N,
                                                                         uint64_t *__restrict__ bsum)
{
    __shared__ uint64_t s[kGridThreads];
    const int tid = (int)threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)tid * 4;
    uint64_t a = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < N) a += (uint64_t)in[base + j];
    s[tid] = a;
    __syncthreads();
    for (int d = kGridThreads / 2; d > 0; d >>= 1) {
        if (tid < d) s[tid] += s[tid + d];
        __syncthreads();
    }
    if (tid == 0) bsum[blockIdx.x] = s[0];
}

// Exclusive scan of the nb workgroup sums in place (one workgroup, 1024 at a time) and their total.
__global__ __launch_bounds__(1024) void rt_grid_scan_top_kernel(uint64_t *__restrict__ bsum, int nb,
                                                                uint64_t *__restrict__ total)
{
    __shared__ uint64_t s[1024];
    __shared__ uint64_t carry;
    const int tid = (int)threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + tid;
        const uint64_t v = i < nb ? bsum[i] : 0ull;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const uint64_t t = tid >= d ? s[tid - d] : 0ull;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        const uint64_t c = carry;
        if (i < nb) bsum[i] = c + s[tid] - v;
        __syncthreads();
        if (tid == 1023) carry = c + s[1023];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// out[i] = the sum of in[0 .. i), out[N] = the total.  in and out may be the same array (a thread
// reads its four elements before it writes them).  CELLS: in is the per-cell count, which becomes
// the fill's cursor (0), and cells longer than kSortSmall are listed for the long sort.
template <typename T, typename O, bool CELLS>
__global__ __launch_bounds__(kGridThreads) void rt_grid_scan_down_kernel(T *in, uint64_t N, const uint64_t *__restrict__ bsum,
                                                                         O *out, int *__restrict__ list, uint64_t list_cap,
                                                                         unsigned long long *__restrict__ nlong)
{
    __shared__ uint64_t s[kGridThreads];
    const int tid = (int)threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)tid * 4;
    uint64_t v[4], a = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = base + j < N ? (uint64_t)in[base + j] : 0ull;
        a += v[j];
    }
    s[tid] = a;
    __syncthreads();
    for (int d = 1; d < kGridThreads; d <<= 1) {
        const uint64_t t = tid >= d ? s[tid - d] : 0ull;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    uint64_t run = bsum[blockIdx.x] + s[tid] - a;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t i = base + j;
        if (i < N) {
            out[i] = (O)run;
            run += v[j];
            if (CELLS) {
                in[i] = 0;
                if (v[j] > (uint64_t)kSortSmall) {
                    const unsigned long long k = atomicAdd(nlong, 1ull);
                    if (k < list_cap) list[k] = (int)i;
                }
            }
            if (i == N - 1) out[N] = (O)run;
        }
    }
}

// The triangle of candidate g: coff[i] <= g < coff[i + 1] (coff ascending, coff[0] = 0, g < coff[n]).
__device__ __forceinline__ int cand_tri(const uint64_t *__restrict__ coff, int n, uint64_t g)
{
    int lo = 0, hi = n;
    for (int s = 0; s < 32 && hi - lo > 1; ++s) {
        const int mid = lo + ((hi - lo) >> 1);
        if (coff[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Candidate `local` of a triangle's packed range -> cell coordinates; false past the range.
__device__ __forceinline__ bool cand_cell(uint64_t r, uint64_t local, int &x, int &y, int &z)
{
    const int c0x = (int)(r & 1023), c0y = (int)(r >> 10 & 1023), c0z = (int)(r >> 20 & 1023);
    const int c1x = (int)(r >> 30 & 1023), c1y = (int)(r >> 40 & 1023), c1z = (int)(r >> 50 & 1023);
    if (c1x < c0x || c1y < c0y || c1z < c0z) return false;
    const unsigned nx = (unsigned)(c1x - c0x + 1), ny = (unsigned)(c1y - c0y + 1);
    if (local >= (uint64_t)nx * ny * (unsigned)(c1z - c0z + 1)) return false;
    const unsigned l = (unsigned)local;   // < 2^27
    x = c0x + (int)(l % nx);
    y = c0y + (int)(l / nx % ny);
    z = c0z + (int)(l / (nx * ny));
    return true;
}

// A thread per candidate pair: the FP64 separating-axis test, a count per cell, and the wave's
// verdicts as one word for the fill.  256 threads, 4 waves a SIMD wanted (<= 128 VGPRs): the test
// is FP64 arithmetic on 9 + 3 doubles with nothing to wait for but the triangle's load.
__global__ __launch_bounds__(kGridThreads) void rt_grid_count_kernel(const cg_tri *__restrict__ tris, int n,
                                                                     const uint64_t *__restrict__ coff,
                                                                     const uint64_t *__restrict__ rng, GridDims d,
                                                                     uint64_t B, int *__restrict__ cnt, uint64_t cells,
                                                                     unsigned long long *__restrict__ mask, uint64_t nmask)
{
    const uint64_t g = (uint64_t)blockIdx.x * kGridThreads + threadIdx.x;
    bool hit = false;
    if (g < B) {
        const int i = cand_tri(coff, n, g);
        int x, y, z;
        if (cand_cell(rng[i], g - coff[i], x, y, z)) {
            const cg_tri t = tris[i];
            const double v[3][3] = {{t.v0.x, t.v0.y, t.v0.z}, {t.v1.x, t.v1.y, t.v1.z}, {t.v2.x, t.v2.y, t.v2.z}};
            const double gh = d.h, hw = 0.5 * gh, eps = 1e-4 * gh;
            double c[3];
            grid_cell_centre(d.lo, gh, x, y, z, c);
            const uint64_t cell = ((uint64_t)z * d.res[1] + y) * d.res[0] + x;
            hit = cell < cells && tri_meets_cell(v, c, hw, eps);
            if (hit) atomicAdd(&cnt[cell], 1);
        }
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && (g >> 6) < nmask) mask[g >> 6] = m;
}

// A thread per candidate: the accepted ones take the next slot of their cell's segment.
__global__ __launch_bounds__(kGridThreads) void rt_grid_fill_kernel(int n, const uint64_t *__restrict__ coff,
                                                                    const uint64_t *__restrict__ rng, GridDims d, uint64_t B,
                                                                    const unsigned long long *__restrict__ mask,
                                                                    uint64_t nmask, const int *__restrict__ start,
                                                                    int *__restrict__ cur, uint64_t cells,
                                                                    int *__restrict__ out, uint64_t E)
{
    const uint64_t g = (uint64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (g >= B || (g >> 6) >= nmask) return;
    if (!(mask[g >> 6] >> (g & 63) & 1ull)) return;
    const int i = cand_tri(coff, n, g);
    int x, y, z;
    if (!cand_cell(rng[i], g - coff[i], x, y, z)) return;
    const uint64_t cell = ((uint64_t)z * d.res[1] + y) * d.res[0] + x;
    if (cell >= cells) return;
    const int k = atomicAdd(&cur[cell], 1);
    const int64_t pos = (int64_t)start[cell] + k;
    if (k >= 0 && pos >= 0 && pos < (int64_t)start[cell + 1] && (uint64_t)pos < E) out[pos] = i;
}

// Segments of 2 .. kSortSmall entries: a thread each, insertion sort in place.
__global__ __launch_bounds__(kGridThreads) void rt_grid_sort_small_kernel(const int *__restrict__ start, uint64_t cells,
                                                                          int *__restrict__ tris, uint64_t E)
{
    const uint64_t c = (uint64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (c >= cells) return;
    const int s = start[c], k = start[c + 1] - s;
    if (k < 2 || k > kSortSmall || s < 0 || (uint64_t)s + (uint64_t)k > E) return;
    int *a = tris + s;
    for (int i = 1; i < kSortSmall; ++i) {
        if (i >= k) break;
        const int x = a[i];
        int j = i;
        for (int q = 0; q < kSortSmall && j > 0; ++q) {
            const int y = a[j - 1];
            if (y <= x) break;
            a[j] = y;
            --j;
        }
        a[j] = x;
    }
}

// Bitonic network on a[0 .. k) by one workgroup, every compare-exchange ascending (the merge's
// first step mirrors, the rest are half-cleaners): entries k .. P - 1 of the padded power of two
// act as +infinity without being stored, since a pair reaching past k never swaps.
__device__ __forceinline__ void bitonic_sort(int *a, int k, int tid)
{
    unsigned P = 2;
    for (int s = 0; s < 31 && P < (unsigned)k; ++s) P <<= 1;
    const unsigned half = P >> 1;
    for (unsigned size = 2; size <= P; size <<= 1) {
        const unsigned hs = size >> 1;
        for (unsigned t = (unsigned)tid; t < half; t += kGridThreads) {
            const unsigned blk = t / hs, off = t % hs;
            const unsigned i = blk * size + off, j = blk * size + size - 1 - off;
            if (j < (unsigned)k) {
                const int x = a[i], y = a[j];
                if (x > y) {
                    a[i] = y;
                    a[j] = x;
                }
            }
        }
        __syncthreads();
        for (unsigned st = hs >> 1; st >= 1; st >>= 1) {
            for (unsigned t = (unsigned)tid; t < half; t += kGridThreads) {
                const unsigned i = (t / st) * 2 * st + t % st, j = i + st;
                if (j < (unsigned)k) {
                    const int x = a[i], y = a[j];
                    if (x > y) {
                        a[i] = y;
                        a[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Segments longer than kSortSmall: a workgroup per listed cell.
__global__ __launch_bounds__(kGridThreads) void rt_grid_sort_long_kernel(const int *__restrict__ list, uint64_t nlist,
                                                                         const int *__restrict__ start, uint64_t cells,
                                                                         int *tris, uint64_t E)
{
    __shared__ int lds[kSortLds];
    if (blockIdx.x >= nlist) return;
    const int c = list[blockIdx.x];
    if (c < 0 || (uint64_t)c >= cells) return;
    const int s = start[c], k = start[c + 1] - s;
    if (k <= kSortSmall || s < 0 || (uint64_t)s + (uint64_t)k > E) return;   // uniform over the workgroup
    const int tid = (int)threadIdx.x;
    if (k <= kSortLds) {
        for (int i = tid; i < k; i += kGridThreads) lds[i] = tris[s + i];
        __syncthreads();
        bitonic_sort(lds, k, tid);
        for (int i = tid; i < k; i += kGridThreads) tris[s + i] = lds[i];
    } else {
        bitonic_sort(tris + s, k, tid);
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

bool rt_grid_dims(const float vmin[3], const float vmax[3], int n, GridDims &d)
{
    std::memset(&d, 0, sizeof d);
    if (n <= 0) return false;
    float lo[3], hi[3];
    double ext[3], vol = 1.0;
    for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(FLT_MAX, vmin[a]);     // the host's accumulators start at +-FLT_MAX
        hi[a] = std::max(-FLT_MAX, vmax[a]);
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return false;
        lo[a] -= 1e-4f;
        hi[a] += 1e-4f;
        ext[a] = (double)hi[a] - lo[a];
        vol *= ext[a];
    }
    double h = 0.5 * std::cbrt(vol / std::max(1.0, n / 2.0));
    for (int a = 0; a < 3; ++a) h = std::max(h, ext[a] / 512.0);
    for (int a = 0; a < 3; ++a) {
        d.lo[a] = lo[a];
        const double q = std::ceil(ext[a] / h);   // 1 .. 512; a NaN (all extents 0) gives 1
        d.res[a] = q >= 512.0 ? 512 : (q >= 1.0 ? (int)q : 1);
    }
    d.h = (float)h;
    d.inv_h = (float)(1.0 / h);
    return true;
}

static hipError_t grid_events(GridBuild &gb)
{
    for (Event &e : gb.ev) {
        const hipError_t r = e.ensure(hipEventDefault);   // timing events
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}

#define GRID_TRY(call)                       \
    do {                                     \
        const hipError_t e_ = (call);        \
        if (e_ != hipSuccess) return e_;     \
    } while (0)

// mem[0]: bounds partials [kBoundsBlocks][8], the seven results, four 64-bit totals
static float *small_part(GridBuild &gb) { return (float *)gb.mem[0].p; }
static float *small_out(GridBuild &gb) { return (float *)gb.mem[0].p + kBoundsBlocks * 8; }
static unsigned long long *small_totals(GridBuild &gb)
{
    return (unsigned long long *)((char *)gb.mem[0].p + kBoundsBlocks * 8 * 4 + 64);
}

hipError_t rt_grid_bounds_device(GridBuild &gb, const cg_tri *d_tris, int n, SceneBounds &out, hipStream_t st)
{
    out = SceneBounds{};
    gb.phase_live = 0;
    gb.cells = gb.entries = gb.cands = 0;
    if (n <= 0) return hipSuccess;
    GRID_TRY(grid_events(gb));
    GRID_TRY(gb.mem[0].ensure((size_t)kBoundsBlocks * 8 * 4 + 64 + 64));
    const int nb = std::min(kBoundsBlocks, (n + kGridThreads - 1) / kGridThreads);
    GRID_TRY(hipEventRecord(gb.ev[0], st));
    hipLaunchKernelGGL(rt_grid_bounds_kernel, dim3(nb), dim3(kGridThreads), 0, st, d_tris, n, small_part(gb));
    hipLaunchKernelGGL(rt_grid_bounds_final_kernel, dim3(1), dim3(kGridThreads), 0, st, small_part(gb), nb,
                       small_out(gb));
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipEventRecord(gb.ev[1], st));
    float h[7];
    GRID_TRY(hipMemcpyAsync(h, small_out(gb), sizeof h, hipMemcpyDeviceToHost, st));
    GRID_TRY(hipStreamSynchronize(st));
    gb.phase_live |= 1u;
    for (int a = 0; a < 3; ++a) {
        out.vmin[a] = h[a];
        out.vmax[a] = h[3 + a];
    }
    out.nmax = h[6];
    return hipSuccess;
}

hipError_t rt_grid_build_device(GridBuild &gb, const cg_tri *d_tris, int n, const GridDims &d, uint64_t max_entries,
                                uint64_t max_cands, const std::function<hipError_t(int, size_t, void **)> &ensure,
                                bool &built, hipStream_t st)
{
    built = false;
    if (n <= 0) return hipSuccess;
    GRID_TRY(grid_events(gb));
    GRID_TRY(gb.mem[0].ensure((size_t)kBoundsBlocks * 8 * 4 + 64 + 64));
    const uint64_t cells = (uint64_t)d.res[0] * d.res[1] * d.res[2];
    const uint64_t N = (uint64_t)n;
    const int nbT = (int)((N + kScanTile - 1) / kScanTile), nbC = (int)((cells + kScanTile - 1) / kScanTile);
    gb.cells = cells;
    // mem[1]: rng[n], coff[n + 1], the scans' workgroup sums, the per-cell count / cursor
    size_t off = 0;
    const size_t o_rng = off; off = align256(off + N * 8);
    const size_t o_coff = off; off = align256(off + (N + 1) * 8);
    const size_t o_bsT = off; off = align256(off + (size_t)nbT * 8);
    const size_t o_bsC = off; off = align256(off + (size_t)nbC * 8);
    const size_t o_cnt = off; off = align256(off + cells * 4);
    GRID_TRY(gb.mem[1].ensure(off));
    char *m1 = (char *)gb.mem[1].p;
    uint64_t *rng = (uint64_t *)(m1 + o_rng), *coff = (uint64_t *)(m1 + o_coff);
    uint64_t *bsT = (uint64_t *)(m1 + o_bsT), *bsC = (uint64_t *)(m1 + o_bsC);
    int *cnt = (int *)(m1 + o_cnt);
    unsigned long long *tot = small_totals(gb);   // [0] B, [1] E, [2] long cells
    void *p_start = nullptr;
    GRID_TRY(ensure(0, (cells + 1) * 4, &p_start));
    int *start = (int *)p_start;

    // ranges
    GRID_TRY(hipEventRecord(gb.ev[2], st));
    GRID_TRY(hipMemsetAsync(tot, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(rt_grid_ranges_kernel, dim3((n + kGridThreads - 1) / kGridThreads), dim3(kGridThreads), 0, st,
                       d_tris, n, d, rng, coff);
    hipLaunchKernelGGL(rt_grid_scan_sums_kernel<uint64_t>, dim3(nbT), dim3(kGridThreads), 0, st, coff, N, bsT);
    hipLaunchKernelGGL(rt_grid_scan_top_kernel, dim3(1), dim3(1024), 0, st, bsT, nbT, (uint64_t *)&tot[0]);
    hipLaunchKernelGGL((rt_grid_scan_down_kernel<uint64_t, uint64_t, false>), dim3(nbT), dim3(kGridThreads), 0, st, coff,
                       N, bsT, coff, (int *)nullptr, (uint64_t)0, (unsigned long long *)nullptr);
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipEventRecord(gb.ev[3], st));
    unsigned long long h_tot[4] = {};
    GRID_TRY(hipMemcpyAsync(h_tot, tot, sizeof h_tot, hipMemcpyDeviceToHost, st));
    GRID_TRY(hipStreamSynchronize(st));
    gb.phase_live |= 2u;
    const uint64_t B = h_tot[0];
    gb.cands = B;
    if (B > max_cands) return hipSuccess;   // declined: too many candidate pairs to test

    // count
    const uint64_t nmask = (B + 63) / 64;
    const uint64_t list_cap = std::min<uint64_t>(cells, B / (kSortSmall + 1) + 1);
    const size_t o_list = align256(std::max<uint64_t>(nmask, 1) * 8);
    GRID_TRY(gb.mem[2].ensure(o_list + align256(list_cap * 4)));
    unsigned long long *mask = (unsigned long long *)gb.mem[2].p;
    int *list = (int *)((char *)gb.mem[2].p + o_list);
    const unsigned cblocks = (unsigned)((B + kGridThreads - 1) / kGridThreads);
    GRID_TRY(hipEventRecord(gb.ev[4], st));
    GRID_TRY(hipMemsetAsync(cnt, 0, cells * 4, st));
    if (cblocks)
        hipLaunchKernelGGL(rt_grid_count_kernel, dim3(cblocks), dim3(kGridThreads), 0, st, d_tris, n, coff, rng, d, B, cnt,
                           cells, mask, nmask);
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipEventRecord(gb.ev[5], st));

    // offsets
    GRID_TRY(hipEventRecord(gb.ev[6], st));
    hipLaunchKernelGGL(rt_grid_scan_sums_kernel<int>, dim3(nbC), dim3(kGridThreads), 0, st, cnt, cells, bsC);
    hipLaunchKernelGGL(rt_grid_scan_top_kernel, dim3(1), dim3(1024), 0, st, bsC, nbC, (uint64_t *)&tot[1]);
    hipLaunchKernelGGL((rt_grid_scan_down_kernel<int, int, true>), dim3(nbC), dim3(kGridThreads), 0, st, cnt, cells, bsC,
                       start, list, list_cap, &tot[2]);
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipEventRecord(gb.ev[7], st));
    GRID_TRY(hipMemcpyAsync(h_tot, tot, sizeof h_tot, hipMemcpyDeviceToHost, st));
    GRID_TRY(hipStreamSynchronize(st));
    gb.phase_live |= 4u | 8u;
    const uint64_t E = h_tot[1], nlong = std::min<uint64_t>(h_tot[2], list_cap);
    gb.entries = E;
    if (E > max_entries || E > (uint64_t)INT_MAX) return hipSuccess;   // declined: the lists would be too long

    // fill and order
    void *p_tris = nullptr;
    GRID_TRY(ensure(1, std::max<uint64_t>(E, 1) * 4, &p_tris));
    int *out = (int *)p_tris;
    GRID_TRY(hipEventRecord(gb.ev[8], st));
    if (cblocks && E)
        hipLaunchKernelGGL(rt_grid_fill_kernel, dim3(cblocks), dim3(kGridThreads), 0, st, n, coff, rng, d, B, mask, nmask,
                           start, cnt, cells, out, E);
    if (E > 1)
        hipLaunchKernelGGL(rt_grid_sort_small_kernel, dim3((unsigned)((cells + kGridThreads - 1) / kGridThreads)),
                           dim3(kGridThreads), 0, st, start, cells, out, E);
    if (nlong)
        hipLaunchKernelGGL(rt_grid_sort_long_kernel, dim3((unsigned)nlong), dim3(kGridThreads), 0, st, list, nlong, start,
                           cells, out, E);
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipEventRecord(gb.ev[9], st));
    gb.phase_live |= 16u;
    built = true;
    return hipSuccess;
}

size_t rt_grid_scratch_bytes(const GridBuild &gb) { return gb.mem[0].bytes + gb.mem[1].bytes + gb.mem[2].bytes; }

hipError_t rt_grid_phase_ms(GridBuild &gb, double out[kGridPhases])
{
    for (int p = 0; p < kGridPhases; ++p) {
        out[p] = -1.0;
        if (!(gb.phase_live >> p & 1u)) continue;
        GRID_TRY(hipEventSynchronize(gb.ev[2 * p + 1]));
        float ms = 0.f;
        GRID_TRY(hipEventElapsedTime(&ms, gb.ev[2 * p], gb.ev[2 * p + 1]));
        out[p] = ms;
    }
    return hipSuccess;
}

}  // namespace cg
