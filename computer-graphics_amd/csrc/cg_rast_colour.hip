// cg_rast_colour.hip -- rasteriser colour modes 1-2 (randColourSelect,
// rasteriser/Source/skeleton.cpp:647-662): every fragment PixelShader shades
// takes three glibc rand() values, in the reference's fragment order --
// triangle by triangle (:262-281), row by row (:500-508), left to right.
// Which fragments shade depends on the z-buffer at that moment, so the order
// is reconstructed exactly:
//   rast_count_kernel      one wave per row, the ordered z-buffer walk of the
//                          fill: shaded fragments per (triangle, row);
//   rast_scan_rows_kernel  per triangle, exclusive prefix over its rows;
//   rast_scan_tris_kernel  exclusive prefix over triangles (and the total S);
//   rast_rand_kernel       the frame's 3 S rand() values (cg_glibc_rand.h,
//                          jump-ahead to the frame's call offset);
//   rast_fill_rand_kernel  the same walk again, each shaded fragment numbered
//                          (base of its (triangle, row) + rank in the row), the
//                          last one per pixel shaded with its three values.
// The post-pass is shared with colour mode 0 (kStateDirect state).
//
// A frame sequence (cg_rast_draw_sequence_device) chains the call index on the
// device instead of on the host, with nothing read back:
//   rast_seq_chain_kernel  frame f's record {offset_f, S_f, status_f} and
//                          offset_{f+1} = offset_f + 3 S_f;
//   rast_seq_seek_kernel   the 61-word window at offset_f: x^(offset_f + 341)
//                          mod P by square-and-multiply in one wave;
//   rast_rand_dev_kernel   rast_rand_kernel with the window and the length
//                          read from device memory, launched over the chunks
//                          of the stream's capacity.
#include <vector>

#include "cg_glibc_rand.h"
#include "cg_host.h"
#include "cg_rast_dev.h"

namespace cg {

constexpr int kRandChunk = 31 * 32;    // rand() values per generator thread

// The row's records (lane q holds record base + q) overlapping [x0, x0 + 63].
struct RecLane {
    int lx, rx, shd;
    float lz, sz;
    bool ov;
};
__device__ __forceinline__ RecLane rec_lane(const RowRec *rr, int q, int cnt, int x0)
{
    RecLane r{0, 0, 0, 0.f, 0.f, false};
    if (q < cnt) {
        const RowRec &m = rr[q];
        r.lx = m.lx; r.rx = m.rx; r.lz = m.lz; r.sz = m.sz; r.shd = rec_shadow(m);
        r.ov = !(r.rx - 1 < x0 || r.lx > x0 + 63);
    }
    return r;
}

__global__ __launch_bounds__(64) void rast_count_kernel(RastArgs A, const RowRec *__restrict__ recs,
                                                       const int *__restrict__ count, int *__restrict__ pc)
{
    extern __shared__ int s_cnt[];                        // per record of the row
    const int y = blockIdx.x, lane = threadIdx.x;
    if (y >= A.H) return;
    const int cnt = count[y];
    const RowRec *rr = recs + (size_t)y * A.n;
    for (int i = lane; i < cnt; i += 64) s_cnt[i] = 0;
    __syncthreads();
    for (int x0 = 0; x0 < A.W; x0 += 64) {
        const int x = x0 + lane;
        float depth = 0.0f;                               // :247
        for (int base = 0; base < cnt; base += 64) {
            const RecLane R = rec_lane(rr, base + lane, cnt, x0);
            unsigned long long m = __ballot(R.ov && !R.shd);   // shadow triangles never shade
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1ull;
                const int lx = __builtin_amdgcn_readlane(R.lx, b), rx = __builtin_amdgcn_readlane(R.rx, b);
                const float lz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(R.lz), b));
                const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(R.sz), b));
                const int i = x - lx;
                const bool in = x < A.W && i >= 0 && x < rx;             // :504, :573
                const float zinv = lz + (sz * (float)i);                 // :543
                const bool pass = in && zinv >= depth;                   // :574
                if (pass) depth = zinv;                                  // :665
                const unsigned long long pm = __ballot(pass);
                if (lane == 0 && pm) s_cnt[base + b] += __popcll(pm);
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < cnt; i += 64) pc[(size_t)rec_t(rr[i]) * A.H + y] = s_cnt[i];
}

// block-wide inclusive scan of v (256 threads); `total` = the block's sum
__device__ __forceinline__ long long block_scan256(long long v, long long &total, long long *s_w)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    long long before = 0;
    total = 0;
    for (int q = 0; q < 4; ++q) {
        const long long x = s_w[q];
        before += q < w ? x : 0;
        total += x;
    }
    __syncthreads();
    return v + before;
}

// per triangle: exclusive prefix of its shaded-fragment counts over its rows
__global__ __launch_bounds__(256) void rast_scan_rows_kernel(const RastHdr *__restrict__ hdr, const int *n_dev,
                                                           int n_cap, int H, int *__restrict__ pc,
                                                           long long *__restrict__ tot)
{
    __shared__ long long s_w[4];
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        const RastHdr h = hdr[t];
        long long carry = 0;
        for (int y0 = h.ylo; y0 <= h.yhi; y0 += 256) {
            const int y = y0 + (int)threadIdx.x;
            const long long v = y <= h.yhi ? pc[(size_t)t * H + y] : 0;
            long long chunk;
            const long long inc = block_scan256(v, chunk, s_w);
            if (y <= h.yhi) pc[(size_t)t * H + y] = (int)(carry + inc - v);
            carry += chunk;
        }
        if (threadIdx.x == 0) tot[t] = carry;
    }
}

// exclusive prefix over triangles; total[0] = S, the frame's shaded fragments
__global__ __launch_bounds__(256) void rast_scan_tris_kernel(const long long *__restrict__ tot, const int *n_dev,
                                                           int n_cap, long long *__restrict__ tbase,
                                                           long long *__restrict__ total)
{
    __shared__ long long s_w[4];
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap;
    long long carry = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        const long long v = t < n ? tot[t] : 0;
        long long chunk;
        const long long inc = block_scan256(v, chunk, s_w);
        if (t < n) tbase[t] = carry + inc - v;
        carry += chunk;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// The 61 state words at the frame's first rand() call (cg_glibc_rand.h).
struct RandWindow {
    uint32_t w[61];
};

// Values [b C, (b + 1) C) of a stream whose window is w: the chunk's window
// r[idx + b C + j] = sum_i J_b[i] w[i + j] (J_b = x^(b C) mod P), then the
// recurrence r[i] = r[i - 31] + r[i - 3], 31 values per round in registers.
template <class Win>   // the 61 window words, indexable
__device__ __forceinline__ void rand_chunk(const Win &w, const uint32_t *__restrict__ jt, int b, long long nvals,
                                           int32_t *__restrict__ out)
{
    uint32_t o[kRandDeg];
#pragma unroll
    for (int j = 0; j < kRandDeg; ++j) o[j] = 0u;
    for (int i = 0; i < kRandDeg; ++i) {
        const uint32_t c = jt[(size_t)b * kRandDeg + i];
#pragma unroll
        for (int j = 0; j < kRandDeg; ++j) o[j] += c * w[i + j];
    }
    const long long p0 = (long long)b * kRandChunk;
    for (int m0 = 0; m0 < kRandChunk; m0 += kRandDeg) {
#pragma unroll
        for (int j = 0; j < kRandDeg; ++j)
            if (p0 + m0 + j < nvals) out[p0 + m0 + j] = (int32_t)(o[j] >> 1);      // rand() = r >> 1
        uint32_t nn[kRandDeg];
#pragma unroll
        for (int j = 0; j < kRandDeg; ++j) nn[j] = o[j] + (j < 3 ? o[28 + j] : nn[j - 3]);
#pragma unroll
        for (int j = 0; j < kRandDeg; ++j) o[j] = nn[j];
    }
}

// Thread b produces values [b C, (b + 1) C) of the frame's stream.
__global__ __launch_bounds__(256) void rast_rand_kernel(RandWindow W, const uint32_t *__restrict__ jt, int nb,
                                                      long long nvals, int32_t *__restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    rand_chunk(W.w, jt, b, nvals, out);
}

// ---- frame sequences: the chain, the seek and the generator on the device ----

// Word offsets in the context's generator tables (rast_seq_tables): the
// sequence's window, the probe's window (cg_glibc_rand_device), the seed-1
// state words r[3 .. 94], then J_b for every chunk of the capacity.
constexpr int kSeqWin = 0, kSeqProbeWin = 64, kSeqSeed = 128, kSeqJump = 224;

// Frame f's record and the next frame's start: info[0] = {offset_f, S_f,
// status_f}, info[1] = {offset_f + 3 S_f, -1, 0} (the closing record after the
// last frame).  offset_f is `start` for the call's first frame, else what the
// previous frame's step left in info[0].  mode 0: no fragments draw, S = -1.
__global__ __launch_bounds__(64) void rast_seq_chain_kernel(const long long *__restrict__ total,
                                                          cg_rast_seq_frame *info, int first,
                                                          unsigned long long start, long long cap, int mode)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long off = first ? start : (unsigned long long)info[0].rand_offset;
    const long long S = mode != 0 ? total[0] : -1;
    cg_rast_seq_frame cur, next;
    cur.rand_offset = off;
    cur.n_shaded = S;
    cur.status = S > cap ? CG_E_CAPACITY : 0;
    cur.pad = 0;
    next.rand_offset = off + (S > 0 ? 3ull * (unsigned long long)S : 0ull);
    next.n_shaded = -1;
    next.status = 0;
    next.pad = 0;
    info[0] = cur;
    info[1] = next;
}

// c = a b mod P in one wave: lane i holds coefficient i (lanes >= 31 hold 0).
// s_b is b at [31, 62) between zeros, so lane k sums a_i b_(k - i) over every
// i without a bounds test; the 61-term product goes to s_t (zeros above it)
// and x^k = x^(k - 3) + x^(k - 31), k = 60 .. 31, folds to
//   c_i = t_i + h'_i + (i >= 28 ? h'_(i - 28) : 0),  h'_m = sum_r t_(31 + m + 3 r)
// (rand_poly_mulmod's loop, summed per coefficient).
__device__ __forceinline__ uint32_t rand_poly_mulmod_wave(uint32_t a, uint32_t b, uint32_t *s_b, uint32_t *s_t,
                                                          int lane)
{
    __syncthreads();
    s_b[kRandDeg + lane] = b;
    __syncthreads();
    uint32_t t = 0u;
#pragma unroll
    for (int i = 0; i < kRandDeg; ++i)
        t += (uint32_t)__builtin_amdgcn_readlane((int)a, i) * s_b[kRandDeg + lane - i];
    s_t[lane] = t;                                        // lanes 61-63: 0
    __syncthreads();
    uint32_t h = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) h += s_t[kRandDeg + lane + 3 * r];
    const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)h, 0), h1 = (uint32_t)__builtin_amdgcn_readlane((int)h, 1),
                   h2 = (uint32_t)__builtin_amdgcn_readlane((int)h, 2);
    const uint32_t c = t + h + (lane == 28 ? h0 : lane == 29 ? h1 : lane == 30 ? h2 : 0u);
    return lane < kRandDeg ? c : 0u;
}

// The 61 state words at call index *d_off (rand_window on the device): one
// wave, x^(k + 341) mod P by square-and-multiply (rand_poly_xpow), applied to
// seed[j] = r[3 + j], j < 92.  skip: the frame's status (non-zero: nothing to do).
__global__ __launch_bounds__(64) void rast_seq_seek_kernel(const unsigned long long *__restrict__ d_off,
                                                         const int32_t *__restrict__ skip,
                                                         const uint32_t *__restrict__ seed,
                                                         uint32_t *__restrict__ win)
{
    __shared__ uint32_t s_b[128], s_t[128];
    const int lane = threadIdx.x;
    if (skip && *skip != 0) return;
    s_b[lane] = 0u; s_b[64 + lane] = 0u;
    s_t[lane] = 0u; s_t[64 + lane] = 0u;
    const unsigned long long k = *d_off + 344ull - 3ull;
    uint32_t elo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)k);
    uint32_t ehi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(k >> 32));
    uint32_t res = lane == 0 ? 1u : 0u, base = lane == 1 ? 1u : 0u;
    while (elo | ehi) {
        if (elo & 1u) res = rand_poly_mulmod_wave(res, base, s_b, s_t, lane);
        elo = (elo >> 1) | (ehi << 31);
        ehi >>= 1;
        if (elo | ehi) base = rand_poly_mulmod_wave(base, base, s_b, s_t, lane);
    }
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < kRandDeg; ++i) {
        const int j = i + lane < 92 ? i + lane : 91;
        v += (uint32_t)__builtin_amdgcn_readlane((int)res, i) * seed[j];
    }
    if (lane < 61) win[lane] = v;
}

// rast_rand_kernel with the window and the stream's length in device memory:
// launched over the nb_cap chunks of the capacity, chunks past the length exit
// at once.  info: the frame's record (3 n_shaded values; a non-zero status
// generates nothing); null: nfixed values (the probe).
__global__ __launch_bounds__(256) void rast_rand_dev_kernel(const uint32_t *__restrict__ win,
                                                          const cg_rast_seq_frame *__restrict__ info,
                                                          long long nfixed, const uint32_t *__restrict__ jt,
                                                          int nb_cap, int32_t *__restrict__ out)
{
    __shared__ uint32_t s_w[64];                          // every thread reads the same word: LDS broadcasts
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (info && info->status != 0) return;
    const long long nvals = info ? 3 * info->n_shaded : nfixed;
    if ((long long)blockIdx.x * blockDim.x * kRandChunk >= nvals) return;   // the whole workgroup
    if (threadIdx.x < 61) s_w[threadIdx.x] = win[threadIdx.x];
    __syncthreads();
    if (b >= nb_cap || (long long)b * kRandChunk >= nvals) return;
    const uint32_t *w = s_w;
    rand_chunk(w, jt, b, nvals, out);
}

__global__ __launch_bounds__(64) void rast_fill_rand_kernel(RastArgs A0, const RowRec *__restrict__ recs,
                                                          const int *__restrict__ count, const int *__restrict__ pc,
                                                          const long long *__restrict__ tbase,
                                                          const int32_t *__restrict__ rnd, int mode,
                                                          float4 *__restrict__ state, float *__restrict__ depth_out,
                                                          int32_t *__restrict__ shadow_out,
                                                          const cg_rast_seq_frame *__restrict__ info)
{
    extern __shared__ long long s_run[];                  // next fragment number per record
    const RastArgs A = with_device_light(A0);
    const int y = blockIdx.x, lane = threadIdx.x;
    if (y >= A.H) return;
    if (info && info->status != 0) return;                // sequence frame over the capacity: planes untouched
    const int cnt = count[y];
    const RowRec *rr = recs + (size_t)y * A.n;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int i = lane; i < cnt; i += 64) {
        const int t = rec_t(rr[i]);
        s_run[i] = tbase[t] + pc[(size_t)t * A.H + y];
    }
    __syncthreads();
    for (int x0 = 0; x0 < A.W; x0 += 64) {
        const int x = x0 + lane;
        float depth = 0.0f;                               // :247
        int shadow = 0, win = -1;                         // :259
        long long widx = 0;
        for (int base = 0; base < cnt; base += 64) {
            const RecLane R = rec_lane(rr, base + lane, cnt, x0);
            unsigned long long m = __ballot(R.ov);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1ull;
                const int lx = __builtin_amdgcn_readlane(R.lx, b), rx = __builtin_amdgcn_readlane(R.rx, b);
                const float lz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(R.lz), b));
                const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(R.sz), b));
                const int shd = __builtin_amdgcn_readlane(R.shd, b);
                const int i = x - lx;
                const bool in = x < A.W && i >= 0 && x < rx;             // :504, :573
                const float zinv = lz + (sz * (float)i);                 // :543
                if (!shd) {
                    const bool pass = in && zinv >= depth;               // :574
                    const unsigned long long pm = __ballot(pass);
                    if (pm) {
                        const long long run = s_run[base + b];
                        if (pass) {
                            depth = zinv;                                // :665
                            win = base + b;
                            widx = run + __popcll(pm & lt);
                        }
                        if (lane == 0) s_run[base + b] = run + __popcll(pm);
                    }
                } else if (in && zinv > depth) {                         // :668-669
                    shadow = 1;
                }
            }
        }
        if (x < A.W) {
            float4 st = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
            if (win >= 0) {
                const RowRec r = rr[win];
                const int i = x - r.lx;
                const float X = r.lX + (r.sX * (float)i);                // :547-548 numerators
                const float Y = r.lY + (r.sY * (float)i);
                const cg_vec4 tn = A.tris[rec_t(r)].normal;
                const vec3 D = illum_D(A, depth, X, Y, v3(tn.x, tn.y, tn.z));
                const float r0 = rand_unit(rnd[3 * widx]), r1 = rand_unit(rnd[3 * widx + 1]),
                            r2 = rand_unit(rnd[3 * widx + 2]);
                const vec3 rc = mode == 1 ? v3(r0, r1, r2) : v3(r0 - 0.2f, 1.0f, r2 - 0.2f);   // :652 / :660
                const float ind = A.ind_first;                           // modes 1-2 never rewrite it
                const vec3 sc = rc * (D + v3(ind, ind, ind));
                st = make_float4(__int_as_float(kStateDirect), sc.x, sc.y, sc.z);
            }
            const size_t o = (size_t)y * A.W + x;
            state[o] = st;
            if (depth_out) depth_out[o] = depth;
            shadow_out[o] = shadow;
        }
    }
}

// J_b = x^(b C) mod P for b < nb, grown once per process as callers need more
static const std::vector<uint32_t> &rand_jump_table(long long nb)
{
    static std::vector<uint32_t> jtab;
    static uint32_t step[kRandDeg];
    if (jtab.empty()) {
        rand_poly_xpow(kRandChunk, step);
        jtab.assign(kRandDeg, 0u);
        jtab[0] = 1u;
    }
    while ((long long)(jtab.size() / kRandDeg) < nb) {
        uint32_t next[kRandDeg];
        rand_poly_mulmod(&jtab[jtab.size() - kRandDeg], step, next);
        jtab.insert(jtab.end(), next, next + kRandDeg);
    }
    return jtab;
}

// The 3 S rand() values of a frame whose first call has index `offset`, generated on `st` into
// the context's buffer rnd_buf (the jump table into jt_buf; both sized by S).  The upload reads
// the process's jump table from host memory: the caller synchronises `st` before it returns.
int rast_rand_stream(cg_ctx *c, int rnd_buf, int jt_buf, uint64_t offset, long long S, hipStream_t st, int32_t **out)
{
    hipError_t e;
    const long long nvals = 3 * S;
    const int nb = (int)((nvals + kRandChunk - 1) / kRandChunk);
    int32_t *rnd = (int32_t *)ctx_buf(c, rnd_buf, (size_t)(nvals > 0 ? nvals : 1) * sizeof(int32_t), &e);
    if (!rnd) return ctx_fail(c, e, "alloc rand stream");
    if (nb > 0) {
        const std::vector<uint32_t> &jtab = rand_jump_table(nb);
        uint32_t *jt = (uint32_t *)ctx_buf(c, jt_buf, (size_t)nb * kRandDeg * sizeof(uint32_t), &e);
        if (!jt) return ctx_fail(c, e, "alloc jump table");
        if ((e = hipMemcpyAsync(jt, jtab.data(), (size_t)nb * kRandDeg * sizeof(uint32_t), hipMemcpyHostToDevice, st)) !=
            hipSuccess)
            return ctx_fail(c, e, "upload jump table");
        RandWindow W;
        rand_window(offset, W.w);
        hipLaunchKernelGGL(rast_rand_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, W, jt, nb, nvals, rnd);
        if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rand generator launch");
    }
    *out = rnd;
    return CG_OK;
}

// Host side of colour modes 1-2, between rast_rows_kernel and the post-pass.
// Synchronises once (the stream's length S decides the generator's size).
int rast_colour_fill(cg_ctx *c, const RastArgs &A, const cg_rast_params *p, const RowRec *recs, const int *count,
                     const RastHdr *hdr, const int *n_dev, int max_recs, float4 *state, float *d_depth,
                     int32_t *shadow, hipStream_t st, long long *n_shaded)
{
    hipError_t e;
    const int n = A.n > 0 ? A.n : 1, H = A.H;
    int *pc = (int *)ctx_buf(c, kBufPc, (size_t)n * H * sizeof(int), &e);
    if (!pc) return ctx_fail(c, e, "alloc pass counts");
    long long *tl = (long long *)ctx_buf(c, kBufTl, (2 * (size_t)n + 2) * sizeof(long long), &e);
    if (!tl) return ctx_fail(c, e, "alloc triangle counts");
    long long *tot = tl, *tbase = tl + n, *total = tl + 2 * n;
    if ((e = hipMemsetAsync(pc, 0, (size_t)n * H * sizeof(int), st)) != hipSuccess) return ctx_fail(c, e, "memset");
    const size_t lds_cnt = (size_t)(max_recs > 0 ? max_recs : 1) * sizeof(int);
    hipLaunchKernelGGL(rast_count_kernel, dim3(H), dim3(64), lds_cnt, st, A, recs, count, pc);
    hipLaunchKernelGGL(rast_scan_rows_kernel, dim3(n < 1024 ? n : 1024), dim3(256), 0, st, hdr, n_dev, A.n, H, pc,
                       tot);
    hipLaunchKernelGGL(rast_scan_tris_kernel, dim3(1), dim3(256), 0, st, tot, n_dev, A.n, tbase, total);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "colour count launch");
    long long S = 0;
    if ((e = hipMemcpyAsync(&S, total, sizeof(S), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return ctx_fail(c, e, "shaded-fragment count");
    *n_shaded = S;
    int32_t *rnd = nullptr;
    if (const int rc = rast_rand_stream(c, kBufRnd, kBufJt, p->rand_offset, S, st, &rnd)) return rc;
    hipLaunchKernelGGL(rast_fill_rand_kernel, dim3(H), dim3(64), (size_t)(max_recs > 0 ? max_recs : 1) * 8, st, A,
                       recs, count, pc, tbase, rnd, p->colour_mode, state, d_depth, shadow,
                       (const cg_rast_seq_frame *)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "colour fill launch");
    // the jump table upload reads host memory: keep it alive until the copy ran
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return ctx_fail(c, e, "colour fill");
    return CG_OK;
}

// The context's generator tables with J_b for nb chunks (kSeqWin ..): built
// and uploaded when a call needs more chunks than *have holds (first use of a
// capacity; synchronous), untouched otherwise.
int rast_seq_tables(cg_ctx *c, long long nb, long long *have, uint32_t **tables)
{
    hipError_t e;
    const size_t words = (size_t)kSeqJump + (size_t)(nb > *have ? nb : *have) * kRandDeg;
    uint32_t *t = (uint32_t *)ctx_buf(c, kBufSeq, words * sizeof(uint32_t), &e);
    if (!t) return ctx_fail(c, e, "alloc generator tables");
    *tables = t;
    if (nb <= *have) return CG_OK;
    *have = 0;
    const std::vector<uint32_t> &jtab = rand_jump_table(nb);
    const std::vector<uint32_t> r = rand_state_prefix(3 + 92);
    if ((e = hipMemcpy(t + kSeqSeed, r.data() + 3, 92 * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(t + kSeqJump, jtab.data(), (size_t)nb * kRandDeg * sizeof(uint32_t), hipMemcpyHostToDevice)) !=
            hipSuccess)
        return ctx_fail(c, e, "upload generator tables");
    *have = nb;
    return CG_OK;
}

// Colour modes 1-2 of a sequence frame, between rast_rows_kernel and the
// post-pass: rast_colour_fill with the chain, the seek and the generator's
// length on the device.  Enqueues only.
int rast_seq_colour_fill(cg_ctx *c, const RastArgs &A, const cg_rast_params *p, const RowRec *recs, const int *count,
                         const RastHdr *hdr, const int *n_dev, int max_recs, float4 *state, float *d_depth,
                         int32_t *shadow, hipStream_t st, const RastSeq &q)
{
    hipError_t e;
    const int n = A.n > 0 ? A.n : 1, H = A.H;
    int *pc = (int *)ctx_buf(c, kBufPc, (size_t)n * H * sizeof(int), &e);
    if (!pc) return ctx_fail(c, e, "alloc pass counts");
    long long *tl = (long long *)ctx_buf(c, kBufTl, (2 * (size_t)n + 2) * sizeof(long long), &e);
    if (!tl) return ctx_fail(c, e, "alloc triangle counts");
    int32_t *rnd = (int32_t *)ctx_buf(c, kBufRnd, 3 * (size_t)(q.cap > 0 ? q.cap : 1) * sizeof(int32_t), &e);
    if (!rnd) return ctx_fail(c, e, "alloc rand stream");
    long long *tot = tl, *tbase = tl + n, *total = tl + 2 * n;
    if ((e = hipMemsetAsync(pc, 0, (size_t)n * H * sizeof(int), st)) != hipSuccess) return ctx_fail(c, e, "memset");
    const size_t lds_cnt = (size_t)(max_recs > 0 ? max_recs : 1) * sizeof(int);
    hipLaunchKernelGGL(rast_count_kernel, dim3(H), dim3(64), lds_cnt, st, A, recs, count, pc);
    hipLaunchKernelGGL(rast_scan_rows_kernel, dim3(n < 1024 ? n : 1024), dim3(256), 0, st, hdr, n_dev, A.n, H, pc,
                       tot);
    hipLaunchKernelGGL(rast_scan_tris_kernel, dim3(1), dim3(256), 0, st, tot, n_dev, A.n, tbase, total);
    // everything above is offset-independent; from here on the frame follows its predecessor
    uint32_t *win = q.win ? q.win : q.tables + kSeqWin;
    if (q.wait_ev && (e = hipStreamWaitEvent(st, q.wait_ev, 0)) != hipSuccess) return ctx_fail(c, e, "chain wait");
    hipLaunchKernelGGL(rast_seq_chain_kernel, dim3(1), dim3(64), 0, st, (const long long *)total, q.info, q.first,
                       (unsigned long long)q.start, q.cap, 1);
    if (q.done_ev && (e = hipEventRecord(q.done_ev, st)) != hipSuccess) return ctx_fail(c, e, "chain event");
    hipLaunchKernelGGL(rast_seq_seek_kernel, dim3(1), dim3(64), 0, st,
                       (const unsigned long long *)&q.info->rand_offset, (const int32_t *)&q.info->status,
                       (const uint32_t *)(q.tables + kSeqSeed), win);
    if (q.nb_cap > 0)
        hipLaunchKernelGGL(rast_rand_dev_kernel, dim3((q.nb_cap + 255) / 256), dim3(256), 0, st,
                           (const uint32_t *)win, (const cg_rast_seq_frame *)q.info, 0ll,
                           (const uint32_t *)(q.tables + kSeqJump), q.nb_cap, rnd);
    hipLaunchKernelGGL(rast_fill_rand_kernel, dim3(H), dim3(64), (size_t)(max_recs > 0 ? max_recs : 1) * 8, st, A,
                       recs, count, pc, tbase, rnd, p->colour_mode, state, d_depth, shadow,
                       (const cg_rast_seq_frame *)q.info);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "sequence colour fill launch");
    return CG_OK;
}

// A colour mode 0 frame of a sequence: its record, the offset passed on unchanged.
int rast_seq_chain_mode0(cg_ctx *c, hipStream_t st, const RastSeq &q)
{
    hipError_t e;
    if (q.wait_ev && (e = hipStreamWaitEvent(st, q.wait_ev, 0)) != hipSuccess) return ctx_fail(c, e, "chain wait");
    hipLaunchKernelGGL(rast_seq_chain_kernel, dim3(1), dim3(64), 0, st, (const long long *)nullptr, q.info, q.first,
                       (unsigned long long)q.start, q.cap, 0);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "sequence chain launch");
    if (q.done_ev && (e = hipEventRecord(q.done_ev, st)) != hipSuccess) return ctx_fail(c, e, "chain event");
    return CG_OK;
}

// A colour mode 1-2 frame of a sequence on the compact route: its record from the frame's own
// fragment count *total (device).  The route sizes the stream by that count, so no capacity flags it.
int rast_seq_chain_exact(cg_ctx *c, hipStream_t st, const RastSeq &q, const long long *total)
{
    hipError_t e;
    if (q.wait_ev && (e = hipStreamWaitEvent(st, q.wait_ev, 0)) != hipSuccess) return ctx_fail(c, e, "chain wait");
    hipLaunchKernelGGL(rast_seq_chain_kernel, dim3(1), dim3(64), 0, st, total, q.info, q.first,
                       (unsigned long long)q.start, LLONG_MAX, 1);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "sequence chain launch");
    if (q.done_ev && (e = hipEventRecord(q.done_ev, st)) != hipSuccess) return ctx_fail(c, e, "chain event");
    return CG_OK;
}

// cg_glibc_rand_device: n values from the call index at d_off, by the seek and
// the generator of the sequence (their own window slot).
int rast_rand_probe(cg_ctx *c, uint32_t *tables, int nb, const uint64_t *d_off, int n, int32_t *d_out, hipStream_t st)
{
    hipLaunchKernelGGL(rast_seq_seek_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long *)d_off,
                       (const int32_t *)nullptr, (const uint32_t *)(tables + kSeqSeed), tables + kSeqProbeWin);
    hipLaunchKernelGGL(rast_rand_dev_kernel, dim3((nb + 255) / 256), dim3(256), 0, st,
                       (const uint32_t *)(tables + kSeqProbeWin), (const cg_rast_seq_frame *)nullptr, (long long)n,
                       (const uint32_t *)(tables + kSeqJump), nb, d_out);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? ctx_fail(c, e, "rand probe launch") : CG_OK;
}

long long rast_rand_chunks(long long nvals) { return (nvals + kRandChunk - 1) / kRandChunk; }

}  // namespace cg

// Host-only probe of the restated generator: n values of glibc rand() from
// call `offset` on (seed 1) -- what rast_rand_kernel produces on the device.
extern "C" int cg_glibc_rand(uint64_t offset, int n, int32_t *out)
{
    if (n < 0 || (n && !out)) return CG_E_INVALID;
    uint32_t w[61];
    cg::rand_window(offset, w);
    uint32_t r[cg::kRandDeg];
    for (int j = 0; j < cg::kRandDeg; ++j) r[j] = w[j];
    for (int k = 0; k < n; k += cg::kRandDeg) {
        for (int j = 0; j < cg::kRandDeg && k + j < n; ++j) out[k + j] = (int32_t)(r[j] >> 1);
        uint32_t nn[cg::kRandDeg];
        for (int j = 0; j < cg::kRandDeg; ++j) nn[j] = r[j] + (j < 3 ? r[28 + j] : nn[j - 3]);
        for (int j = 0; j < cg::kRandDeg; ++j) r[j] = nn[j];
    }
    return CG_OK;
}
