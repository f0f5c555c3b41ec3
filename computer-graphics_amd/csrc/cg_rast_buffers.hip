// cg_rast_buffers.hip -- the rasteriser's HDR shade buffers, owner ids and picking (gfx950):
// cg_rast_draw_buffers*, cg_rast_render_buffers*, cg_rast_pick.
//
// The reference's Draw leaves three float vec3 buffers behind besides the picture, the depth
// and the shadow marks (rasteriser/Source/skeleton.cpp:243-307): screenBuffer, lowLightBuffer,
// highLightBuffer.  A frame here computes them in its post-pass and keeps only the 8-bit
// picture.  One more kernel, queued after the frame's own, rebuilds them from what the frame
// left in context scratch -- the ordered z-buffer's state word per pixel (record + 1 | shadow
// mark) and the row records -- with the post-pass's own expressions (shade3c, illum_D,
// darken_at), and says which fragment owns each pixel: the last one that wrote
// screenBuffer[y][x] in drawing order (:574-661), as its clipped triangle, its input triangle
// and its pos3d (:546-549).
//
// Colour modes 1-2 never make state words (their fill keeps a colour per pixel); a buffers call
// has the route run the mode-0 fill once more for them (the owner does not depend on the colour
// mode: modes 1-2 ignore textures, :604), and `screen` comes from the colour fill's float4.
#include "cg_host.h"
#include "cg_rast_dev.h"

namespace cg {

typedef unsigned long long u64;

struct BufIn {
    const void *words;        // state words, 2 or 4 bytes (A.state16)
    const float4 *direct;     // colour modes 1-2: the colour fill's state
    const RowRec *recs;
    const u64 *row_off;       // compact route; null: row y's records at y * A.n
    u64 rec_cap;
    const u64 *pre;           // prefix of the clip's per-input counts; null: tri = clip
    int n_in, n_room;
};
struct BufOut {
    float *screen, *low, *high;
    int32_t *clip, *tri;
    cg_vec4 *pos;
};

// Tile: 64 x 8 pixels, one XCD row group high (the post-pass's tile), state words with halo 1.
constexpr int kBufTW = 64, kBufTH = 8, kBufHW = kBufTW + 2, kBufHH = kBufTH + 2;
static_assert(kBufTH == kXcdRows, "a tile row is one XCD row group");

__device__ __forceinline__ uint32_t buf_word(const RastArgs &A, const void *words, size_t o)
{
    if (!A.state16) return static_cast<const uint32_t *>(words)[o];
    const uint32_t v = static_cast<const uint16_t *>(words)[o];
    return (v & 0x7fffu) | ((v >> 15) << 31);      // the 4-byte form
}

// the record a state word names on row y; false: no owner
__device__ __forceinline__ bool buf_owner(const RastArgs &A, const BufIn &I, uint32_t word, int y, RowRec &R)
{
    const int rec = (int)(word & ~kStShadow) - 1;
    if (rec < 0) return false;
    const u64 o = (I.row_off ? I.row_off[y] : (u64)y * (u64)(unsigned)A.n) + (u64)(unsigned)rec;
    if (o >= I.rec_cap) return false;
    R = I.recs[o];
    return (unsigned)rec_t(R) < (unsigned)A.n;
}

// Clipped triangle t -> input triangle: input i's survivors are pre[i] .. pre[i + 1] - 1 of the
// list (rast_setup_kernel, rast_big_gather_kernel); room k -> k, boxes[k]'s 7 inputs -> n_room + k.
__device__ __forceinline__ int buf_tri(const BufIn &I, int t)
{
    if (!I.pre) return t;
    int lo = 0, hi = I.n_in - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (I.pre[mid] <= (u64)(unsigned)t) lo = mid;
        else hi = mid - 1;
    }
    return lo < I.n_room ? lo : I.n_room + (lo - I.n_room) / 7;
}

// Interpolate's pos3d of fragment x of the record (:546-549): illum_D's first three lines
__device__ __forceinline__ cg_vec4 buf_pos(const RowRec &R, int x)
{
    const float fi = (float)(x - R.lx);
    const float zinv = R.lz + (R.sz * fi);
    const float X = R.lX + (R.sX * fi), Y = R.lY + (R.sY * fi);
    cg_vec4 p;
    p.z = 1 / zinv;
    p.x = X / zinv;
    p.y = Y / zinv;
    p.w = 1.0f;
    return p;
}

// DIRECT: colour modes 1-2.  TEX: texture modes 1-3 possible (mode 0 only).
template <bool DIRECT, bool TEX>
__global__ __launch_bounds__(256) void rast_buffers_kernel(RastArgs A0, BufIn I, BufOut O)
{
    const RastArgs A = with_device_light(A0);
    __shared__ uint32_t s_st[kBufHH][kBufHW];
    // a tile row of a vec3 plane is 192 consecutive dwords of the plane: staged here so that each
    // wave stores 64 consecutive dwords instead of three strided ones per lane
    __shared__ float s_v[3][kBufTH][3 * kBufTW];
    const int W = A.W, H = A.H;
    int m;
    const int g = xcd_group(H, (W + kBufTW - 1) / kBufTW, m);
    if (g < 0) return;
    const int gx0 = m * kBufTW, gy0 = g * kBufTH;
    constexpr int kStR = (kBufHH * kBufHW + 255) / 256;
    uint32_t wv[kStR];
#pragma unroll
    for (int r = 0; r < kStR; ++r) {
        const int i = threadIdx.x + 256 * r;
        const int cy = i / kBufHW, cx = i - cy * kBufHW;
        const int gx = gx0 - 1 + cx, gy = gy0 - 1 + cy;
        const bool in = i < kBufHH * kBufHW && gx >= 0 && gy >= 0 && gx < W && gy < H;
        wv[r] = in ? buf_word(A, I.words, (size_t)gy * W + gx) : 0u;
    }
#pragma unroll
    for (int r = 0; r < kStR; ++r) {
        const int i = threadIdx.x + 256 * r;
        if (i < kBufHH * kBufHW) (&s_st[0][0])[i] = wv[r];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, x = gx0 + tx;
    const bool want_shade = O.screen || O.low || O.high;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int ty = (int)(threadIdx.x >> 6) + 4 * r, y = gy0 + ty;
        const bool in = x < W && y < H;
        const size_t o = (size_t)y * W + x;
        RowRec R;
        const bool own = in && buf_owner(A, I, s_st[ty + 1][tx + 1], y, R);
        vec3 sc = v3(0.f, 0.f, 0.f), lo = sc, hi = sc;
        if (want_shade && in) {
            if (DIRECT) {
                shade3c(A, I.direct[o], cg_vec3{0.f, 0.f, 0.f}, sc, lo, hi);
            } else if (own) {            // :580-585, rebuilt as rast_post_kernel does
                const float fi = (float)(x - R.lx);
                const float z = R.lz + (R.sz * fi);                               // :543
                const float X = R.lX + (R.sX * fi), Y = R.lY + (R.sY * fi);       // :547-548 numerators
                const int t = rec_t(R);
                const cg_vec4 tn = A.tris[t].normal;
                const cg_vec3 col = A.tris[t].color;
                vec3 N = v3(tn.x, tn.y, tn.z);
                int tex = 0;
                uint32_t texel = 0u;
                if (TEX && R.tex != 0 && rast_tex_present(A, R.tex)) {
                    tex = R.tex;
                    N = rast_tex_normal(A, tex, R.index, z, X, Y, x, y, N, texel);
                }
                const vec3 D = illum_D(A, z, X, Y, N);
                const float4 s4 = make_float4(__int_as_float(t | (x == R.first_x ? (1 << 30) : 0)), D.x, D.y, D.z);
                shade3c(A, s4, col, sc, lo, hi, tex, texel);
            }
            // the post-pass's darkening (:286-303): interior pixels only, subtracted once
            if (x >= 1 && y >= 1 && x < W - 1 && y < H - 1) {
                const float d = darken_at(&s_st[0][0], kBufHW, ty + 1, tx + 1);
                sc = sc - v3(d, d, d);
            }
        }
        s_v[0][ty][3 * tx] = sc.x; s_v[0][ty][3 * tx + 1] = sc.y; s_v[0][ty][3 * tx + 2] = sc.z;
        s_v[1][ty][3 * tx] = lo.x; s_v[1][ty][3 * tx + 1] = lo.y; s_v[1][ty][3 * tx + 2] = lo.z;
        s_v[2][ty][3 * tx] = hi.x; s_v[2][ty][3 * tx + 1] = hi.y; s_v[2][ty][3 * tx + 2] = hi.z;
        if (in) {
            const int t = own ? rec_t(R) : CG_RAST_OWNER_NONE;
            if (O.clip) O.clip[o] = t;
            if (O.tri) O.tri[o] = own ? buf_tri(I, t) : CG_RAST_OWNER_NONE;
            if (O.pos) O.pos[o] = own ? buf_pos(R, x) : cg_vec4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if (!want_shade) return;       // uniform: every thread of the grid sees the same pointers
    __syncthreads();
    float *const planes[3] = {O.screen, O.low, O.high};
    const int nx = min(kBufTW, W - gx0) * 3;          // dwords of a tile row that lie in the frame
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        float *const out = planes[b];
        if (!out) continue;
        for (int j = threadIdx.x; j < kBufTH * 3 * kBufTW; j += 256) {
            const int ty = j / (3 * kBufTW), k = j - ty * (3 * kBufTW);
            const int y = gy0 + ty;
            if (y < H && k < nx) out[((size_t)y * W + gx0) * 3 + k] = s_v[b][ty][k];
        }
    }
}

// One pixel of the above for cg_rast_pick: out[0] hit, [1] clip, [2] tri, [4..7] pos.
__global__ __launch_bounds__(64) void rast_pick_kernel(RastArgs A, BufIn I, int x, int y, int *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    RowRec R;
    const bool own = buf_owner(A, I, buf_word(A, I.words, (size_t)y * A.W + x), y, R);
    const int t = own ? rec_t(R) : CG_RAST_OWNER_NONE;
    const cg_vec4 p = own ? buf_pos(R, x) : cg_vec4{0.f, 0.f, 0.f, 0.f};
    out[0] = own ? 1 : 0;
    out[1] = t;
    out[2] = own ? buf_tri(I, t) : CG_RAST_OWNER_NONE;
    out[3] = 0;
    out[4] = __float_as_int(p.x); out[5] = __float_as_int(p.y); out[6] = __float_as_int(p.z); out[7] = __float_as_int(p.w);
}

// One workgroup: pre[i] = counts[0] + .. + counts[i - 1] (negative counts as 0), pre[n] the total.
// The dense route's setup keeps this prefix in LDS only; the compact route stores its own.
__global__ __launch_bounds__(256) void rast_buffers_prefix_kernel(const int *__restrict__ counts, int n,
                                                                 u64 *__restrict__ pre)
{
    constexpr int kItems = 16;
    __shared__ u64 s_sum[256];
    __shared__ u64 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256 * kItems) {
        const int base = i0 + (int)threadIdx.x * kItems;
        int v[kItems];
        u64 s = 0;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            v[k] = base + k < n ? max(counts[base + k], 0) : 0;
            s += (u64)(unsigned)v[k];
        }
        s_sum[threadIdx.x] = s;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {       // inclusive scan of the threads' sums
            const u64 a = threadIdx.x >= (unsigned)o ? s_sum[threadIdx.x - o] : 0;
            __syncthreads();
            s_sum[threadIdx.x] += a;
            __syncthreads();
        }
        u64 run = s_carry + s_sum[threadIdx.x] - s;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            if (base + k < n) pre[base + k] = run;
            run += (u64)(unsigned)v[k];
        }
        __syncthreads();
        if (threadIdx.x == 255) s_carry += s_sum[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) pre[n] = s_carry;
}

// ---- host ----
// The latest frame's scratch as the kernels take it; n_room < 0: the caller's list was the
// clipped list (cg_rast_render_buffers*).  want_tri: the clip -> input prefix is needed.
static int buffers_inputs(cg_ctx *c, int n_room, bool want_tri, hipStream_t st, BufIn *out)
{
    const RastFrame &fr = *ctx_rast_frame(c);
    if (!fr.valid || !fr.words) return ctx_invalid(c, "buffers: the frame left no state words");
    BufIn I;
    I.words = fr.words;
    I.direct = fr.direct;
    I.recs = fr.recs;
    I.row_off = fr.row_off;
    I.rec_cap = fr.rec_cap;
    I.pre = nullptr;
    I.n_in = 0;
    I.n_room = 0;
    if (want_tri && n_room >= 0 && fr.counts && fr.n_in > 0) {
        const u64 *pre = fr.pre;
        if (!pre) {
            hipError_t e;
            u64 *p = (u64 *)ctx_buf(c, kBufClipPre, ((size_t)fr.n_in + 1) * sizeof(u64), &e);
            if (!p) return ctx_fail(c, e, "alloc clip prefix");
            hipLaunchKernelGGL(rast_buffers_prefix_kernel, dim3(1), dim3(256), 0, st, fr.counts, fr.n_in, p);
            if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_buffers_prefix launch");
            pre = p;
        }
        I.pre = pre;
        I.n_in = fr.n_in;
        I.n_room = n_room;
    }
    *out = I;
    return CG_OK;
}

// The buffers kernel over the frame just queued on st (planes in device memory; any may be null).
int rast_buffers_device(cg_ctx *c, const cg_rast_buffers *d, int n_room, hipStream_t st)
{
    BufOut O{d->screen, d->low, d->high, d->clip, d->tri, d->pos};
    if (!O.screen && !O.low && !O.high && !O.clip && !O.tri && !O.pos) return CG_OK;
    BufIn I;
    if (const int rc = buffers_inputs(c, n_room, O.tri != nullptr, st, &I)) return rc;
    const RastFrame &fr = *ctx_rast_frame(c);
    const RastArgs &A = fr.A;
    const dim3 grid(xcd_grid(A.H, (A.W + kBufTW - 1) / kBufTW));
    if (fr.mode != 0)
        hipLaunchKernelGGL((rast_buffers_kernel<true, false>), grid, dim3(256), 0, st, A, I, O);
    else if (A.textured)
        hipLaunchKernelGGL((rast_buffers_kernel<false, true>), grid, dim3(256), 0, st, A, I, O);
    else
        hipLaunchKernelGGL((rast_buffers_kernel<false, false>), grid, dim3(256), 0, st, A, I, O);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CG_OK : ctx_fail(c, e, "rast_buffers launch");
}

// One pixel of the frame just queued on st: out8 (host) as rast_pick_kernel leaves it.  Waits.
int rast_pick_device(cg_ctx *c, int n_room, int x, int y, hipStream_t st, int *out8)
{
    BufIn I;
    if (const int rc = buffers_inputs(c, n_room, true, st, &I)) return rc;
    hipError_t e;
    int *d = (int *)ctx_buf(c, kBufPick, 8 * sizeof(int), &e);
    if (!d) return ctx_fail(c, e, "alloc pick record");
    const RastFrame &fr = *ctx_rast_frame(c);
    if (x < 0 || y < 0 || x >= fr.A.W || y >= fr.A.H) return CG_E_INVALID;
    hipLaunchKernelGGL(rast_pick_kernel, dim3(1), dim3(64), 0, st, fr.A, I, x, y, d);
    if ((e = hipGetLastError()) != hipSuccess) return ctx_fail(c, e, "rast_pick launch");
    if ((e = hipMemcpyAsync(out8, d, 8 * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return ctx_fail(c, e, "pick record");
    return CG_OK;
}

// 2 or 4: the bytes of the latest frame's state word (0: none)
int rast_frame_state_bytes(cg_ctx *c)
{
    const RastFrame &fr = *ctx_rast_frame(c);
    return fr.valid ? (fr.A.state16 ? 2 : 4) : 0;
}

}  // namespace cg
