// The text of the rasteriser's dense post-pass kernel, included by cg_rast.hip once per output policy:
//   CG_RAST_POST_NAME  the kernel's identifier
//   CG_RAST_POST_F32   0: `out` holds PutPixelSDL's words (rast_post_kernel)
//                      1: `out` holds float4 pixels (CG_PIX_RGBA_F32, rast_post_f32_kernel): the vec3
//                         antiAliasing returns and w = 1 inside, +0 four times on the border, and the
//                         same zeros over a whole frame whose status word is set
//   CG_RAST_POST_OUT   the pixel type of `out`
// Shared as text, as cg_rt_pixel_kernel.inc is: rast_post_kernel keeps its machine code.
template <bool DIRECT, bool TEX>
__global__ __launch_bounds__(256) void CG_RAST_POST_NAME(const cg_rtri *__restrict__ tris, RastArgs A0,
                                                       const void *__restrict__ state_v,
                                                       const RowRec *__restrict__ recs,
                                                       const int32_t *__restrict__ sh,
                                                       CG_RAST_POST_OUT *__restrict__ out,
                                                       const int32_t *__restrict__ skip)
{
#if CG_RAST_POST_F32
    const bool undrawn = DIRECT && skip && *skip != 0;    // sequence frame over the capacity: all uncovered
#else
    if (DIRECT && skip && *skip != 0) return;             // sequence frame over the capacity: plane untouched
#endif
    RastArgs A = A0;
    if (!DIRECT && A.d_light) {                           // light from the device geometry (:223)
        const cg_vec4 L = *A.d_light;
        A.light[0] = L.x; A.light[1] = L.y; A.light[2] = L.z;
    }
    __shared__ float s_c[9][kPostHH][kPostHW];      // sc.xyz, lo.xyz, hi.xyz
    __shared__ float s_d[kPostHH][kPostHW];
    // The halo-2 words (colour modes 1-2: the shadow marks; mode 0: the state
    // words) live in s_c's space: every thread takes what it needs from them
    // (its pixels' records and darkenings) into registers before the barrier
    // after which s_c is written.  26.4 KB instead of 29.7: six workgroups
    // per CU instead of five.
    static_assert(sizeof(uint32_t) * kPostSH * kPostSW <= sizeof(float) * 9 * kPostHH * kPostHW, "halo words fit");
    int (*s_sh)[kPostSW] = reinterpret_cast<int (*)[kPostSW]>(&s_c[0][0][0]);
    const int W = A.W, H = A.H;
    static_assert(kPostTH == kXcdRows, "a post tile row is one XCD row group");
    int m;
    const int g = xcd_group(H, (W + kPostTW - 1) / kPostTW, m);
    if (g < 0) return;
    const int gx0 = m * kPostTW, gy0 = g * kPostTH;
#if CG_RAST_POST_F32
    if (undrawn) {                                        // workgroup-uniform, before any barrier
        for (int i = threadIdx.x; i < kPostTH * kPostTW; i += 256) {
            const int ty = i / kPostTW, x = gx0 + i - ty * kPostTW, y = gy0 + ty;
            if (x < W && y < H) out[(size_t)y * W + x] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        return;
    }
#endif
    const uint32_t *st4 = static_cast<const uint32_t *>(state_v);
    const uint16_t *st2 = static_cast<const uint16_t *>(state_v);
    auto state_at = [&](size_t o) -> uint32_t {   // the 4-byte form
        if (!A.state16) return st4[o];
        const uint32_t v = st2[o];
        return (v & 0x7fffu) | ((v >> 15) << 31);
    };
    const float4 *st16 = static_cast<const float4 *>(state_v);
    // all global loads first (shadow marks, shade state), so each thread has them in flight together
    constexpr int kShR = (kPostSH * kPostSW + 255) / 256, kStR = (kPostHH * kPostHW + 255) / 256;
    // mode 0: the state words (record + 1, mark in bit 31) of the tile + halo 2
    uint32_t (*s_st)[kPostSW] = reinterpret_cast<uint32_t (*)[kPostSW]>(&s_c[0][0][0]);
    uint32_t shv[kShR];
#pragma unroll
    for (int r = 0; r < kShR; ++r) {
        const int i = threadIdx.x + 256 * r;
        const int cy = i / kPostSW, cx = i - cy * kPostSW;
        const int gx = gx0 - 2 + cx, gy = gy0 - 2 + cy;
        const bool in = i < kPostSH * kPostSW && gx >= 0 && gy >= 0 && gx < W && gy < H;
        if (DIRECT) shv[r] = in ? (uint32_t)sh[(size_t)gy * W + gx] : 0u;
        else shv[r] = in ? state_at((size_t)gy * W + gx) : 0u;
    }
#pragma unroll
    for (int r = 0; r < kShR; ++r) {
        const int i = threadIdx.x + 256 * r;
        if (i < kPostSH * kPostSW) {
            if (DIRECT) (&s_sh[0][0])[i] = (int)shv[r];
            else (&s_st[0][0])[i] = shv[r];
        }
    }
    __syncthreads();
    float dv[kStR];   // each pixel's darkening, from the marks before s_c is written
#pragma unroll
    for (int r = 0; r < kStR; ++r) {
        const int i = threadIdx.x + 256 * r;
        const int cy = i / kPostHW, cx = i - cy * kPostHW;
        const int gx = gx0 - 1 + cx, gy = gy0 - 1 + cy;
        dv[r] = 0.0f;
        if (i < kPostHH * kPostHW && gx >= 1 && gy >= 1 && gx < W - 1 && gy < H - 1)
            dv[r] = DIRECT ? darken_at(&s_sh[0][0], kPostSW, cy + 1, cx + 1)
                           : darken_at(&s_st[0][0], kPostSW, cy + 1, cx + 1);
    }
    if constexpr (DIRECT) {
        __syncthreads();   // the marks are dead: s_c's space is free
#pragma unroll
        for (int r = 0; r < kStR; ++r) {
            const int i = threadIdx.x + 256 * r;
            if (i >= kPostHH * kPostHW) break;
            const int cy = i / kPostHW, cx = i - cy * kPostHW;
            const int gx = gx0 - 1 + cx, gy = gy0 - 1 + cy;
            vec3 sc = v3(0.f, 0.f, 0.f), lo = sc, hi = sc;
            const float d = dv[r];
            if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
                const float4 s4 = st16[(size_t)gy * W + gx];
                const int tb = __float_as_int(s4.x);
                const bool tri = tb >= 0 && !(tb & kStateDirect);
                shade3c(A, s4, tri ? tris[tb & ~(1 << 30)].color : cg_vec3{0.f, 0.f, 0.f}, sc, lo, hi);
            }
            s_c[0][cy][cx] = sc.x; s_c[1][cy][cx] = sc.y; s_c[2][cy][cx] = sc.z;
            s_c[3][cy][cx] = lo.x; s_c[4][cy][cx] = lo.y; s_c[5][cy][cx] = lo.z;
            s_c[6][cy][cx] = hi.x; s_c[7][cy][cx] = hi.y; s_c[8][cy][cx] = hi.z;
            s_d[cy][cx] = d;
        }
    } else {
        // The shading fragments of the tile + halo 1: each thread's record
        // loads go out together, then their triangles', then the arithmetic --
        // two dependent round trips instead of two per pixel.
        RowRec rv[kStR];
        int recv[kStR];
#pragma unroll
        for (int r = 0; r < kStR; ++r) {
            const int i = threadIdx.x + 256 * r;
            const int cy = i / kPostHW, cx = i - cy * kPostHW;
            const int gx = gx0 - 1 + cx, gy = gy0 - 1 + cy;
            const bool in = i < kPostHH * kPostHW && gx >= 0 && gy >= 0 && gx < W && gy < H;
            recv[r] = in ? (int)(s_st[cy + 1][cx + 1] & ~kStShadow) - 1 : -1;
            if (recv[r] >= 0) rv[r] = recs[(size_t)gy * A.n + recv[r]];
        }
        __syncthreads();   // the state words are dead: s_c's space is free
        cg_vec4 tnv[kStR];
        cg_vec3 colv[kStR];
#pragma unroll
        for (int r = 0; r < kStR; ++r)
            if (recv[r] >= 0) {
                const int t = rec_t(rv[r]);
                tnv[r] = tris[t].normal;
                colv[r] = tris[t].color;
            }
#pragma unroll
        for (int r = 0; r < kStR; ++r) {
            const int i = threadIdx.x + 256 * r;
            if (i >= kPostHH * kPostHW) break;
            const int cy = i / kPostHW, cx = i - cy * kPostHW;
            const int gx = gx0 - 1 + cx, gy = gy0 - 1 + cy;
            vec3 sc = v3(0.f, 0.f, 0.f), lo = sc, hi = sc;
            const float d = dv[r];
            if (recv[r] >= 0) {   // a shading fragment (:580-585, rebuilt as shade_from_record does)
                const RowRec &R = rv[r];
                const float fi = (float)(gx - R.lx);
                const float z = R.lz + (R.sz * fi);                               // :543, as the fill evaluated it
                const float X = R.lX + (R.sX * fi), Y = R.lY + (R.sY * fi);       // :547-548 numerators
                const int t = rec_t(R);
                vec3 N = v3(tnv[r].x, tnv[r].y, tnv[r].z);
                int tex = 0;
                uint32_t texel = 0u;
                if (TEX && R.tex != 0 && rast_tex_present(A, R.tex)) {
                    tex = R.tex;
                    N = rast_tex_normal(A, tex, R.index, z, X, Y, gx, gy, N, texel);
                }
                const vec3 D = illum_D(A, z, X, Y, N);                            // :580-585 (:590-645)
                const float4 s4 = make_float4(__int_as_float(t | (gx == R.first_x ? (1 << 30) : 0)), D.x, D.y, D.z);
                shade3c(A, s4, colv[r], sc, lo, hi, tex, texel);
            }
            s_c[0][cy][cx] = sc.x; s_c[1][cy][cx] = sc.y; s_c[2][cy][cx] = sc.z;
            s_c[3][cy][cx] = lo.x; s_c[4][cy][cx] = lo.y; s_c[5][cy][cx] = lo.z;
            s_c[6][cy][cx] = hi.x; s_c[7][cy][cx] = hi.y; s_c[8][cy][cx] = hi.z;
            s_d[cy][cx] = d;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPostTH * kPostTW; i += 256) {
        const int ty = i / kPostTW, tx = i - ty * kPostTW;
        const int x = gx0 + tx, y = gy0 + ty;
        if (x >= W || y >= H) continue;
        const size_t o = (size_t)y * W + x;
        if (x < 1 || y < 1 || x >= W - 1 || y >= H - 1) {   // :283-284 border never written
#if CG_RAST_POST_F32
            out[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // w = 0: uncovered
#else
            out[o] = 0u;
#endif
            continue;
        }
        const int cy = ty + 1, cx = tx + 1;
        auto tap = [&](int b, int yy, int xx) { return v3(s_c[b][yy][xx], s_c[b + 1][yy][xx], s_c[b + 2][yy][xx]); };
        auto dk = [&](int yy, int xx) { const float d = s_d[yy][xx]; return v3(d, d, d); };
        const int ty5[5] = {cy, cy - 1, cy + 1, cy, cy}, tx5[5] = {cx, cx, cx, cx - 1, cx + 1};  // c, up, down, left, right
        vec3 sv[5], lv[5], hv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            sv[k] = tap(0, ty5[k], tx5[k]);
            lv[k] = tap(3, ty5[k], tx5[k]);
            hv[k] = tap(6, ty5[k], tx5[k]);
        }
        sv[0] = sv[0] - dk(cy, cx);                        // darkened: itself, up, left
        sv[1] = sv[1] - dk(cy - 1, cx);
        sv[3] = sv[3] - dk(cy, cx - 1);
        // :1741-1750 (x / 5.0f and / 3.0f via div_const, bit-identical)
        vec3 val = div_const((((sv[0] + sv[1]) + sv[2]) + sv[3]) + sv[4], 5.0f, 1.0f / 5.0f);
        vec3 val1 = div_const((((lv[0] + lv[1]) + lv[2]) + lv[3]) + lv[4], 5.0f, 1.0f / 5.0f);
        vec3 val2 = div_const((((hv[0] + hv[1]) + hv[2]) + hv[3]) + hv[4], 5.0f, 1.0f / 5.0f);
        val = div_const((val + val1) + val2, 3.0f, 1.0f / 3.0f);
#if CG_RAST_POST_F32
        out[o] = make_float4(val.x, val.y, val.z, 1.0f);
#else
        out[o] = put_pixel(val);
#endif
    }
}
