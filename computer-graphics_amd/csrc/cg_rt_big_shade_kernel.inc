// The text of the large-scene shading kernel (K7), included by cg_rt_big.hip once per output policy:
//   CG_RT_BIG_SHADE_NAME  the kernel's identifier
//   CG_RT_BIG_SHADE_F32   0: `out` holds put_pixel's words (rt_big_shade_kernel)
//                         1: `out` holds float4 pixels (CG_PIX_RGBA_F32, rt_big_shade_f32_kernel) -- the
//                            sum over 9 that put_pixel is given, and the number of sub-rays that hit
//   CG_RT_BIG_SHADE_OUT   the pixel type of `out`
// Shared as text, not as a __device__ body behind two wrappers: a body reads RtFrame and BigBufs
// through copies of the kernel arguments, which changes the machine code of rt_big_shade_kernel
// (codeobj.kernel_sha256 pins it for the committed profiles).
template <int LM>
#ifdef CG_SHADE_WAVES   // A/B builds
__global__ __launch_bounds__(kRtThreads, CG_SHADE_WAVES) void CG_RT_BIG_SHADE_NAME(
#else
__global__ __launch_bounds__(kRtThreads) void CG_RT_BIG_SHADE_NAME(
#endif
    RtFrame F, const RtTri *__restrict__ tc,
                                                                  const RtShade *__restrict__ shade,
                                                                  const RtSphere *__restrict__ sph, BigBufs B,
                                                                  CG_RT_BIG_SHADE_OUT *__restrict__ out)
{
    constexpr bool kLat = LM > 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // wave: uniform (SGPR)
    const int tx = blockIdx.x * (kRtTileW / 8) + wave, ty = blockIdx.y;
    if (tx >= B.tiles_x) return;
    const int u = tx * 8 + (lane & 7), L = ty * 8 + (lane >> 3);
    const bool inside = u < F.W && L < F.rows_out;
    if (!inside) return;
    const int v = shard_row(F, L);
    const bool active = v < F.H;
    uint32_t px = 0u;
    [[maybe_unused]] float4 rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // padding rows: zero bytes
    if (active) {
        const size_t npix = (size_t)F.rows_out * F.W, pix = (size_t)L * F.W + u;
        const vec4 dir = pixel_dir(F, u, v);
        const bool flags_fit = kLat || 9 * F.n_lights <= 64;
        const unsigned long long pshadowed = !kLat && flags_fit && F.n_lights > 0 ? B.sh_bits[pix] : 0ull;
        // rays past the queue still carry pending bits: the lit search per lane
        const unsigned long long pleft = !kLat && flags_fit && F.n_lights > 0 ? B.pend_bits[pix] : 0ull;
        const int bin = (tx / kBinTilesX) + (ty / kBinTilesY) * B.bins_x;
        vec3 pc = v3(0.0f, 0.0f, 0.0f);
        bool valid = false;
        [[maybe_unused]] int nhit = 0;
        const vec3 ind = v3(F.indirect, F.indirect, F.indirect);
        const float m = 0.5f;
        for (int s = 0; s < 9; ++s) {
            const int i = s / 3 - 1, j = s % 3 - 1;
            const vec3 nd = v3(dir.x + (m * (float)i), dir.y + (m * (float)j), F.focal);   // :137
            const size_t id = kLat ? (size_t)(2 * L + j + 1) * B.lat_w + ((LM == 2 ? 3 : 2) * u + i + 1)
                                   : s * npix + pix;
            int bi;
            vec3 pos, normal;
            hit_geometry(F, B, shade, sph, nd, id, bi, pos, normal);
            if (bi == INT_MIN) continue;
            valid = true;
            if constexpr (CG_RT_BIG_SHADE_F32) ++nhit;
            unsigned long long shadowed = pshadowed, left = pleft;
            if (kLat && F.n_lights > 0) {
                shadowed = B.sh_bits[id];
                left = B.pend_bits[id];
            }
            vec3 oc = object_colour(shade, sph, bi);
            for (int l = 0; l < F.n_lights; ++l) {                                    // :151-153
                const RtLight Lt = F.lights[l];
                const ShadowRay q = shadow_ray(Lt, pos, normal);
                bool ts;
                const int bit = kLat ? l : s * F.n_lights + l;
                if (flags_fit) {
                    ts = ((shadowed >> bit) & 1ull) != 0;
                    if (!ts && ((left >> bit) & 1ull)) ts = lit_blocked_lane(tc, B, q.origin, q.nd, q.len, q.rmag);
                } else {
                    ts = grid_blocker(B.grid, tc, q) >= 0 || any_hit_bin(tc, B, F.n_tris, bin, q);
                }
                pc = pc + big_direct_light(F, sph, Lt, q, normal, oc, ts);
            }
            pc = pc + (oc * ind);                                                     // :156
        }
        if constexpr (CG_RT_BIG_SHADE_F32) {
            const vec3 q = valid ? div_const(pc, 9.0f, 1.0f / 9.0f) : v3(0.0f, 0.0f, 0.0f);
            rad = make_float4(q.x, q.y, q.z, (float)nhit);
        } else {
            px = valid ? put_pixel(div_const(pc, 9.0f, 1.0f / 9.0f)) : put_pixel(v3(0.0f, 0.0f, 0.0f));     // :160-166
        }
    }
#if CG_RT_BIG_SHADE_F32
    out[(size_t)L * F.W + u] = rad;
#else
    out[(size_t)L * F.W + u] = px;
#endif
}
