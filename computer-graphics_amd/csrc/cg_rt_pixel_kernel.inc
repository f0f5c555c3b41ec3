// The text of the per-pixel raytracer kernel, included by cg_rt.hip once per output policy:
//   CG_RT_PIXEL_NAME  the kernel's identifier
//   CG_RT_PIXEL_F32   0: `out` holds put_pixel's words (rt_pixel_kernel)
//                     1: `out` holds float4 pixels (CG_PIX_RGBA_F32, rt_pixel_f32_kernel) -- the sum
//                        over 9 that put_pixel is given, and the number of sub-rays that hit
//   CG_RT_PIXEL_OUT   the pixel type of `out`
// Shared as text, not as a __device__ body behind two wrappers: a body reads RtFrame through a copy
// of the kernel argument instead of from the kernel-argument segment, which changes the machine code
// of rt_pixel_kernel (codeobj.kernel_sha256 pins it for the committed profiles).
template <bool CULL>
__global__ __launch_bounds__(kRtThreads, kRtPixelWaves) void CG_RT_PIXEL_NAME(RtFrame F, const RtTri *__restrict__ tc,
                                                              const RtShade *__restrict__ shade,
                                                              const RtSphere *__restrict__ sph,
                                                              CG_RT_PIXEL_OUT *__restrict__ out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * kRtTileW + wave * 8 + (lane & 7);
    const int L = blockIdx.y * kRtTileH + (lane >> 3);
    const bool inside = u < F.W && L < F.rows_out;
    const int v = inside ? shard_row(F, L) : 0;
    const bool active = inside && v < F.H;
    vec4 dir = v4((float)(u - F.W / 2), (float)(v - F.H / 2), F.focal, 1.0f);        // :126
    dir = mat4_mul(F.R, dir);                                                         // :128
    unsigned long long mask = ~0ull;
    if (CULL) {
        // exact float extremes of the wave's sub-ray directions (:137): newDir.x =
        // fl(dir.x + 0.5 i) is monotone in dir.x, so the bundle lies in this box
        float ax = active ? dir.x : __int_as_float(0x7fc00000), ay = active ? dir.y : __int_as_float(0x7fc00000);
        float x0 = wave_min(active ? ax : FLT_MAX), x1 = wave_max(active ? ax : -FLT_MAX);
        float y0 = wave_min(active ? ay : FLT_MAX), y1 = wave_max(active ? ay : -FLT_MAX);
        x0 = x0 - 0.5f; x1 = x1 + 0.5f; y0 = y0 - 0.5f; y1 = y1 + 0.5f;
        bool keep = true;
        if (lane < F.n_tris && x0 <= x1 && y0 <= y1) keep = !cull_primary(tc[lane], x0, x1, y0, y1, F.focal);
        mask = __ballot(keep && lane < F.n_tris);
    }
    // every lane stays to the end: the certificates' wave reductions read all 64
    uint32_t px = 0u;
    [[maybe_unused]] float4 rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // Pass 1: the 9 primary rays (:134-140); hits staged in LDS (bi, t) so one
    // shadow certificate covers the whole wave's hits and all lights at once.
    __shared__ int s_bi[9][kRtThreads];
    __shared__ float s_t[9][kRtThreads];
    const float m = 0.5f;
    if (active) {
        // sub-ray k = 3 (i + 1) + (j + 1): d = (dir.x + m i, dir.y + m j, focal)  (:137),
        // walked in three groups sharing d.y (closest_primary_group)
        float dx[3], dy[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            dx[q] = dir.x + (m * (float)(q - 1));
            dy[q] = dir.y + (m * (float)(q - 1));
        }
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            int bi[3];
            float t[3];
            const float dyj[1] = {dy[jj]};
            closest_primary_group<CULL, 3, 1>(F, tc, sph, dx, dyj, mask, bi, t);         // :140
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) {
                s_bi[3 * ii + jj][threadIdx.x] = bi[ii];
                s_t[3 * ii + jj][threadIdx.x] = t[ii];
            }
        }
    }
    // one mask for every light of the set (the mask walk must stop at n_tris)
    unsigned long long smask = F.n_tris >= 64 ? ~0ull : ((1ull << F.n_tris) - 1ull);
    if (CULL && F.cull_shadow && F.n_lights > 0) {
        LanePosBox pb;
        pb.init();
        if (active)
            for (int k = 0; k < 9; ++k) {
                const int bi = s_bi[k][threadIdx.x];
                if (bi == INT_MIN) continue;
                const float t = s_t[k][threadIdx.x];
                const int i = k / 3 - 1, j = k % 3 - 1;
                vec3 nd = v3(dir.x + (m * (float)i), dir.y + (m * (float)j), F.focal);
                pb.add(v3(F.cam[0] + t * nd.x, F.cam[1] + t * nd.y, F.cam[2] + t * nd.z));   // :326/:345
            }
        smask = shadow_mask_box(F, tc, shadow_box_of_positions(F, pb), lane);
    }
    if (active) {
        // Pass 2: shading in the reference's order (:143-157)
        vec3 pc = v3(0.0f, 0.0f, 0.0f);
        bool valid = false;
        [[maybe_unused]] int nhit = 0;
        const vec3 ind = v3(F.indirect, F.indirect, F.indirect);
        for (int k = 0; k < 9; ++k) {
            const int i = k / 3 - 1, j = k % 3 - 1;
            const int bi = s_bi[k][threadIdx.x];
            if (bi == INT_MIN) continue;
            const float t = s_t[k][threadIdx.x];
            vec3 nd = v3(dir.x + (m * (float)i), dir.y + (m * (float)j), F.focal);
            vec3 pos = v3(F.cam[0] + t * nd.x, F.cam[1] + t * nd.y, F.cam[2] + t * nd.z);  // :326/:345
            valid = true;
            if constexpr (CG_RT_PIXEL_F32) ++nhit;
            vec3 oc = object_colour(shade, sph, bi);
            for (int l = 0; l < F.n_lights; ++l)                                          // :151-153
                pc = pc + direct_light<CULL>(F, tc, shade, sph, bi, pos, oc, l, smask);
            pc = pc + (oc * ind);                                                         // :156
        }
        if constexpr (CG_RT_PIXEL_F32) {
            const vec3 q = valid ? div_const(pc, 9.0f, 1.0f / 9.0f) : v3(0.0f, 0.0f, 0.0f);
            rad = make_float4(q.x, q.y, q.z, (float)nhit);
        } else {
            px = valid ? put_pixel(div_const(pc, 9.0f, 1.0f / 9.0f)) : put_pixel(v3(0.0f, 0.0f, 0.0f));         // :160-166
        }
    }
#if CG_RT_PIXEL_F32
    if (inside) out[(size_t)L * F.W + u] = rad;   // padding rows: zero bytes
#else
    if (inside) out[(size_t)L * F.W + u] = px;
#endif
}
