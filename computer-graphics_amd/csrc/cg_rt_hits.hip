// cg_rt_hits.hip -- per-pixel hit records and picking (cg_rt_hits_device, cg_rt_pick): the
// reference's Intersection (raytracer/Source/skeleton.cpp:40-45) of one camera sub-ray per pixel,
// which every frame computes and discards.
//
//   rt_hits_small_kernel   scenes of <= 64 triangles: one thread per pixel, every triangle in index
//                          order and every sphere, ClosestIntersection (:263-363) as
//                          rt_probe_closest_kernel states it, so the records are the probe's bytes.
//   rt_pick_reduce_kernel  one ray against any number of triangles: workgroups stride over the
//   rt_pick_final_kernel   scene, each thread keeps the lexicographic minimum of (distance, index)
//                          over the hits it accepts, compared as floats (-0 ties with +0); the
//                          minimum of the partial results is unique, so no schedule changes it.  The
//                          record is then formed again from the winning index with the same
//                          expressions, and the spheres follow (:341-355).
// Large scenes take a hits-only pass of the binned path instead (cg_rt_big.hip).  The ray of pixel
// (x, y), sub-ray s is rt_pixel_ray's on the host and pixel_ray's here: one expression tree.
#include <float.h>
#include <limits.h>

#include <algorithm>

#include "cg_host.h"
#include "cg_rt_dev.h"

namespace cg {

namespace {

constexpr int kPickThreads = 256;
constexpr int kPickGroups = 128;   // a stride covers 32,768 triangles

// skeleton.cpp:126-137: d = R * (x - W/2, y - H/2, focal, 1), dir = (d.x + 0.5 i, d.y + 0.5 j, focal, 1)
// for sub-ray s = 3 (i + 1) + (j + 1)
CG_HD vec4 pixel_ray(const float *R, int W, int H, float focal, int x, int y, int s)
{
    vec4 d = v4((float)(x - W / 2), (float)(y - H / 2), focal, 1.0f);
    d = mat4_mul(R, d);
    return v4(d.x + (0.5f * (float)(s / 3 - 1)), d.y + (0.5f * (float)(s % 3 - 1)), focal, 1.0f);
}

__device__ __forceinline__ cg_isect miss_record()
{
    cg_isect ci;
    ci.distance = FLT_MAX;
    ci.position = cg_vec4{0, 0, 0, 0};
    ci.triangleIndex = 0;
    ci.sphereIndex = 0;
    return ci;
}

// One triangle against the ray (s, d), the reference's expressions (:283-335): whether the hit is
// accepted whatever the closest so far is, its t and distance.
__device__ __forceinline__ bool tri_accepts(const cg_tri &T, vec4 s, vec3 d, float &t, float &distance)
{
    const vec3 nd = -d;
    vec3 e1 = v3(T.v1.x - T.v0.x, T.v1.y - T.v0.y, T.v1.z - T.v0.z);
    vec3 e2 = v3(T.v2.x - T.v0.x, T.v2.y - T.v0.y, T.v2.z - T.v0.z);
    vec3 sol = v3(s.x - T.v0.x, s.y - T.v0.y, s.z - T.v0.z);
    float det = det3(nd, e1, e2);
    t = det3(sol, e1, e2) / det;
    distance = t * length(d);
    if (distance < 0.0f) return false;                       // :311
    if (!(distance < FLT_MAX)) return false;                 // :313 against the initial record; a NaN never wins
    float uu = det3(nd, sol, e2) / det;
    float vv = det3(nd, e1, sol) / det;
    return (uu >= 0) && (vv >= 0) && ((uu + vv) <= 1);       // :328
}

// ClosestIntersection of the ray (s, d) over the whole scene, rt_probe_closest_kernel's loop.
__device__ __forceinline__ cg_isect closest_all(const RtFrame &F, const cg_tri *__restrict__ tris,
                                               const RtSphere *__restrict__ sph, vec4 s, vec3 d)
{
    const float bound = FLT_MAX;
    cg_isect ci = miss_record();
    vec3 s3 = xyz(s);
    vec3 nd = -d;
    for (int k = 0; k < F.n_tris; ++k) {
        cg_tri T = tris[k];
        vec3 e1 = v3(T.v1.x - T.v0.x, T.v1.y - T.v0.y, T.v1.z - T.v0.z);
        vec3 e2 = v3(T.v2.x - T.v0.x, T.v2.y - T.v0.y, T.v2.z - T.v0.z);
        vec3 sol = v3(s.x - T.v0.x, s.y - T.v0.y, s.z - T.v0.z);
        float det = det3(nd, e1, e2);
        float t = det3(sol, e1, e2) / det;
        float distance = t * length(d);
        if (distance < 0.0f) continue;
        if (distance >= ci.distance || distance > bound) continue;   // strict <: the lower index keeps a tie
        float uu = det3(nd, sol, e2) / det;
        float vv = det3(nd, e1, sol) / det;
        vec3 td = d * t;
        if ((uu >= 0) && (vv >= 0) && ((uu + vv) <= 1)) {
            ci.position = cg_vec4{s.x + td.x, s.y + td.y, s.z + td.z, s.w + 0};
            ci.distance = distance;
            ci.triangleIndex = k;
            ci.sphereIndex = -1;
        }
    }
    for (int k = 0; k < F.n_sph; ++k) {
        float t;
        if (sphere_intersect(sph[k], s3, d, t)) {
            vec3 td = d * t;
            if (t < ci.distance) {
                ci.position = cg_vec4{s.x + td.x, s.y + td.y, s.z + td.z, s.w + 0};
                ci.distance = t;
                ci.triangleIndex = -1;
                ci.sphereIndex = k;
            }
        }
    }
    return ci;
}

__device__ __forceinline__ int index_of(const cg_isect &ci)
{
    if (!(ci.distance < FLT_MAX)) return INT_MIN;
    return ci.sphereIndex >= 0 ? -1 - ci.sphereIndex : ci.triangleIndex;
}

// A 64 x 4 pixel block per workgroup; the triangle index is uniform, so the records load as scalars.
__global__ __launch_bounds__(256) void rt_hits_small_kernel(RtFrame F, const cg_tri *__restrict__ tris,
                                                            const RtSphere *__restrict__ sph, RtHits Hs)
{
    const int u = blockIdx.x * 64 + (threadIdx.x & 63), L = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= F.W || L >= F.rows_out) return;
    const size_t pix = (size_t)L * F.W + u;
    const int v = shard_row(F, L);
    cg_isect ci = miss_record();
    if (v < F.H) {   // padding rows of the last stripe stay misses
        const vec4 dir = pixel_ray(F.R, F.W, F.H, F.focal, u, v, Hs.sub_ray);
        ci = closest_all(F, tris, sph, v4(F.cam[0], F.cam[1], F.cam[2], F.cam[3]), xyz(dir));
    }
    if (Hs.isect) Hs.isect[pix] = ci;
    if (Hs.index) Hs.index[pix] = index_of(ci);
    if (Hs.distance) Hs.distance[pix] = ci.distance;
}

struct PickBest {
    float d;
    int i;
};
__device__ __forceinline__ PickBest pick_min(PickBest a, PickBest b)
{
    return (b.d < a.d || (b.d == a.d && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ PickBest pick_wave_min(PickBest v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        PickBest w;
        w.d = __shfl_xor(v.d, o, 64);
        w.i = __shfl_xor(v.i, o, 64);
        v = pick_min(v, w);
    }
    return v;
}

__global__ __launch_bounds__(kPickThreads) void rt_pick_reduce_kernel(int n_tris, const cg_tri *__restrict__ tris,
                                                                      cg_vec4 start, cg_vec4 dir,
                                                                      PickBest *__restrict__ part)
{
    const vec4 s = v4(start.x, start.y, start.z, start.w);
    const vec3 d = v3(dir.x, dir.y, dir.z);
    PickBest b{FLT_MAX, INT_MAX};
    for (int k = blockIdx.x * kPickThreads + threadIdx.x; k < n_tris; k += gridDim.x * kPickThreads) {
        float t, distance;
        if (tri_accepts(tris[k], s, d, t, distance)) b = pick_min(b, PickBest{distance, k});
    }
    b = pick_wave_min(b);
    __shared__ PickBest s_b[kPickThreads / 64];
    if ((threadIdx.x & 63) == 0) s_b[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kPickThreads / 64; ++w) b = pick_min(b, s_b[w]);
        part[blockIdx.x] = b;
    }
}

// One wave: the minimum of the partial results, the winner's record, the spheres.
__global__ __launch_bounds__(64) void rt_pick_final_kernel(RtFrame F, const cg_tri *__restrict__ tris,
                                                           const RtSphere *__restrict__ sph, cg_vec4 start,
                                                           cg_vec4 dir, const PickBest *__restrict__ part, int n_part,
                                                           cg_isect *out, int *hit)
{
    PickBest b{FLT_MAX, INT_MAX};
    for (int k = threadIdx.x; k < n_part; k += 64) b = pick_min(b, part[k]);
    b = pick_wave_min(b);
    if (threadIdx.x != 0) return;
    const vec4 s = v4(start.x, start.y, start.z, start.w);
    const vec3 d = v3(dir.x, dir.y, dir.z);
    cg_isect ci = miss_record();
    if (b.i != INT_MAX) {
        float t, distance;
        if (tri_accepts(tris[b.i], s, d, t, distance)) {
            vec3 td = d * t;
            ci.position = cg_vec4{s.x + td.x, s.y + td.y, s.z + td.z, s.w + 0};
            ci.distance = distance;
            ci.triangleIndex = b.i;
            ci.sphereIndex = -1;
        }
    }
    const vec3 s3 = xyz(s);
    for (int k = 0; k < F.n_sph; ++k) {
        float t;
        if (sphere_intersect(sph[k], s3, d, t)) {
            vec3 td = d * t;
            if (t < ci.distance) {
                ci.position = cg_vec4{s.x + td.x, s.y + td.y, s.z + td.z, s.w + 0};
                ci.distance = t;
                ci.triangleIndex = -1;
                ci.sphereIndex = k;
            }
        }
    }
    *out = ci;
    *hit = ci.distance < FLT_MAX;
}

}  // namespace

void rt_pixel_ray(const cg_rt_camera *cam, int x, int y, int sub_ray, cg_vec4 *start, cg_vec4 *dir)
{
    const vec4 d = pixel_ray(cam->R, cam->width, cam->height, cam->focal, x, y, sub_ray);
    *start = cam->camera;
    *dir = cg_vec4{d.x, d.y, d.z, d.w};
}

hipError_t launch_rt_hits_small(const RtFrame &F, const cg_tri *d_tris, const RtSphere *d_sph, const RtHits &Hs,
                                hipStream_t st)
{
    hipLaunchKernelGGL(rt_hits_small_kernel, dim3((F.W + 63) / 64, (F.rows_out + 3) / 4), dim3(256), 0, st, F, d_tris,
                       d_sph, Hs);
    return hipGetLastError();
}

// scratch: rt_pick_scratch_bytes() of device memory (the workgroups' partial results)
size_t rt_pick_scratch_bytes() { return kPickGroups * sizeof(PickBest); }

hipError_t launch_rt_pick(const RtFrame &F, const cg_tri *d_tris, const RtSphere *d_sph, cg_vec4 start, cg_vec4 dir,
                          void *scratch, cg_isect *d_out, int *d_hit, hipStream_t st)
{
    const int groups = std::max(1, std::min(kPickGroups, (F.n_tris + kPickThreads - 1) / kPickThreads));
    hipLaunchKernelGGL(rt_pick_reduce_kernel, dim3(groups), dim3(kPickThreads), 0, st, F.n_tris, d_tris, start, dir,
                       (PickBest *)scratch);
    hipLaunchKernelGGL(rt_pick_final_kernel, dim3(1), dim3(64), 0, st, F, d_tris, d_sph, start, dir,
                       (const PickBest *)scratch, groups, d_out, d_hit);
    return hipGetLastError();
}

}  // namespace cg
