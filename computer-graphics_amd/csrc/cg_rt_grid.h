// cg_rt_grid.h -- what the host builder (rt_grid_build, cg_rt_big.hip) and the device builder
// (cg_rt_grid.hip) of the scene grid share: the sizing rule, a triangle's cell range and the
// triangle-cell test.  Everything here is FP64 / integer code without contraction, so both
// builders compute the same grid bit for bit.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <functional>

#include "cg_internal.h"
#include "cg_own.h"

namespace cg {

// std::min / std::max on doubles, spelled out so that host and device treat a NaN alike
// (the accumulator is kept).
__host__ __device__ inline double grid_min(double a, double b) { return b < a ? b : a; }
__host__ __device__ inline double grid_max(double a, double b) { return a < b ? b : a; }
__host__ __device__ inline float grid_minf(float a, float b) { return b < a ? b : a; }
__host__ __device__ inline float grid_maxf(float a, float b) { return a < b ? b : a; }

// Does the closed triangle v meet the cell box centred at c with half-width
// hw, widened by eps?  Separating-axis test (the box's 3 axes, the
// triangle's normal, the 9 edge x axis products) in FP64 on the float
// vertices; the widening and the 1e-9 relative slack make it a superset of
// the exact overlap, which is all the certified lit search needs (a triangle
// is listed in every cell holding a point of it).
__host__ __device__ inline bool tri_meets_cell(const double v[3][3], const double c[3], double hw, double eps)
{
    const double h = hw + eps;
    double p[3][3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) p[i][k] = v[i][k] - c[k];
    // [min, max] of a, b, d misses [-r, r]
#define CG_GRID_BEYOND(a, b, d, r) \
    (grid_min((a), grid_min((b), (d))) > (r) || grid_max((a), grid_max((b), (d))) < -(r))
    for (int k = 0; k < 3; ++k)
        if (CG_GRID_BEYOND(p[0][k], p[1][k], p[2][k], h)) return false;
    double e[3][3];
    for (int k = 0; k < 3; ++k) {
        e[0][k] = p[1][k] - p[0][k];
        e[1][k] = p[2][k] - p[1][k];
        e[2][k] = p[0][k] - p[2][k];
    }
    const double n[3] = {e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2],
                         e[0][0] * e[1][1] - e[0][1] * e[1][0]};
    const double nd = n[0] * p[0][0] + n[1] * p[0][1] + n[2] * p[0][2];
    if (fabs(nd) > h * (fabs(n[0]) + fabs(n[1]) + fabs(n[2])) * (1.0 + 1e-9)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double ax[3] = {0.0, 0.0, 0.0};   // unit axis a x edge j
            const int b = (a + 1) % 3, d = (a + 2) % 3;
            ax[b] = -e[j][d];
            ax[d] = e[j][b];
            const double q0 = ax[0] * p[0][0] + ax[1] * p[0][1] + ax[2] * p[0][2];
            const double q1 = ax[0] * p[1][0] + ax[1] * p[1][1] + ax[2] * p[1][2];
            const double q2 = ax[0] * p[2][0] + ax[1] * p[2][1] + ax[2] * p[2][2];
            const double r = h * (fabs(ax[0]) + fabs(ax[1]) + fabs(ax[2])) * (1.0 + 1e-9);
            if (CG_GRID_BEYOND(q0, q1, q2, r)) return false;
        }
#undef CG_GRID_BEYOND
    return true;
}

// (int)floor(q) clamped to [0, res - 1].  A quotient outside int (a triangle without one finite
// vertex component keeps the +-FLT_MAX its bounding box starts from) converts to INT_MIN, which
// is what the host's cvttsd2si gives, here on both sides.
__host__ __device__ inline int grid_clamp_cell(double q, int res)
{
    const double f = floor(q);
    int i = (f >= -2147483648.0 && f < 2147483648.0) ? (int)f : INT_MIN;
    i = i > 0 ? i : 0;
    return i < res - 1 ? i : res - 1;
}

// The cells whose widened box meets triangle t's bounding box: c0[a] .. c1[a] per axis.
__host__ __device__ inline void grid_tri_range(const cg_tri &t, const float glo[3], const int res[3], double gh,
                                               double eps, int c0[3], int c1[3])
{
    const float vx[3][3] = {{t.v0.x, t.v0.y, t.v0.z}, {t.v1.x, t.v1.y, t.v1.z}, {t.v2.x, t.v2.y, t.v2.z}};
    for (int a = 0; a < 3; ++a) {
        float mn = FLT_MAX, mx = -FLT_MAX;
        for (int i = 0; i < 3; ++i) {
            mn = grid_minf(mn, vx[i][a]);
            mx = grid_maxf(mx, vx[i][a]);
        }
        c0[a] = grid_clamp_cell(((double)mn - glo[a] - 2.0 * eps) / gh, res[a]);
        c1[a] = grid_clamp_cell(((double)mx - glo[a] + 2.0 * eps) / gh, res[a]);
    }
}

// Centre of cell (x, y, z).
__host__ __device__ inline void grid_cell_centre(const float glo[3], double gh, int x, int y, int z, double c[3])
{
    c[0] = (double)glo[0] + (x + 0.5) * gh;
    c[1] = (double)glo[1] + (y + 0.5) * gh;
    c[2] = (double)glo[2] + (z + 0.5) * gh;
}

// The grid's frame: cubic cells sized for ~1/4 triangle centroid per cell, at most 512 per axis.
struct GridDims {
    float lo[3], h, inv_h;
    int res[3];
};
// Sizing rule of both builders, from the float minimum / maximum of the vertices per axis (NaN
// components ignored; +-INFINITY or +-FLT_MAX where an axis has none) and the triangle count.
// False: no grid (no triangles, or bounds that are not finite).  Host only.
bool rt_grid_dims(const float vmin[3], const float vmax[3], int n, GridDims &d);

// What a scene's triangles contribute to its bounds: the float minimum / maximum of the vertex
// components per axis (start +-INFINITY, NaN ignored) and the largest |normal component|
// (INFINITY when one is not finite; 0 without triangles).
struct SceneBounds {
    float vmin[3] = {INFINITY, INFINITY, INFINITY}, vmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    float nmax = 0.f;
};

// Device builder (cg_rt_grid.hip).  Its scratch is grow-only and lives with the context.
struct GridBuild {
    DevBuf mem[3];                                // bounds partials + totals; per-triangle and per-cell; per-candidate
    Event ev[10];                                 // events 2p, 2p + 1 bracket phase p (created on first use)
    unsigned phase_live = 0;                      // bit p: the latest build recorded phase p
    uint64_t cells = 0, entries = 0, cands = 0;   // of the latest build (cands 0: host build)
};
constexpr int kGridPhases = 5;   // bounds, ranges, count, offsets, fill / order

// Bounds of n device triangles (one pass; the seven floats are read back: one wait on st).
hipError_t rt_grid_bounds_device(GridBuild &gb, const cg_tri *d_tris, int n, SceneBounds &out, hipStream_t st);
// The grid of n device triangles in the frame d.  ensure(0 / 1, bytes, &p) provides the start /
// tris buffers.  built = false: declined (more than max_entries entries or max_cands candidate
// pairs).  Two waits on st (the candidate total, then the entry total); the fill and ordering
// kernels are still queued on st at return.
hipError_t rt_grid_build_device(GridBuild &gb, const cg_tri *d_tris, int n, const GridDims &d, uint64_t max_entries,
                                uint64_t max_cands, const std::function<hipError_t(int, size_t, void **)> &ensure,
                                bool &built, hipStream_t st);
size_t rt_grid_scratch_bytes(const GridBuild &gb);
// Device time of the latest build's phases in ms (-1: not recorded).  Waits for the build.
hipError_t rt_grid_phase_ms(GridBuild &gb, double out[kGridPhases]);

}  // namespace cg
