// cg_api_rt_scene.hip -- the raytracer's device-resident scene and its grid (cg_rt_set_scene*,
// cg_rt_grid_*).  Host code only.
#include <cstring>

#include "cg_ctx.h"

// ---------------------------------------------------------------------------
// RT

// Entry and candidate caps of the scene grid (cg_rt_set_grid_caps; 0 = default).
static constexpr uint64_t kGridEntries = (uint64_t)64 << 20;
static uint64_t grid_entries_cap(const cg_ctx *c)
{
    return std::min<uint64_t>(c->grid_cap_entries > 0 ? (uint64_t)c->grid_cap_entries : kGridEntries, INT_MAX);
}
static uint64_t grid_cands_cap(const cg_ctx *c)
{
    // default: 16 candidate pairs tested per entry the lists may hold
    return std::min<uint64_t>(c->grid_cap_cands > 0 ? (uint64_t)c->grid_cap_cands : 16 * grid_entries_cap(c),
                              (uint64_t)1 << 38);
}

// The part of a scene change both forms share, up to the triangles' arrival: arguments checked by
// the caller.  Frames still in flight on the caller's, auxiliary or slot streams read the scene
// buffers rewritten afterwards (triangles, RtGeo, RtShade): let them finish.
static int scene_begin(cg_ctx *c, int n_tris, int n_spheres)
{
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, hipDeviceSynchronize(), "scene change");
    ++c->rt_scene_gen;
    c->last_masks = {};   // certificates of the previous scene
    size_t nt = n_tris > 0 ? (size_t)n_tris : 1;
    CG_TRY(c, c->tris.ensure(nt * sizeof(cg_tri)), "alloc tris");
    CG_TRY(c, c->tc.ensure(nt * sizeof(RtTri)), "alloc tri constants");
    CG_TRY(c, c->shade.ensure(nt * sizeof(RtShade)), "alloc tri shading");
    CG_TRY(c, c->geo.ensure(nt * sizeof(RtGeo)), "alloc tri geometry");
    CG_TRY(c, c->sph.ensure((size_t)(n_spheres > 0 ? n_spheres : 1) * sizeof(RtSphere)), "alloc spheres");
    return CG_OK;
}

static int scene_spheres(cg_ctx *c, const cg_sphere *spheres, int n_spheres, std::vector<RtSphere> &S, hipStream_t st)
{
    S.resize((size_t)n_spheres);
    for (int i = 0; i < n_spheres; ++i) {
        S[i] = RtSphere{spheres[i].centre.x, spheres[i].centre.y, spheres[i].centre.z,
                        spheres[i].radiusSquared, spheres[i].color.x, spheres[i].color.y,
                        spheres[i].color.z, 0.f};
    }
    if (n_spheres)
        CG_TRY(c, hipMemcpyAsync(c->sph.p, S.data(), S.size() * sizeof(RtSphere),
                                 hipMemcpyHostToDevice, st), "upload spheres");
    return CG_OK;
}

extern "C" int cg_rt_set_scene(cg_ctx *c, const cg_tri *tris, int n_tris, const cg_sphere *spheres,
                               int n_spheres)
{
    if (!c || n_tris < 0 || n_spheres < 0 || (n_tris && !tris) || (n_spheres && !spheres))
        return CG_E_INVALID;
    if (int rc = scene_begin(c, n_tris, n_spheres)) return rc;
    if (n_tris) {
        CG_TRY(c, hipMemcpyAsync(c->tris.p, tris, (size_t)n_tris * sizeof(cg_tri),
                                 hipMemcpyHostToDevice, c->stream), "upload tris");
        // the camera-independent constants (RtGeo) and shading attributes
        // (RtShade), once per scene: every frame, slot and path reads them
        CG_TRY(c, launch_rt_scene((const cg_tri *)c->tris.p, n_tris, (RtGeo *)c->geo.p, (RtShade *)c->shade.p,
                                  c->stream), "rt_scene launch");
    }
    std::vector<RtSphere> S;
    if (int rc = scene_spheres(c, spheres, n_spheres, S, c->stream)) return rc;
    const SceneBounds sb = rt_scene_bounds(tris, n_tris);
    rt_scene_box_from(sb, n_tris, spheres, n_spheres, c->box_lo, c->box_hi);
    c->grid = RtGrid{};
    c->grid_entries = 0;
    c->gbuild.cells = c->gbuild.entries = c->gbuild.cands = 0;
    c->gbuild.phase_live = 0;
    c->big_sized = false;   // the next large-scene frame sizes the pools
    c->hits.sized = false;
    if (n_tris > 64) {   // large scene: grid for the shadow-ray blocker search
        std::vector<int> gs, gt;
        RtGrid g{};
        if (rt_grid_build(tris, n_tris, g, gs, gt, (size_t)grid_entries_cap(c))) {
            CG_TRY(c, c->gstart.ensure(gs.size() * 4), "alloc grid");
            CG_TRY(c, c->gtris.ensure(std::max<size_t>(gt.size(), 1) * 4), "alloc grid");
            CG_TRY(c, hipMemcpy(c->gstart.p, gs.data(), gs.size() * 4, hipMemcpyHostToDevice), "upload grid");
            if (!gt.empty())
                CG_TRY(c, hipMemcpy(c->gtris.p, gt.data(), gt.size() * 4, hipMemcpyHostToDevice), "upload grid");
            g.start = (const int *)c->gstart.p;
            g.tris = (const int *)c->gtris.p;
            c->grid_entries = gt.size();
            c->gbuild.cells = gs.size() - 1;
            c->gbuild.entries = gt.size();
        }
        // hit positions lie on a triangle or a sphere: the box of both
        rt_hit_box_from(sb, spheres, n_spheres, g.blo, g.bhi);
        c->grid = g;
    }
    CG_TRY(c, hipStreamSynchronize(c->stream), "scene upload");
    c->nbound = rt_normal_bound(sb, n_spheres);
    c->n_tris = n_tris;
    c->n_sph = n_spheres;
    return CG_OK;
}

// cg_rt_set_scene for triangles in device memory: the same context state, with the bounds and the
// grid built by cg_rt_grid.hip.  Host waits on `st`: the bounds (after which d_tris has been
// copied and is no longer read), the grid's candidate total, its entry total, and the closing one
// that lets frames on any stream follow.
extern "C" int cg_rt_set_scene_device(cg_ctx *c, const cg_tri *d_tris, int n_tris, const cg_sphere *spheres,
                                      int n_spheres, void *stream)
{
    if (!c || n_tris < 0 || n_spheres < 0 || (n_tris && !d_tris) || (n_spheres && !spheres))
        return CG_E_INVALID;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // waits for the producer of d_tris on `stream` as well
    if (int rc = scene_begin(c, n_tris, n_spheres)) return rc;
    if (n_tris) {
        CG_TRY(c, hipMemcpyAsync(c->tris.p, d_tris, (size_t)n_tris * sizeof(cg_tri), hipMemcpyDeviceToDevice, st),
               "copy tris");
        CG_TRY(c, launch_rt_scene((const cg_tri *)c->tris.p, n_tris, (RtGeo *)c->geo.p, (RtShade *)c->shade.p, st),
               "rt_scene launch");
    }
    std::vector<RtSphere> S;
    if (int rc = scene_spheres(c, spheres, n_spheres, S, st)) return rc;
    c->grid = RtGrid{};
    c->grid_entries = 0;
    c->big_sized = false;
    c->hits.sized = false;
    c->n_tris = -1;   // no scene until the build below is through
    SceneBounds sb;
    CG_TRY(c, rt_grid_bounds_device(c->gbuild, (const cg_tri *)c->tris.p, n_tris, sb, st), "scene bounds");
    rt_scene_box_from(sb, n_tris, spheres, n_spheres, c->box_lo, c->box_hi);
    if (n_tris > 64) {
        RtGrid g{};
        GridDims d;
        if (rt_grid_dims(sb.vmin, sb.vmax, n_tris, d)) {
            for (int k = 0; k < 3; ++k) {
                g.lo[k] = d.lo[k];
                g.res[k] = d.res[k];
            }
            g.h = d.h;
            g.inv_h = d.inv_h;
            bool built = false;
            auto ensure = [&](int which, size_t bytes, void **p) {
                DevBuf &b = which ? c->gtris : c->gstart;
                const hipError_t e = b.ensure(bytes);
                *p = b.p;
                return e;
            };
            CG_TRY(c, rt_grid_build_device(c->gbuild, (const cg_tri *)c->tris.p, n_tris, d, grid_entries_cap(c),
                                           grid_cands_cap(c), ensure, built, st), "grid build");
            if (built) {
                g.start = (const int *)c->gstart.p;
                g.tris = (const int *)c->gtris.p;
                c->grid_entries = c->gbuild.entries;
            }
        }
        rt_hit_box_from(sb, spheres, n_spheres, g.blo, g.bhi);
        c->grid = g;
    }
    CG_TRY(c, hipStreamSynchronize(st), "scene build");
    c->nbound = rt_normal_bound(sb, n_spheres);
    c->n_tris = n_tris;
    c->n_sph = n_spheres;
    return CG_OK;
}

extern "C" int cg_rt_set_grid_caps(cg_ctx *c, long long entries, long long candidates)
{
    if (!c || entries < 0 || candidates < 0) return CG_E_INVALID;
    c->grid_cap_entries = entries;
    c->grid_cap_cands = candidates;
    return CG_OK;
}

extern "C" int cg_rt_grid_dims(const float vmin[3], const float vmax[3], int n_tris, float lo[3], float *h,
                               float *inv_h, int res[3])
{
    if (!vmin || !vmax || !lo || !h || !inv_h || !res) return CG_E_INVALID;
    GridDims d;
    const bool ok = rt_grid_dims(vmin, vmax, n_tris, d);
    for (int k = 0; k < 3; ++k) {
        lo[k] = d.lo[k];
        res[k] = d.res[k];
    }
    *h = d.h;
    *inv_h = d.inv_h;
    return ok ? 1 : 0;
}

extern "C" int cg_rt_grid_get(cg_ctx *c, int res[3], float lo[3], float *h, int *start, size_t start_cap, int *tris,
                              size_t tris_cap, size_t *n_start, size_t *n_entries)
{
    if (!c || !n_start || !n_entries) return CG_E_INVALID;
    if (c->n_tris < 0) return CG_E_NOSCENE;
    *n_start = *n_entries = 0;
    const RtGrid &g = c->grid;
    if (!g.start) return 0;   // no grid
    const size_t cells = (size_t)g.res[0] * g.res[1] * g.res[2];
    *n_start = cells + 1;
    *n_entries = (size_t)c->grid_entries;
    for (int k = 0; k < 3; ++k) {
        if (res) res[k] = g.res[k];
        if (lo) lo[k] = g.lo[k];
    }
    if (h) *h = g.h;
    if (!start && !tris) return 1;   // sizes only
    if ((start && start_cap < *n_start) || (tris && tris_cap < *n_entries)) return CG_E_CAPACITY;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    if (start) CG_TRY(c, hipMemcpy(start, g.start, *n_start * 4, hipMemcpyDeviceToHost), "grid download");
    if (tris && *n_entries) CG_TRY(c, hipMemcpy(tris, g.tris, *n_entries * 4, hipMemcpyDeviceToHost), "grid download");
    return 1;
}

extern "C" int cg_rt_grid_info(cg_ctx *c, uint64_t out[4])
{
    if (!c || !out) return CG_E_INVALID;
    out[0] = c->gbuild.cells;
    out[1] = c->gbuild.entries;
    out[2] = c->gbuild.cands;
    out[3] = (uint64_t)rt_grid_scratch_bytes(c->gbuild);
    return CG_OK;
}

extern "C" int cg_rt_grid_phase_ms(cg_ctx *c, double out[5])
{
    if (!c || !out) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, rt_grid_phase_ms(c->gbuild, out), "grid phase times");
    return CG_OK;
}
