// cg_api_rt.hip -- the raytracer's entry points with device output: lights, frame shape and
// routes, large-scene pools and slots, hit planes and picking, batched lattice launches, frame
// sequences, assemble / pack / unstripe and the probes.  Host code only.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "cg_ctx.h"

// Lights to the device buffer (ordered on `st`; skipped when unchanged) and
// the light-set summary the shadow certificate uses.
static RtLight rt_light_of(const cg_light &l)
{
    return RtLight{l.position.x, l.position.y, l.position.z, l.position.w, l.colour.x, l.colour.y, l.colour.z, 0.f};
}
// The light set as the shadow certificates see it (RtFrame::lmin .. lrho), for one frame's lights.
static void light_summary(const RtLight *L, int n, float lmin[3], float lmax[3], float lc[3], double &lrho)
{
    for (int k = 0; k < 3; ++k) lmin[k] = lmax[k] = lc[k] = 0.f;
    lrho = 0.0;
    if (n > 0) {
        for (int k = 0; k < 3; ++k) lmin[k] = lmax[k] = (&L[0].x)[k];
        for (int l = 0; l < n; ++l) {
            const RtLight &q = L[l];
            for (int k = 0; k < 3; ++k) {
                lmin[k] = std::min(lmin[k], (&q.x)[k]);
                lmax[k] = std::max(lmax[k], (&q.x)[k]);
            }
        }
        for (int k = 0; k < 3; ++k) lc[k] = 0.5f * lmin[k] + 0.5f * lmax[k];
        double rho = 0.0;
        for (int l = 0; l < n; ++l) {
            const RtLight &q = L[l];
            double dx = (double)q.x - lc[0], dy = (double)q.y - lc[1], dz = (double)q.z - lc[2];
            rho = std::max(rho, std::sqrt(dx * dx + dy * dy + dz * dz));
        }
        lrho = rho > 0.0 ? rho * (1.0 + 1e-9) + 1e-12 : 0.0;
    }
}

static int set_lights(cg_ctx *c, const cg_light *lights, int n, hipStream_t st, RtFrame &F)
{
    std::vector<RtLight> L((size_t)n);
    for (int l = 0; l < n; ++l) L[l] = rt_light_of(lights[l]);
    F.n_lights = n;
    light_summary(L.data(), n, F.lmin, F.lmax, F.lc, F.lrho);
    const bool same = L.size() == c->lights_host.size() &&
                      (L.empty() || std::memcmp(L.data(), c->lights_host.data(), L.size() * sizeof(RtLight)) == 0);
    CG_TRY(c, c->lights.ensure(std::max<size_t>(L.size(), 1) * sizeof(RtLight)), "alloc lights");
    if (!same && n > 0) {
        c->lights_host = L;
        CG_TRY(c, hipMemcpyAsync(c->lights.p, c->lights_host.data(), L.size() * sizeof(RtLight),
                                 hipMemcpyHostToDevice, st), "upload lights");
    }
    F.lights = (const RtLight *)c->lights.p;
    return CG_OK;
}

// The frame's shape and sharding (no scene, lights or device state).
static int frame_shape(const cg_rt_camera *cam, const cg_rt_shard *shard, RtFrame &F)
{
    std::memset(&F, 0, sizeof(F));
    F.W = cam->width;
    F.H = cam->height;
    F.focal = cam->focal;
    F.indirect = cam->indirect;
    F.cam[0] = cam->camera.x; F.cam[1] = cam->camera.y; F.cam[2] = cam->camera.z; F.cam[3] = cam->camera.w;
    std::memcpy(F.R, cam->R, sizeof(F.R));
    cg_rt_shard one{0, 1, kRtTileH, 0, 0, 0, 0};
    const cg_rt_shard *s = shard ? shard : &one;
    if (s->rows > 0) {   // band: rows row0 .. row0 + rows - 1
        if (s->row0 < 0) return CG_E_INVALID;
        F.rank = 0;
        F.nranks = 1;
        F.stripe_h = s->rows;
        F.row0 = s->row0;
        F.rows_out = s->rows;
    } else {
        if (s->rows < 0 || s->nranks < 1 || s->rank < 0 || s->rank >= s->nranks || s->stripe_h <= 0)
            return CG_E_INVALID;
        F.rank = s->rank;
        F.nranks = s->nranks;
        F.stripe_h = s->stripe_h;
        F.rows_out = cg_rt_shard_rows(F.H, s);
    }
    F.out_fmt = CG_PIX_ARGB8888;
    if (s->cols < 0 || s->col0 < 0) return CG_E_INVALID;
    if (s->cols > 0) {   // RGB24 window (checked against the format by the caller)
        if (s->col0 % 16 || s->col0 + s->cols > F.W || (s->cols % 16 && s->col0 + s->cols != F.W))
            return CG_E_INVALID;
        F.wcol0 = s->col0;
        F.wcols = s->cols;
    }
    F.cull_primary = 1;   // exact certificates (cg_rt_dev.h); the probes run without them
    F.cull_shadow = 1;
    return CG_OK;
}

int fill_frame(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
               const cg_rt_shard *shard, hipStream_t st, RtFrame &F)
{
    if (!cam || cam->width <= 0 || cam->height <= 0 || n_lights < 0 || n_lights > kMaxLights ||
        (n_lights && !lights))
        return CG_E_INVALID;
    if (c->n_tris < 0) {
        c->err = "render before cg_rt_set_scene";
        return CG_E_NOSCENE;
    }
    const int rc = frame_shape(cam, shard, F);
    if (rc) return rc;
    F.n_tris = c->n_tris;
    F.n_sph = c->n_sph;
    F.nbound = c->nbound;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    return set_lights(c, lights, n_lights, st, F);
}

// Test hook: rows row0 .. row0 + rows - 1 of the frame by
// the reference's loop with no acceleration (cg_rt_brute.hip), synchronous.
extern "C" int cg_rt_render_brute_device(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cam,
                                         int row0, int rows, uint32_t *d_out, void *stream)
{
    if (!c || !d_out || !cam || row0 < 0 || rows <= 0 || row0 + rows > cam->height || n_lights > 64)
        return CG_E_INVALID;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    RtFrame F;
    int rc = fill_frame(c, lights, n_lights, cam, nullptr, st, F);
    if (rc) return rc;
    CG_TRY(c, rt_render_brute(F, (const cg_tri *)c->tris.p, c->n_tris, (const RtSphere *)c->sph.p, row0, rows, d_out,
                              st),
           "brute-force render");
    return CG_OK;
}

// CG_RT_ROUTE_* of a frame whose shape and counts are set (host only)
static int frame_route(const RtFrame &F)
{
    if (F.n_tris > 64) {   // rt_enqueue_kernels: the large-scene path
        const int m = rt_big_mode(F);
        return m == 0 ? CG_RT_ROUTE_BIG_PIXEL : m == 1 ? CG_RT_ROUTE_BIG_LATTICE : CG_RT_ROUTE_BIG_LATTICE_YAW;
    }
    const int k = rt_lattice_kind(F);
    if (k == 0) return CG_RT_ROUTE_PIXEL;
    if (F.n_lights == 1) return k == 1 ? CG_RT_ROUTE_LATTICE : CG_RT_ROUTE_LATTICE_YAW;
    return k == 1 ? CG_RT_ROUTE_LIGHTS : CG_RT_ROUTE_LIGHTS_YAW;
}

extern "C" int cg_rt_route(const cg_rt_camera *cam, int n_tris, int n_spheres, int n_lights, const cg_rt_shard *shard)
{
    if (!cam || cam->width <= 0 || cam->height <= 0 || n_tris < 0 || n_spheres < 0 || n_lights < 0 ||
        n_lights > kMaxLights)
        return CG_E_INVALID;
    RtFrame F;
    const int rc = frame_shape(cam, shard, F);
    if (rc) return rc;
    F.n_tris = n_tris;
    F.n_sph = n_spheres;
    F.n_lights = n_lights;
    return frame_route(F);
}

// A sequence's runs (cg_rt_sequence_runs): consecutive frames on the same route.  Size, shard and
// light count are the call's, so the route alone separates runs; frames of a lattice run share
// batched launches, the other routes' runs are enqueued frame by frame.
static int sequence_runs(const cg_rt_camera *cams, int n_frames, int n_tris, int n_spheres, int n_lights,
                         const cg_rt_shard *shard, std::vector<int> &start, std::vector<int> &route)
{
    start.clear();
    route.clear();
    if (n_frames < 0 || (n_frames && !cams) || n_tris < 0 || n_spheres < 0 || n_lights < 0 || n_lights > kMaxLights)
        return CG_E_INVALID;
    for (int f = 0; f < n_frames; ++f) {
        if (cams[f].width <= 0 || cams[f].height <= 0 || cams[f].width != cams[0].width ||
            cams[f].height != cams[0].height)
            return CG_E_INVALID;
        RtFrame F;
        const int rc = frame_shape(&cams[f], shard, F);
        if (rc) return rc;
        F.n_tris = n_tris;
        F.n_sph = n_spheres;
        F.n_lights = n_lights;
        const int r = frame_route(F);
        if (route.empty() || route.back() != r) {
            start.push_back(f);
            route.push_back(r);
        }
    }
    start.push_back(n_frames);
    return CG_OK;
}

extern "C" int cg_rt_sequence_runs(const cg_rt_camera *cams, int n_frames, int n_tris, int n_spheres, int n_lights,
                                   const cg_rt_shard *shard, int *run_start, int *run_route, int cap)
{
    if (cap < 0 || (cap && (!run_start || !run_route))) return CG_E_INVALID;
    std::vector<int> start, route;
    const int rc = sequence_runs(cams, n_frames, n_tris, n_spheres, n_lights, shard, start, route);
    if (rc) return rc;
    const int runs = (int)route.size(), n = std::min(runs, cap);
    for (int r = 0; r < n; ++r) {
        run_start[r] = start[r];
        run_route[r] = route[r];
    }
    if (cap > 0) run_start[n] = start[n];   // run_start has cap + 1 entries
    return runs;
}

// A large-scene frame slot's buffers (slot 0: the context's own; slot 1: the
// second frame in flight of rt_render_frames).
struct BigSlot {
    DevBuf *tc, *big, *frame;
    PinnedBuf *demand;   // unsigned long long [4]
    Event *ev;
    bool *ev_live;
};
static BigSlot big_slot(cg_ctx *c, int q)
{
    if (q) {
        cg_ctx::ExtraSlot &x = c->xs[q - 1];
        return BigSlot{&x.tc, &x.big, &x.frame, &x.demand, &x.ev, &x.ev_live};
    }
    return BigSlot{&c->tc, &c->big, &c->frame, &c->big_demand, &c->big_ev, &c->big_ev_live};
}

static bool big_observe(cg_ctx *c, bool sizing, int q);
static bool hits_observe(cg_ctx *c, bool sizing);

// Settle both slots' outstanding pool demand (blocks on their last frames).
static int big_observe_all(cg_ctx *c)
{
    for (int q = 0; q < cg_ctx::kBigSlots; ++q) {
        const BigSlot b = big_slot(c, q);
        if (*b.ev_live) {
            CG_TRY(c, hipEventSynchronize(*b.ev), "pool demand");
            big_observe(c, false, q);
        }
    }
    if (c->hits.ev_live) {   // a hits-only pass reports like a frame
        CG_TRY(c, hipEventSynchronize(c->hits.ev), "pool demand");
        hits_observe(c, false);
    }
    return CG_OK;
}

extern "C" int cg_rt_scratch_info(cg_ctx *c, uint64_t *out)
{
    if (!c || !out) return CG_E_INVALID;
    if (int rc = big_observe_all(c)) return rc;
    const unsigned long long *d = c->big_last;
    out[0] = c->big.bytes;
    for (const auto &x : c->xs) out[0] += x.big.bytes;
    out[0] += c->hits.big.bytes;
    out[1] = d[0] + d[1] + d[2] + d[3];
    const BigCaps &caps = c->big_last_hits ? c->hits.caps : c->big_caps;   // the pools the latest pass listed in
    out[2] = (uint64_t)(caps.sup + caps.bin + caps.sbin + caps.sorted);
    out[3] = (uint64_t)c->big_overflows;
    return CG_OK;
}

extern "C" int cg_rt_tile_masks(cg_ctx *c, int frame, uint64_t *masks, uint64_t *obj_masks, int *info)
{
    if (!c || !info) return CG_E_INVALID;
    const auto &L = c->last_masks;
    info[0] = L.tiles_x;
    info[1] = L.tiles_y;
    info[2] = L.obj ? kObjSlots : 0;
    info[3] = L.frames;
    if (!L.lat) return CG_E_INVALID;
    if (!masks && !obj_masks) return CG_OK;
    if (frame < 0 || frame >= L.frames) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, hipStreamSynchronize(L.st), "tile masks");
    const size_t tiles = (size_t)L.tiles_x * L.tiles_y;
    if (masks)
        CG_TRY(c, hipMemcpy(masks, L.lat + (size_t)frame * tiles * 2, tiles * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost),
               "tile masks");
    if (obj_masks && L.obj)
        CG_TRY(c, hipMemcpy(obj_masks, L.obj + (size_t)frame * tiles * kObjSlots, tiles * kObjSlots * sizeof(uint64_t),
                            hipMemcpyDeviceToHost), "tile masks");
    // tile columns outside a windowed launch are black without a certificate: report empty masks
    for (size_t t = 0; t < tiles; ++t) {
        const int tx = (int)(t % L.tiles_x);
        if (tx >= L.col0 && tx < L.col1) continue;
        if (masks) masks[2 * t] = masks[2 * t + 1] = 0;
        if (obj_masks && L.obj) std::fill(obj_masks + t * kObjSlots, obj_masks + (t + 1) * kObjSlots, (uint64_t)0);
    }
    return CG_OK;
}

extern "C" int cg_rt_lattice_path(cg_ctx *c, int *info)
{
    if (!c || !info) return CG_E_INVALID;
    for (int k = 0; k < 4; ++k) info[k] = c->last_path[k];
    return CG_OK;
}

extern "C" int cg_rt_pool_demand(cg_ctx *c, uint64_t *out)
{
    if (!c || !out) return CG_E_INVALID;
    if (int rc = big_observe_all(c)) return rc;
    for (int k = 0; k < 4; ++k) out[k] = c->big_last[k];
    return CG_OK;
}

extern "C" int cg_rt_set_pool_caps(cg_ctx *c, long long sup, long long bin, long long sbin, long long sorted)
{
    if (!c || sup < 0 || bin < 0 || sbin < 0 || sorted < 0) return CG_E_INVALID;
    if (c->stream) CG_TRY(c, hipDeviceSynchronize(), "drain before resizing pools");
    c->big_fixed = sup > 0 || bin > 0 || sbin > 0 || sorted > 0;
    c->big_caps = c->big_fixed ? BigCaps{sup, bin, sbin, sorted} : BigCaps{};
    c->big_sized = false;
    c->big_key = -1;
    c->big_overflows = 0;
    c->hits.caps = BigCaps{};
    c->hits.sized = false;
    c->hits.key = -1;
    return CG_OK;
}

extern "C" int cg_rt_set_pending_cap(cg_ctx *c, int cap)
{
    if (!c || cap < 0) return CG_E_INVALID;
    c->pend_cap = cap;
    return CG_OK;
}

extern "C" int cg_rt_shard_rows(int height, const cg_rt_shard *shard)
{
    cg_rt_shard one{0, 1, kRtTileH, 0, 0, 0, 0};
    const cg_rt_shard *s = shard ? shard : &one;
    if (height <= 0) return CG_E_INVALID;
    if (s->rows > 0) return s->rows;
    if (s->rows < 0 || s->nranks < 1 || s->stripe_h <= 0) return CG_E_INVALID;
    int stripes = (height + s->stripe_h - 1) / s->stripe_h;
    int per = (stripes + s->nranks - 1) / s->nranks;
    return per * s->stripe_h;
}

static int rt_enqueue_kernels(cg_ctx *c, const RtFrame &F, uint32_t *d_out, hipStream_t st, int slot);

// slot: a large scene's frame slot (rt_render_frames' second frame in flight: 1)
int rt_enqueue(cg_ctx *c, const RtFrame &Fin, void *d_out_v, hipStream_t st, int slot)
{
    // RGB24 output: the lattice kernel stores it directly; the other kernels
    // render ARGB into the context's scratch frame, then one pack pass
    RtFrame F = Fin;
    uint32_t *d_out = (uint32_t *)d_out_v;
    const bool pack = F.out_fmt == CG_PIX_RGB24 && !rt_use_lattice(F);
    if (pack) {
        DevBuf &fr = *big_slot(c, slot).frame;
        CG_TRY(c, fr.ensure((size_t)F.rows_out * F.W * sizeof(uint32_t)), "alloc frame");
        d_out = (uint32_t *)fr.p;
        F.out_fmt = CG_PIX_ARGB8888;
    }
    int rc = rt_enqueue_kernels(c, F, d_out, st, slot);
    if (rc || !pack) return rc;
    CG_TRY(c, launch_rt_pack_rgb24(d_out, F.W, F.rows_out, Fin.wcols ? Fin.wcol0 : 0, Fin.wcols ? Fin.wcols : F.W,
                                   (uint8_t *)d_out_v, st), "pack launch");
    return CG_OK;
}

// The large-scene pools' demand of the latest finished frame: capacities grow
// to 1.25x a demand that came within 80 % of them (so steady frames neither
// overflow nor hold more than ~1.6x what they list); a sizing frame sets them
// to 1.25x its demand either way.  True when the frame overflowed a pool (it
// was still right: the consumers fell back to every triangle).
static bool big_observe(cg_ctx *c, bool sizing, int q)
{
    const BigSlot b = big_slot(c, q);
    std::memcpy(c->big_last, b.demand->p, sizeof(c->big_last));
    const unsigned long long *d = c->big_last;
    long long *cap[4] = {&c->big_caps.sup, &c->big_caps.bin, &c->big_caps.sbin, &c->big_caps.sorted};
    bool over = false;
    for (int k = 0; k < 4; ++k) {
        const long long need = (long long)d[k];
        over |= need > *cap[k];
        if (!c->big_fixed && (sizing || need * 5 > *cap[k] * 4))
            *cap[k] = std::min<long long>(need + need / 4 + 4096, (1ll << 31) - 1);
    }
    if (!sizing) c->big_overflows += over;
    *b.ev_live = false;
    c->big_last_hits = false;
    return over;
}

// Large scene: binned certificates (cg_rt_big.hip).  The first frame of a
// scene (or of a new frame shape / path) is sized first: dry passes of the
// list kernels alone report the pools' demand until it fits (a pass in which
// a list overflowed under-counts what depends on it), then -- when the frame
// shades through per-bin shadow lists -- dry passes up to those lists.  Later
// frames stay asynchronous and grow the pools for the next ones from their
// reported demand; a frame that still overflows renders through the fallback.
static int rt_big_enqueue(cg_ctx *c, const RtFrame &F, uint32_t *d_out, hipStream_t st, int slot)
{
    const BigSlot S = big_slot(c, slot);
    if (!S.demand->p) {
        CG_TRY(c, S.demand->ensure(4 * sizeof(unsigned long long)), "alloc pool demand");
        std::memset(S.demand->p, 0, 4 * sizeof(unsigned long long));
    }
    CG_TRY(c, S.ev->ensure(), "pool event");
    if (c->big_caps.sup == 0) {   // first guess; the first frame corrects it
        const long long g = 2ll * F.n_tris + 65536;
        c->big_caps = BigCaps{g, g, 4096, 2 * g};
    }
    // a new frame shape or path (lattice / per-pixel, many lights) is sized again
    const int mode = rt_big_mode(F);   // per-pixel / lattice / lattice with per-pixel columns
    const int lclass = F.n_lights == 0 ? 0 : F.n_lights <= 7 ? 1 : F.n_lights <= 64 ? 2 : 3;
    const long long key = ((((long long)F.W * 65536 + F.rows_out) * 4 + lclass) * 4 + mode) * 2 + (F.nranks == 1);
    if (key != c->big_key) {
        c->big_key = key;
        c->big_sized = false;
    }
    if (c->big_fixed) c->big_sized = true;
    for (int q = 0; q < cg_ctx::kBigSlots; ++q) {   // any slot's finished frame reports its demand
        const BigSlot b = big_slot(c, q);
        if (*b.ev_live && hipEventQuery(*b.ev) == hipSuccess) big_observe(c, false, q);
    }
    int stage = c->big_sized ? 0 : 1;   // dry stage of the next pass (0: render)
    DevBuf &big = *S.big;
    for (int pass = 0; pass < 8; ++pass) {
        const int dry = pass == 7 ? 0 : stage;
        const size_t need = rt_big_scratch_bytes(F, c->big_caps);
        if ((need > big.bytes || need < big.bytes / 2) && big.p) {   // grow, or give back a sized-down half
            CG_TRY(c, hipDeviceSynchronize(), "drain before resizing scratch");
            big.release();
        }
        CG_TRY(c, big.ensure(need), "alloc large-scene scratch");
        CG_TRY(c, launch_rt_big(F, (RtTri *)S.tc->p, (const RtShade *)c->shade.p, (const RtSphere *)c->sph.p,
                                c->grid, big.p, d_out, st, (const RtGeo *)c->geo.p, (const cg_tri *)c->tris.p,
                                c->pend_cap, c->big_caps,
                                (unsigned long long *)S.demand->p, dry),
               "rt_big launch");
        CG_TRY(c, hipEventRecord(*S.ev, st), "pool event");
        *S.ev_live = true;
        if (!dry) break;
        CG_TRY(c, hipEventSynchronize(*S.ev), "pool demand");
        if (big_observe(c, true, slot)) continue;          // grown: the same stage again
        if (stage == 1 && rt_big_shadow_lists(F)) {
            stage = 2;
        } else {
            c->big_sized = true;                     // fits: the next pass renders
            stage = 0;
        }
    }
    return CG_OK;
}

static int lat_tiles_x_host(const RtFrame &F) { return (F.W + kLatTileW - 1) / kLatTileW; }

// Shadow masks per object for the one-light lattice kernel (kObjSlots, cg_internal.h): each
// 64-point chunk walks the masks of the objects its points hit instead of the tile's union mask.
// CG_OBJ_MASKS=0 (A/B runs and the tests, read per call): the union mask, as before.
static bool obj_masks_on(const RtFrame &F)
{
    const char *e = std::getenv("CG_OBJ_MASKS");
    return !(e && e[0] == '0') && F.n_lights == 1 && F.cull_shadow;
}

static int rt_enqueue_kernels(cg_ctx *c, const RtFrame &F, uint32_t *d_out, hipStream_t st, int slot)
{
    // a large scene's whole frame (prepare .. shading), for the bench's frame figures
    KtScope kt(F.n_tris > 64 && F.cull_primary && F.cull_shadow ? KT_RT_BIG_FRAME : -1, st);
    unsigned long long *lat = nullptr;
    if (rt_use_lattice(F)) {
        CG_TRY(c, c->latmask.ensure(rt_lattice_tiles(F) * 2 * sizeof(unsigned long long)), "alloc lattice masks");
        lat = (unsigned long long *)c->latmask.p;
    }
    RtFrameCams cams{};
    for (int k = 0; k < 4; ++k) cams.c[0][k] = F.cam[k];
    unsigned long long *supm = nullptr, *um = nullptr, *obj = nullptr;
    if (lat && obj_masks_on(F)) {
        CG_TRY(c, c->objmask.ensure(rt_lattice_tiles(F) * kObjSlots * sizeof(unsigned long long)), "alloc object masks");
        obj = (unsigned long long *)c->objmask.p;
    }
    if (lat && rt_lattice_unit_bytes(F, 1)) {
        CG_TRY(c, c->umask.ensure(rt_lattice_unit_bytes(F, 1)), "alloc lattice unit masks");
        um = (unsigned long long *)c->umask.p;
    }
    if (lat) {   // two-level tile certificates: super-tiles, then tiles
        CG_TRY(c, c->supmask.ensure(rt_sup_units(F) * 2 * sizeof(unsigned long long)), "alloc super-tile masks");
        supm = (unsigned long long *)c->supmask.p;
    }
    const BigSlot S = big_slot(c, slot);   // slot 1 only for large scenes (rt_render_frames)
    if (slot) {
        const size_t nt = (size_t)std::max(c->n_tris, 1);
        CG_TRY(c, S.tc->ensure(nt * sizeof(RtTri)), "alloc tri constants");
    }
    // large scenes: the super-bin pass forms the frame's RtTri itself (no prepare launch)
    if (F.n_tris > 64 && F.cull_primary && F.cull_shadow) return rt_big_enqueue(c, F, d_out, st, slot);
    CG_TRY(c, launch_rt_prepare((const cg_tri *)c->tris.p, (const RtGeo *)c->geo.p, c->n_tris, cams, 1,
                                (RtTri *)S.tc->p, st, &F, (const RtSphere *)c->sph.p, lat, supm, nullptr, nullptr, &obj),
           "rt_prepare launch");
    CG_TRY(c, launch_rt_pixels(F, (const RtTri *)c->tc.p, (const RtShade *)c->shade.p,
                               (const RtSphere *)c->sph.p, lat, um, d_out, st, obj), "rt_pixel launch");
    if (lat) {
        c->last_masks.lat = lat;
        c->last_masks.obj = obj;
        c->last_masks.tiles_x = lat_tiles_x_host(F);
        c->last_masks.tiles_y = (int)(rt_lattice_tiles(F) / lat_tiles_x_host(F));
        c->last_masks.frames = 1;
        c->last_masks.col0 = 0;
        c->last_masks.col1 = lat_tiles_x_host(F);
        c->last_masks.st = st;
    }
    return CG_OK;
}

extern "C" int cg_rt_render_device(cg_ctx *c, const cg_light *lights, int n_lights,
                                   const cg_rt_camera *cam, const cg_rt_shard *shard,
                                   uint32_t *d_out, void *stream)
{
    if (!c || !d_out) return CG_E_INVALID;
    RtFrame F;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    int rc = fill_frame(c, lights, n_lights, cam, shard, st, F);
    if (rc) return rc;
    if (F.wcols) return CG_E_INVALID;   // windows are for the RGB24 wire format
    return rt_enqueue(c, F, d_out, st);
}

// ---- hit planes and picking (cg_rt_hits.hip; large scenes: a hits-only pass of cg_rt_big.hip) ----
extern "C" int cg_rt_pixel_ray(const cg_rt_camera *cam, int x, int y, int sub_ray, cg_vec4 *start, cg_vec4 *dir)
{
    if (!cam || !start || !dir || cam->width <= 0 || cam->height <= 0 || sub_ray < 0 || sub_ray > 8 || x < 0 ||
        x >= cam->width || y < 0 || y >= cam->height)
        return CG_E_INVALID;
    rt_pixel_ray(cam, x, y, sub_ray, start, dir);
    return CG_OK;
}

// big_observe for the hits slot: its demand becomes the latest reported one, its own capacities grow.
static bool hits_observe(cg_ctx *c, bool sizing)
{
    cg_ctx::HitsSlot &S = c->hits;
    std::memcpy(c->big_last, S.demand.p, sizeof(c->big_last));
    const unsigned long long *d = c->big_last;
    long long *cap[4] = {&S.caps.sup, &S.caps.bin, &S.caps.sbin, &S.caps.sorted};
    bool over = false;
    for (int k = 0; k < 4; ++k) {
        const long long need = (long long)d[k];
        over |= need > *cap[k];
        if (!c->big_fixed && (sizing || need * 5 > *cap[k] * 4))
            *cap[k] = std::min<long long>(need + need / 4 + 4096, (1ll << 31) - 1);
    }
    if (!sizing) c->big_overflows += over;
    S.ev_live = false;
    c->big_last_hits = true;
    return over;
}

// The hits-only pass of a large scene, sized as rt_big_enqueue sizes a frame: dry passes of the list
// kernels on the first call of a scene or shape, then growth from the demand each call reports.
static int rt_hits_big_enqueue(cg_ctx *c, const RtFrame &F, const RtHits &Hs, hipStream_t st)
{
    cg_ctx::HitsSlot &S = c->hits;
    if (!S.demand.p) {
        CG_TRY(c, S.demand.ensure(4 * sizeof(unsigned long long)), "alloc pool demand");
        std::memset(S.demand.p, 0, 4 * sizeof(unsigned long long));
    }
    CG_TRY(c, S.ev.ensure(), "pool event");
    CG_TRY(c, S.tc.ensure((size_t)std::max(c->n_tris, 1) * sizeof(RtTri)), "alloc tri constants");
    if (c->big_fixed) {
        S.caps = c->big_caps;
    } else if (S.caps.sup == 0) {   // first guess; the first call corrects it
        const long long g = 2ll * F.n_tris + 65536;
        S.caps = BigCaps{g, g, 4096, 2 * g};
    }
    const long long key = ((long long)F.W * 65536 + F.rows_out) * 2 + (F.nranks == 1);
    if (key != S.key) {
        S.key = key;
        S.sized = false;
    }
    if (c->big_fixed) S.sized = true;
    if (S.ev_live && hipEventQuery(S.ev) == hipSuccess) hits_observe(c, false);
    int stage = S.sized ? 0 : 1;
    KtScope kt(KT_RT_HITS_PASS, st);
    for (int pass = 0; pass < 8; ++pass) {
        const int dry = pass == 7 ? 0 : stage;
        const size_t need = rt_big_scratch_bytes(F, S.caps, true);
        if ((need > S.big.bytes || need < S.big.bytes / 2) && S.big.p) {
            CG_TRY(c, hipDeviceSynchronize(), "drain before resizing scratch");
            S.big.release();
        }
        CG_TRY(c, S.big.ensure(need), "alloc hits scratch");
        CG_TRY(c, launch_rt_big(F, (RtTri *)S.tc.p, (const RtShade *)c->shade.p, (const RtSphere *)c->sph.p, c->grid,
                                S.big.p, nullptr, st, (const RtGeo *)c->geo.p, (const cg_tri *)c->tris.p, 0, S.caps,
                                (unsigned long long *)S.demand.p, dry, &Hs),
               "rt_big hits launch");
        CG_TRY(c, hipEventRecord(S.ev, st), "pool event");
        S.ev_live = true;
        if (!dry) break;
        CG_TRY(c, hipEventSynchronize(S.ev), "pool demand");
        if (hits_observe(c, true)) continue;   // grown: the same stage again
        S.sized = true;
        stage = 0;
    }
    return CG_OK;
}

extern "C" int cg_rt_hits_device(cg_ctx *c, const cg_rt_camera *cam, int sub_ray, const cg_rt_shard *shard,
                                 cg_isect *d_isect, int32_t *d_index, float *d_distance, void *stream)
{
    if (!c || !cam || cam->width <= 0 || cam->height <= 0 || sub_ray < 0 || sub_ray > 8 ||
        (!d_isect && !d_index && !d_distance))
        return CG_E_INVALID;
    if (c->n_tris < 0) {
        c->err = "hits before cg_rt_set_scene";
        return CG_E_NOSCENE;
    }
    RtFrame F;
    if (int rc = frame_shape(cam, shard, F)) return rc;
    if (F.wcols) return CG_E_INVALID;   // windows are for the RGB24 wire format
    F.n_tris = c->n_tris;
    F.n_sph = c->n_sph;
    F.nbound = c->nbound;   // no light set: n_lights 0, lights null
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const RtHits Hs{sub_ray, d_isect, d_index, d_distance};
    if (F.n_tris > 64) return rt_hits_big_enqueue(c, F, Hs, st);
    CG_TRY(c, launch_rt_hits_small(F, (const cg_tri *)c->tris.p, (const RtSphere *)c->sph.p, Hs, st), "rt_hits launch");
    return CG_OK;
}

extern "C" int cg_rt_hits(cg_ctx *c, const cg_rt_camera *cam, int sub_ray, cg_isect *isect, int32_t *index,
                          float *distance)
{
    if (!c || !cam || cam->width <= 0 || cam->height <= 0 || (!isect && !index && !distance)) return CG_E_INVALID;
    if (sub_ray < 0 || sub_ray > 8) return CG_E_INVALID;
    if (c->n_tris < 0) return CG_E_NOSCENE;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t n = (size_t)cam->width * cam->height;
    CG_TRY(c, c->hits.planes.ensure(n * (sizeof(cg_isect) + sizeof(int32_t) + sizeof(float))), "alloc hit planes");
    cg_isect *d_isect = (cg_isect *)c->hits.planes.p;
    int32_t *d_index = (int32_t *)(d_isect + n);
    float *d_distance = (float *)(d_index + n);
    cg_rt_shard whole{0, 1, cam->height, 0, cam->height, 0, 0};   // a band of exactly the frame's rows
    if (int rc = cg_rt_hits_device(c, cam, sub_ray, &whole, isect ? d_isect : nullptr, index ? d_index : nullptr,
                                   distance ? d_distance : nullptr, c->stream))
        return rc;
    if (isect) CG_TRY(c, hipMemcpyAsync(isect, d_isect, n * sizeof(cg_isect), hipMemcpyDeviceToHost, c->stream), "d2h");
    if (index) CG_TRY(c, hipMemcpyAsync(index, d_index, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream), "d2h");
    if (distance)
        CG_TRY(c, hipMemcpyAsync(distance, d_distance, n * sizeof(float), hipMemcpyDeviceToHost, c->stream), "d2h");
    CG_TRY(c, hipStreamSynchronize(c->stream), "hits sync");
    return CG_OK;
}

extern "C" int cg_rt_pick(cg_ctx *c, const cg_rt_camera *cam, int x, int y, int sub_ray, cg_isect *out, int *hit)
{
    if (!c || !out || !hit) return CG_E_INVALID;
    cg_vec4 start, dir;
    if (int rc = cg_rt_pixel_ray(cam, x, y, sub_ray, &start, &dir)) return rc;
    if (c->n_tris < 0) return CG_E_NOSCENE;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t part = (rt_pick_scratch_bytes() + 15) & ~(size_t)15;
    CG_TRY(c, c->hits.pick.ensure(part + sizeof(cg_isect) + sizeof(int)), "alloc pick scratch");
    char *p = (char *)c->hits.pick.p;
    cg_isect *d_out = (cg_isect *)(p + part);
    int *d_hit = (int *)(d_out + 1);
    RtFrame F;
    std::memset(&F, 0, sizeof(F));
    F.n_tris = c->n_tris;
    F.n_sph = c->n_sph;
    CG_TRY(c, launch_rt_pick(F, (const cg_tri *)c->tris.p, (const RtSphere *)c->sph.p, start, dir, p, d_out, d_hit,
                             c->stream), "rt_pick launch");
    CG_TRY(c, hipMemcpyAsync(out, d_out, sizeof(cg_isect), hipMemcpyDeviceToHost, c->stream), "d2h");
    CG_TRY(c, hipMemcpyAsync(hit, d_hit, sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h");
    CG_TRY(c, hipStreamSynchronize(c->stream), "pick sync");
    return CG_OK;
}

// Frames f0 .. f0 + nf - 1 of a batch, one prepare + one lattice launch
// (rt_use_lattice(F) holds for every frame; they differ only in cameraPos, or -- a frame
// sequence, d_recs -- in whatever an RtFrameRec holds).

// The launch geometry a lattice order is recorded for (0 never occurs): the
// same key means the same tiles in the same window, so the recording predicts
// the next launch's per-tile cost.  (A different key would still give a valid
// permutation -- the key only avoids a useless order.)
static unsigned long long lat_order_key(const cg_ctx *c, const RtFrame &F)
{
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&h](long long v) { h = (h ^ (unsigned long long)v) * 1099511628211ull; };
    mix(F.W); mix(F.H); mix(F.rows_out); mix(F.row0); mix(F.rank); mix(F.nranks); mix(F.stripe_h);
    mix(F.tx0); mix(F.txn); mix(F.n_lights); mix(F.n_tris); mix(F.n_sph); mix(c->rt_scene_gen);
    uint32_t b;
    std::memcpy(&b, &F.focal, 4); mix(b);
    for (int k : {0, 8, 12}) { std::memcpy(&b, &F.R[k], 4); mix(b); }
    return h | 1ull;
}
// CG_LAT_ORDER (A/B runs): 0 the default dispatch order, 1 frame-major measured order, 2
// interleaved measured order (frame groups, tile-major inside a group; the default).  Measured on
// C2's 20-frame calls (profiles/r05_ab_order.json): interleaved takes the 1/8 bands of the N = 8
// split from 163-169 to 145-168 us (the floor bands gain most: their launch ended on a heavy
// tile's tail), frame-major gains nothing there; both cost whole frames 1-2 % (0.920 -> 0.935 ms
// per 20-frame lattice launch), so only launches of at most kLatOrderRounds rounds of resident
// workgroups take the order (a band's ~13k workgroups: yes; a whole frame's 105k: no).
// Published certificates beside the lattice launch: CG_CERT_CONC=1 (read per call; off by
// default).  Measured on one MI355X (profiles/r06_ab_conc.json, the driver's 20-frame C2 call):
// 14.2-14.5k frames/s against 18.7-18.9k with the certificates first -- once the lattice launch
// holds the CUs the certificate launch is dispatched only as its workgroups retire (its span
// 80 -> 420 us; a high-priority auxiliary stream changes nothing), so lattice workgroups wait for
// their words or, past the bound, render uncertified, which costs ~15x a certified tile (every
// tile uncertified: 1.45k frames/s).  The path stays as the uncertified-path exactness test
// (CG_LAT_FORCE_UNCERT=1, tests/test_rt_conc_gpu.py).
static bool cert_concurrent()
{
    const char *e = std::getenv("CG_CERT_CONC");
    return e && e[0] == '1';
}
// How long a lattice workgroup waits for its published certificates before it renders the tile
// uncertified: wall-clock ticks (100 MHz), default 1 ms; CG_LAT_SPIN for A/B runs (0: never wait).
static uint32_t lat_spin_ticks()
{
    const char *e = std::getenv("CG_LAT_SPIN");
    return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 100000u;
}

static int lat_order_mode()
{
    static const int m = [] {
        const char *e = std::getenv("CG_LAT_ORDER");
        return e && *e ? std::atoi(e) : 2;
    }();
    return m;
}
constexpr long long kLatOrderRounds = 12;
static long long lat_resident_wgs()
{
    static const long long r = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return (long long)cus * 6;   // rt_lattice_kernel: 6 workgroups per CU
    }();
    return r;
}

static int rt_enqueue_lattice_batch(cg_ctx *c, const RtFrame &F0, const cg_rt_camera *cams, int nf,
                                    void *d_out, size_t stride, hipStream_t st, uint32_t *d_done,
                                    uint32_t *tiles_per_frame, const uint8_t *groups, int ngroups,
                                    const RtFrameRec *d_recs = nullptr, bool uniform = true,
                                    hipEvent_t uploaded = nullptr)
{
    // d_recs (frame sequences): the launch's per-frame records on the device -- the frames may
    // differ in focal, indirect, R (within F0's lattice kind) and lights too; F0 is the first
    // frame's.  uniform: every frame shares F0's focal and R (the measured order is keyed on them).
    // uploaded: recorded on st after the records' upload (certificates on aux wait for it).
    // Workgroups only for the tile columns the scene's box can be seen in by
    // some camera of the batch (O(1) per camera from the box, rt_box_columns);
    // the launch's edge workgroups store the rest black.  C2: 73 of 120 tile
    // columns -- the other 47 cost a workgroup each (~1.6 us) per tile row.
    RtFrame F = F0;
    static const bool window = [] {   // CG_LAT_WINDOW=0: every tile column (A/B runs)
        const char *e = std::getenv("CG_LAT_WINDOW");
        return !(e && e[0] == '0');
    }();
    if (window) {
        int a = F.W, b = 0;
        for (int f = 0; f < nf; ++f) {
            int c0, c1;
            ctx_rt_columns(c, &cams[f], &c0, &c1);
            if (c0 < c1) {
                a = std::min(a, c0);
                b = std::max(b, c1);
            }
        }
        const int tx = (F.W + kLatTileW - 1) / kLatTileW;
        int t0 = a / kLatTileW, t1 = (b + kLatTileW - 1) / kLatTileW;
        if (t0 >= t1) {   // nothing visible: one tile column (certified black) and the edges
            t0 = 0;
            t1 = 1;
        }
        if (t0 > 0 || t1 < tx) {
            F.tx0 = t0;
            F.txn = t1 - t0;
        }
    }
    *tiles_per_frame = (uint32_t)((F.txn ? F.txn : (F.W + kLatTileW - 1) / kLatTileW) *
                                  ((F.rows_out + kLatTileH - 1) / kLatTileH));
    if (!c->aux) {
        // default priority: a high-priority auxiliary stream (certificates
        // dispatched ahead of a running lattice launch) gained ~2 % on
        // back-to-back calls, but left the process's later streams sharing
        // hardware queues -- the rasteriser's overlapped frames then ran
        // serialised (C3 10.1-11.1k instead of 21.0-21.3k frames/s)
        {
            // A/B knob: CG_AUX_PRIO=1 creates the auxiliary stream at the highest priority
            const char *pe = std::getenv("CG_AUX_PRIO");
            int lo = 0, hi = 0;
            if (pe && pe[0] == '1' && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
                CG_TRY(c, c->aux.ensure_priority(hipStreamNonBlocking, hi), "aux stream");
            else
                CG_TRY(c, c->aux.ensure(hipStreamNonBlocking), "aux stream");
        }
        for (int k = 0; k < 2; ++k) {
            CG_TRY(c, c->ev_cert[k].ensure(), "aux event");
            CG_TRY(c, c->ev_lat[k].ensure(), "aux event");
            CG_TRY(c, hipEventRecord(c->ev_lat[k], c->aux), "aux event");
        }
    }
    // this call's slot (its buffers were last read by the lattice launch two
    // calls ago, ev_lat[k])
    const int k = c->slot;
    c->slot ^= 1;
    DevBuf &btc = c->ptc[k], &blat = c->plat[k], &bsup = c->psup[k], &bum = c->pumask[k];
    const size_t tiles = rt_lattice_tiles(F);
    // Both slots' certificate buffers are sized together, for a full batch
    // (kMaxFrameBatch frames): a call never allocates -- hipMalloc / hipFree,
    // the latter a device-wide wait -- in front of its kernels merely because
    // it batches more frames than the previous one or is the first on its
    // slot.  The light sets' unit masks (40 MB per 4K frame) are the
    // exception: they are sized for the largest batch this context has asked
    // for so far (a one-frame or band call keeps ~40 MB per slot, not 1.3 GB),
    // growing both slots together when a call batches more.
    const size_t nfa = std::max(nf, kMaxFrameBatch);
    for (int q = 0; q < 2; ++q) {
        CG_TRY(c, c->plat[q].ensure(nfa * tiles * 2 * sizeof(unsigned long long)), "alloc lattice masks");
        CG_TRY(c, c->ptc[q].ensure(nfa * std::max(F.n_tris, 1) * sizeof(RtTri)), "alloc tri constants");
        CG_TRY(c, c->psup[q].ensure(nfa * rt_sup_units(F) * 2 * sizeof(unsigned long long)), "alloc super-tile masks");
        if (obj_masks_on(F))
            CG_TRY(c, c->pobj[q].ensure(nfa * tiles * kObjSlots * sizeof(unsigned long long)), "alloc object masks");
    }
    if (rt_lattice_unit_bytes(F, nf)) {
        c->umask_frames = std::max(c->umask_frames, nf);
        for (int q = 0; q < 2; ++q)
            CG_TRY(c, c->pumask[q].ensure(rt_lattice_unit_bytes(F, c->umask_frames)), "alloc lattice unit masks");
    }
    RtFrameCams fc{};
    for (int f = 0; f < nf; ++f) {
        fc.c[f][0] = cams[f].camera.x; fc.c[f][1] = cams[f].camera.y;
        fc.c[f][2] = cams[f].camera.z; fc.c[f][3] = cams[f].camera.w;
    }
    unsigned long long *lat = (unsigned long long *)blat.p;
    unsigned long long *supm = (unsigned long long *)bsup.p;
    unsigned long long *obj = obj_masks_on(F) ? (unsigned long long *)c->pobj[k].p : nullptr;
    const bool cold = hipEventQuery(c->ev_lat[0]) == hipSuccess && hipEventQuery(c->ev_lat[1]) == hipSuccess;
    // Measured order (one-light lattice kernel): sort the latest complete
    // recording of this geometry -- the other slot's (the previous call) when
    // every lattice launch is done, else this slot's (two calls ago, complete:
    // cst waited on it) -- in the certificate launch; this launch records into
    // this slot.
    const int gx = F.txn ? F.txn : lat_tiles_x_host(F), gy = (F.rows_out + kLatTileH - 1) / kLatTileH;
    const unsigned long long key = lat_order_key(c, F);
    LatOrder order{};
    LatFlatten flat{};
    const bool ordered = lat_order_mode() > 0 && F.n_lights == 1 && uniform &&
                         (long long)gx * gy * nf <= kLatOrderRounds * lat_resident_wgs();
    // Published certificates (LatReady, cg_internal.h): the one-light lattice
    // launch starts beside its certificate launch instead of after it, each
    // workgroup waiting only for its own super-tile (calls in the default
    // order: whole frames; band calls keep the measured order, whose sort the
    // certificate launch does first)
    const bool conc = cert_concurrent() && !ordered && F.n_lights == 1 && F.n_tris <= 62 &&
                      !rt_lattice_unit_bytes(F, nf) && !d_recs;   // sequences: certificates first
    // certificates on aux, after the slot's previous reader, so that they run
    // beside the lattice launch still queued before them (or, published, beside
    // this call's own).  A cold call with unpublished certificates (every
    // earlier lattice launch of this context complete: nothing to run beside)
    // keeps them on the caller's stream -- the cross-stream wait would leave
    // the GPU idle for ~12 us between certificates and lattice.
    hipStream_t cst = (cold && !conc) ? st : c->aux;
    if (!cold) CG_TRY(c, hipStreamWaitEvent(cst, c->ev_lat[k], 0), "aux wait");
    if (d_recs && cst != st) CG_TRY(c, hipStreamWaitEvent(cst, uploaded, 0), "aux wait");
    LatPublish pub{};
    LatReady ready{};
    if (conc) {
        const size_t units = rt_sup_units(F), words = nfa * units;
        for (int q = 0; q < 2; ++q) {
            const size_t had = c->pflag[q].bytes;
            CG_TRY(c, c->pflag[q].ensure(words * sizeof(uint32_t)), "alloc certificate words");
            if (c->pflag[q].bytes != had) {   // fresh words: zero (no generation), before any launch reads them
                CG_TRY(c, hipMemsetAsync(c->pflag[q].p, 0, c->pflag[q].bytes, st), "zero certificate words");
                CG_TRY(c, hipStreamSynchronize(st), "zero certificate words");
            }
        }
        uint32_t gen = ++c->cert_gen;
        if (gen == 0u) gen = ++c->cert_gen;
        pub = LatPublish{(uint32_t *)c->pflag[k].p, gen, (int)units};
        const char *fe = std::getenv("CG_LAT_FORCE_UNCERT");   // test hook, read per call
        ready = LatReady{(const uint32_t *)c->pflag[k].p, gen, (int)units, (lat_tiles_x_host(F) + kSup - 1) / kSup,
                         fe && fe[0] == '1', lat_spin_ticks(), (const RtGeo *)c->geo.p, (RtTri *)btc.p};
    }
    if (ordered) {
        for (int q = 0; q < 2; ++q) {
            // a reallocated cost map holds no recording: forget both slots' keys, or a later
            // call of the earlier geometry would sort uninitialised memory
            if ((size_t)gx * gy > c->lcost[q].bytes) c->lrec_key[0] = c->lrec_key[1] = 0ull;
            CG_TRY(c, c->lcost[q].ensure((size_t)gx * gy), "alloc lattice order");
            CG_TRY(c, c->lflat[q].ensure((size_t)gx * gy * sizeof(uint32_t)), "alloc lattice order");
        }
        const int src = (cold && c->lrec_key[k ^ 1] == key) ? (k ^ 1) : c->lrec_key[k] == key ? k : -1;
        if (src >= 0) flat = LatFlatten{(const uint8_t *)c->lcost[src].p, (uint32_t *)c->lflat[k].p, gx * gy};
    }
    CG_TRY(c, launch_rt_prepare((const cg_tri *)c->tris.p, (const RtGeo *)c->geo.p, c->n_tris, fc, nf,
                                (RtTri *)btc.p, cst, &F, (const RtSphere *)c->sph.p, lat, supm,
                                flat.n > 0 ? &flat : nullptr, conc ? &pub : nullptr, &obj, d_recs),
           "rt_prepare launch");
    if (conc && !pub.done) ready = LatReady{};   // not published (the split certificate form): nothing to wait for
    if (ordered) {
        if (flat.n < 0) order.flat = (const uint32_t *)c->lflat[k].p;   // sorted by the certificate launch
        order.cost = (uint8_t *)c->lcost[k].p;
        c->lrec_key[k] = key;
        order.ngroups = -1;   // frame-major
        if (lat_order_mode() == 2) {
            order.ngroups = 0;
            if (groups && ngroups > 0 && ngroups <= kLatMaxGroups) {
                order.ngroups = ngroups;
                for (int g = 0; g <= ngroups; ++g) order.gs[g] = groups[g];
            }
        }
    }
    // light sets: the per-unit shadow certificates, with the other certificates
    unsigned long long *um = nullptr;
    if (rt_lattice_unit_bytes(F, nf)) {
        um = (unsigned long long *)bum.p;
        CG_TRY(c, launch_rt_lattice_units(F, (const RtTri *)btc.p, (const RtShade *)c->shade.p, (const RtSphere *)c->sph.p,
                                          lat, fc, nf, um, cst, d_recs),
               "rt_lattice_units launch");
    }
    if (!cold || conc) CG_TRY(c, hipEventRecord(c->ev_cert[k], cst), "aux record");
    if (!cold && !conc) CG_TRY(c, hipStreamWaitEvent(st, c->ev_cert[k], 0), "aux wait");
    CG_TRY(c, launch_rt_lattice_frames(F, (const RtTri *)btc.p, (const RtShade *)c->shade.p,
                                       (const RtSphere *)c->sph.p, lat, um, fc, nf, stride, (uint32_t *)d_out, st,
                                       d_done, ordered ? &order : nullptr, ready.flags ? &ready : nullptr, obj,
                                       d_recs),
           "rt_lattice launch");
    c->last_path[0] = ordered ? (order.ngroups < 0 ? 1 : 2) : 0;
    c->last_path[1] = ready.flags != nullptr;
    c->last_path[2] = ready.flags != nullptr && ready.force;
    c->last_path[3] = (int)std::min<long long>((long long)gx * gy * nf, INT_MAX);
    c->last_masks.lat = lat;
    c->last_masks.obj = obj;
    c->last_masks.tiles_x = lat_tiles_x_host(F);
    c->last_masks.tiles_y = (int)(tiles / lat_tiles_x_host(F));
    c->last_masks.frames = nf;
    c->last_masks.col0 = F.txn ? F.tx0 / kSup * kSup : 0;
    c->last_masks.col1 = F.txn ? std::min(lat_tiles_x_host(F), (F.tx0 + F.txn + kSup - 1) / kSup * kSup) : lat_tiles_x_host(F);
    c->last_masks.st = st;
    // published: whatever the caller queues after this call follows the certificates too
    if (conc) CG_TRY(c, hipStreamWaitEvent(st, c->ev_cert[k], 0), "aux wait");
    CG_TRY(c, hipEventRecord(c->ev_lat[k], st), "aux record");
    return CG_OK;
}

// Large-scene frames in flight: 2 by default; CG_BIG_SLOTS = 1 .. kBigSlots for A/B runs.
static int big_slots()
{
    static const int n = [] {
        const char *e = std::getenv("CG_BIG_SLOTS");
        const int v = e ? std::atoi(e) : 2;
        return std::max(1, std::min(v, cg_ctx::kBigSlots));
    }();
    return n;
}

extern "C" int cg_pix_bytes(int pix_format)
{
    switch (pix_format) {
    case CG_PIX_ARGB8888: return 4;
    case CG_PIX_RGB24: return 3;
    case CG_PIX_RGBA_F32: return 16;
    default: return CG_E_INVALID;
    }
}

extern "C" int cg_rt_render_frames_device(cg_ctx *c, const cg_light *lights, int n_lights,
                                          const cg_rt_camera *cams, int n_frames, const cg_rt_shard *shard,
                                          void *d_out, size_t frame_stride, int pix_format, void *stream)
{
    return rt_render_frames(c, lights, n_lights, cams, n_frames, shard, d_out, frame_stride, pix_format, stream,
                            nullptr, nullptr, nullptr, 0, 0);
}

extern "C" int cg_rt_render_sequence_device(cg_ctx *c, const cg_light *lights, int n_lights,
                                            const cg_rt_camera *cams, int n_frames, const cg_rt_shard *shard,
                                            void *d_out, size_t frame_stride, int pix_format, void *stream)
{
    if (n_lights < 0 || n_lights > kMaxLights || (n_lights && !lights)) return CG_E_INVALID;
    return rt_render_frames(c, lights, n_lights, cams, n_frames, shard, d_out, frame_stride, pix_format, stream,
                            nullptr, nullptr, nullptr, 0, std::max(n_lights, 1));
}

// Frames first .. first + count - 1 of a call one by one (rt_enqueue), frame f as fill(f, F) sets
// it.  Large scenes: consecutive frames are dealt round-robin to big_slots() slots, each with its
// own buffers and stream: independent frames in flight.
template <class Fill>
static int rt_enqueue_each(cg_ctx *c, int first, int count, bool big, uint8_t *out, size_t fbytes, hipStream_t st,
                           uint32_t *d_done, uint32_t *target, Fill fill)
{
    const int ns = (count > 1 && big) ? std::min(big_slots(), count) : 1;
    if (ns > 1) {
        CG_TRY(c, c->bev_start.ensure(), "slot event");
        // the other slots start after what the caller queued before this
        // call (the scene, the lights just uploaded on st)
        CG_TRY(c, hipEventRecord(c->bev_start, st), "slot event");
        for (int q = 1; q < ns; ++q) {
            cg_ctx::ExtraSlot &x = c->xs[q - 1];
            CG_TRY(c, x.st.ensure(hipStreamNonBlocking), "slot stream");
            CG_TRY(c, x.done.ensure(), "slot event");
            CG_TRY(c, hipStreamWaitEvent(x.st, c->bev_start, 0), "slot wait");
        }
    }
    for (int i = 0; i < count; ++i) {
        const int f = first + i;
        RtFrame F;
        int rc = fill(f, F);
        if (rc) return rc;
        const int q = i % ns;
        hipStream_t fs = q ? c->xs[q - 1].st : st;
        rc = rt_enqueue(c, F, out + (size_t)f * fbytes, fs, q);
        if (rc) return rc;
        if (d_done) {
            CG_TRY(c, hipStreamWriteValue32(fs, d_done + f, 1u, 0), "frame signal");
            target[f] = 1u;
        }
    }
    for (int q = 1; q < ns; ++q) {   // the call ends on the caller's stream
        cg_ctx::ExtraSlot &x = c->xs[q - 1];
        CG_TRY(c, hipEventRecord(x.done, x.st), "slot event");
        CG_TRY(c, hipStreamWaitEvent(st, x.done, 0), "slot wait");
    }
    return CG_OK;
}

// cg_rt_render_sequence_device (validated by rt_render_frames; F0: frame 0's shape): the call's
// lights and per-frame records go to the device once, then each run (sequence_runs) is enqueued --
// lattice runs kMaxFrameBatch frames a launch over their records, the others frame by frame, each
// frame with its own region of the uploaded lights.
static int rt_enqueue_sequence(cg_ctx *c, const RtFrame &F0, const cg_light *lights, int n_lights,
                               const cg_rt_camera *cams, int n_frames, const cg_rt_shard *shard, uint8_t *out,
                               size_t stride, size_t fbytes, int pix_format, hipStream_t st)
{
    std::vector<int> start, route;
    int rc = sequence_runs(cams, n_frames, c->n_tris, c->n_sph, n_lights, shard, start, route);
    if (rc) return rc;
    // the slot: lights (n_frames x n_lights RtLight), then the records
    const size_t lbytes = (size_t)n_frames * n_lights * sizeof(RtLight), rbytes = (size_t)n_frames * sizeof(RtFrameRec);
    const size_t bytes = lbytes + rbytes;
    if (bytes > c->seq[0].dev.bytes || bytes > c->seq[0].host.bytes) {
        const size_t grow = bytes + bytes / 2;   // a somewhat longer call later allocates nothing
        CG_TRY(c, hipDeviceSynchronize(), "drain before resizing sequence slots");
        for (auto &q : c->seq) {
            CG_TRY(c, q.dev.ensure(grow), "alloc sequence slot");
            CG_TRY(c, q.host.ensure(grow), "alloc sequence staging");
            if (!q.up || !q.done) {
                CG_TRY(c, q.up.ensure(), "sequence event");
                CG_TRY(c, q.done.ensure(), "sequence event");
                CG_TRY(c, hipEventRecord(q.up, st), "sequence event");
                CG_TRY(c, hipEventRecord(q.done, st), "sequence event");
            }
        }
    }
    cg_ctx::SeqSlot &S = c->seq[c->seq_slot];
    c->seq_slot ^= 1;
    // the staging memory: free once the slot's previous upload (two calls ago, at the head of that
    // call's work) is done -- the one host wait of a sequence call: a third call queued with no
    // wait since the first blocks here until the stream has reached the first call's upload; the
    // device copy: once that call's kernels are (any stream, no host wait)
    CG_TRY(c, hipEventSynchronize(S.up), "sequence staging");
    CG_TRY(c, hipStreamWaitEvent(st, S.done, 0), "sequence slot wait");
    // from here on the slot is this call's: whatever happens below, `done` is recorded behind what
    // was enqueued, so that a later call's wait on the slot covers it and nothing more
    struct Done {
        hipEvent_t ev;
        hipStream_t st;
        ~Done() { (void)hipEventRecord(ev, st); }
    } done_on_exit{S.done, st};
    RtLight *hl = (RtLight *)S.host.p;
    RtFrameRec *hr = (RtFrameRec *)((uint8_t *)S.host.p + lbytes);
    const RtLight *dl = (const RtLight *)S.dev.p;
    const RtFrameRec *dr = (const RtFrameRec *)((const uint8_t *)S.dev.p + lbytes);
    for (size_t l = 0; l < (size_t)n_frames * n_lights; ++l) hl[l] = rt_light_of(lights[l]);
    for (int f = 0; f < n_frames; ++f) {
        RtFrameRec &r = hr[f];
        std::memset(&r, 0, sizeof(r));
        r.cam[0] = cams[f].camera.x; r.cam[1] = cams[f].camera.y; r.cam[2] = cams[f].camera.z; r.cam[3] = cams[f].camera.w;
        r.focal = cams[f].focal;
        r.indirect = cams[f].indirect;
        std::memcpy(r.R, cams[f].R, sizeof(r.R));
        light_summary(hl + (size_t)f * n_lights, n_lights, r.lmin, r.lmax, r.lc, r.lrho);
        r.light_off = (uint32_t)((size_t)f * n_lights);
    }
    CG_TRY(c, hipMemcpyAsync(S.dev.p, S.host.p, bytes, hipMemcpyHostToDevice, st), "upload sequence");
    CG_TRY(c, hipEventRecord(S.up, st), "sequence event");
    // frame f as rt_enqueue and the lattice launches take it: its shape, the scene, its record
    auto frame_of = [&](int f, RtFrame &F) -> int {
        const int e = frame_shape(&cams[f], shard, F);
        if (e) return e;
        F.n_tris = F0.n_tris;
        F.n_sph = F0.n_sph;
        F.nbound = F0.nbound;
        F.n_lights = n_lights;
        for (int k = 0; k < 3; ++k) {
            F.lmin[k] = hr[f].lmin[k];
            F.lmax[k] = hr[f].lmax[k];
            F.lc[k] = hr[f].lc[k];
        }
        F.lrho = hr[f].lrho;
        F.lights = dl + (size_t)f * n_lights;
        F.out_fmt = pix_format;
        return CG_OK;
    };
    for (size_t r = 0; r < route.size() && !rc; ++r) {
        const int a = start[r], b = start[r + 1], rt = route[r];
        const bool lattice = rt == CG_RT_ROUTE_LATTICE || rt == CG_RT_ROUTE_LATTICE_YAW || rt == CG_RT_ROUTE_LIGHTS ||
                             rt == CG_RT_ROUTE_LIGHTS_YAW;
        if (!lattice) {
            rc = rt_enqueue_each(c, a, b - a, c->n_tris > 64, out, fbytes, st, nullptr, nullptr, frame_of);
            continue;
        }
        for (int f0 = a; f0 < b && !rc; f0 += kMaxFrameBatch) {
            const int nf = std::min(kMaxFrameBatch, b - f0);
            RtFrame F;
            if ((rc = frame_of(f0, F))) break;
            F.lights = dl;   // the records' light_off counts from the call's array
            bool uniform = true;
            for (int f = f0 + 1; f < f0 + nf && uniform; ++f)
                uniform = std::memcmp(&cams[f].focal, &cams[f0].focal, sizeof(float)) == 0 &&
                          std::memcmp(cams[f].R, cams[f0].R, sizeof(cams[f0].R)) == 0;
            uint32_t wg = 0;
            rc = rt_enqueue_lattice_batch(c, F, cams + f0, nf, out + (size_t)f0 * fbytes, stride, st, nullptr, &wg,
                                          nullptr, 0, dr + f0, uniform, S.up);
        }
    }
    return rc;
}

namespace cg {
// cg_rt_render_frames_device, plus per-frame completion signals for cg_dist:
// with d_done (signal memory, zeroed by the caller), frame f is complete once
// d_done[f] >= target[f] (the lattice kernels count the frame's tiles as they
// are stored; other paths write 1 after the frame's kernels).
// group_starts (optional, ngroups + 1 entries, the last n_frames): frames
// dispatched group after group (cg_dist's chunks, sent as each completes).
int rt_render_frames(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cams, int n_frames,
                     const cg_rt_shard *shard, void *d_out, size_t frame_stride, int pix_format, void *stream,
                     uint32_t *d_done, uint32_t *target, const int *group_starts, int ngroups, int light_stride)
{
    if (!c || !d_out || n_frames < 0 || (n_frames && !cams)) return CG_E_INVALID;
    if (cg_pix_bytes(pix_format) < 0) return CG_E_INVALID;
    if (pix_format == CG_PIX_RGBA_F32 && ((uintptr_t)d_out & 15)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    for (int f = 1; f < n_frames; ++f)
        if (cams[f].width != cams[0].width || cams[f].height != cams[0].height) return CG_E_INVALID;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    RtFrame F;
    int rc = fill_frame(c, lights, n_lights, &cams[0], shard, st, F);
    if (rc) return rc;
    F.out_fmt = pix_format;
    if (F.wcols && pix_format != CG_PIX_RGB24) return CG_E_INVALID;
    const size_t px = (size_t)F.rows_out * (F.wcols ? F.wcols : F.W);
    const size_t stride = frame_stride ? frame_stride : px;   // pixels
    if (stride < px) return CG_E_INVALID;
    uint8_t *out = (uint8_t *)d_out;
    const size_t fbytes = stride * (size_t)cg_pix_bytes(pix_format);
    // light_stride != 0: frame f has its own lights, lights[f * n_lights ..] (cg_rt_render_sequence_device)
    if (light_stride) return rt_enqueue_sequence(c, F, lights, n_lights, cams, n_frames, shard, out, stride, fbytes,
                                                 pix_format, st);
    // one batched launch needs the lattice path for every frame, frames that
    // differ only in cameraPos (same focal, R, indirect)
    bool batch = rt_use_lattice(F);
    for (int f = 1; batch && f < n_frames; ++f)
        batch = cams[f].focal == cams[0].focal && cams[f].indirect == cams[0].indirect &&
                std::memcmp(cams[f].R, cams[0].R, sizeof(cams[0].R)) == 0;
    if (!batch)
        return rt_enqueue_each(c, 0, n_frames, F.n_tris > 64 && F.cull_primary && F.cull_shadow, out, fbytes, st, d_done,
                               target, [&](int f, RtFrame &Ff) -> int {
                                   if (f == 0) {   // filled above
                                       Ff = F;
                                       return CG_OK;
                                   }
                                   const int e = fill_frame(c, lights, n_lights, &cams[f], shard, st, Ff);
                                   Ff.out_fmt = pix_format;
                                   return e;
                               });
    // (A cold call split into a head batch, whose lattice launch runs beside
    // the rest's certificates on a high-priority auxiliary stream, measured
    // slower: 16.0k against 17.2k frames/s for the driver's 20-frame C2 call --
    // the certificates beside a lattice launch took 0.56 ms instead of 0.12.)
    for (int f0 = 0; f0 < n_frames;) {
        const int nf = std::min(kMaxFrameBatch, n_frames - f0);
        uint32_t wg = 0;
        uint8_t gs[kLatMaxGroups + 1];   // the groups within this launch's frames
        int ng = 0;
        if (group_starts && ngroups > 0) {
            gs[0] = 0;
            for (int g = 1; g <= ngroups && ng < kLatMaxGroups; ++g) {
                const int e = std::min(group_starts[g], f0 + nf) - f0;
                if (e > gs[ng]) gs[++ng] = (uint8_t)e;
            }
            if (ng == 0 || gs[ng] != nf) ng = 0;   // not covering the launch: one group
        }
        rc = rt_enqueue_lattice_batch(c, F, cams + f0, nf, out + (size_t)f0 * fbytes, stride, st,
                                      d_done ? d_done + f0 : nullptr, &wg, ng ? gs : nullptr, ng);
        if (rc) return rc;
        if (d_done)
            for (int f = f0; f < f0 + nf; ++f) target[f] = wg;   // the launch's workgroups per frame
        f0 += nf;
    }
    return CG_OK;
}
}  // namespace cg

extern "C" int cg_rt_assemble_device(cg_ctx *c, const void *d_src, int pix_format, const int *row0,
                                     const int *rows, int n_blocks, int width, int height, int n_frames,
                                     uint32_t *d_frames, size_t frame_stride, int col0, int cols, void *stream)
{
    if (cols < 0 || col0 < 0 || (cols > 0 && (col0 % 4 || cols % 4 || col0 + cols > width))) return CG_E_INVALID;
    if (!c || !d_src || !d_frames || !row0 || !rows || n_blocks < 1 || n_blocks > kMaxBlocks || width <= 0 ||
        height <= 0 || n_frames < 1 || n_frames > 65535)
        return CG_E_INVALID;
    if (pix_format != CG_PIX_ARGB8888 && pix_format != CG_PIX_RGB24) return CG_E_INVALID;
    if (frame_stride == 0) frame_stride = (size_t)width * height;
    if (frame_stride < (size_t)width * height) return CG_E_INVALID;
    RtBlocks B{};
    B.n = n_blocks;
    B.W = width;
    B.H = height;
    B.bpp = cg_pix_bytes(pix_format);
    B.wcol0 = col0;
    B.wcols = cols;
    B.cum[0] = 0;
    for (int b = 0; b < n_blocks; ++b) {
        if (rows[b] < 0 || row0[b] < 0) return CG_E_INVALID;
        B.row0[b] = row0[b];
        B.rows[b] = rows[b];
        B.cum[b + 1] = B.cum[b] + rows[b];
    }
    if (B.cum[n_blocks] > 65535) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_rt_assemble((const uint8_t *)d_src, B, n_frames, d_frames, frame_stride,
                                 stream ? (hipStream_t)stream : c->stream), "assemble launch");
    return CG_OK;
}

extern "C" int cg_rt_pack_radiance_device(cg_ctx *c, const float *d_rgba, size_t n_pixels, float scale,
                                          uint32_t *d_argb, void *stream)
{
    if (!c || (n_pixels && (!d_rgba || !d_argb)) || ((uintptr_t)d_rgba & 15) || n_pixels > ((size_t)1 << 39))
        return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_rt_pack_radiance(d_rgba, n_pixels, scale, d_argb, stream ? (hipStream_t)stream : c->stream),
           "pack radiance launch");
    return CG_OK;
}

extern "C" int cg_rt_unstripe_batch_device(cg_ctx *c, const uint32_t *d_gathered, int width, int height,
                                           int nranks, int stripe_h, int nframes, uint32_t *d_frames, void *stream)
{
    if (!c || !d_gathered || !d_frames || width <= 0 || height <= 0 || nranks < 1 || stripe_h <= 0 ||
        nframes < 1 || nframes > 65535)
        return CG_E_INVALID;
    cg_rt_shard s{0, nranks, stripe_h, 0, 0, 0, 0};
    int rows = cg_rt_shard_rows(height, &s);
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_rt_unstripe(d_gathered, width, height, nranks, stripe_h, rows, nframes, d_frames,
                                 stream ? (hipStream_t)stream : c->stream), "unstripe launch");
    return CG_OK;
}

extern "C" int cg_rt_unstripe_device(cg_ctx *c, const uint32_t *d_gathered, int width, int height,
                                     int nranks, int stripe_h, uint32_t *d_frame, void *stream)
{
    return cg_rt_unstripe_batch_device(c, d_gathered, width, height, nranks, stripe_h, 1, d_frame, stream);
}

extern "C" int cg_rt_probe_closest(cg_ctx *c, const cg_vec4 *starts, const cg_vec4 *dirs, int n,
                                   cg_isect *out, int *hit)
{
    if (!c || n < 0 || (n && (!starts || !dirs || !out || !hit))) return CG_E_INVALID;
    if (c->n_tris < 0) return CG_E_NOSCENE;
    if (n == 0) return CG_OK;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, c->probe_a.ensure((size_t)n * sizeof(cg_vec4)), "alloc");
    CG_TRY(c, c->probe_b.ensure((size_t)n * sizeof(cg_vec4)), "alloc");
    CG_TRY(c, c->probe_c.ensure((size_t)n * sizeof(cg_isect)), "alloc");
    CG_TRY(c, c->probe_d.ensure((size_t)n * sizeof(int)), "alloc");
    CG_TRY(c, hipMemcpyAsync(c->probe_a.p, starts, (size_t)n * sizeof(cg_vec4), hipMemcpyHostToDevice, c->stream), "h2d");
    CG_TRY(c, hipMemcpyAsync(c->probe_b.p, dirs, (size_t)n * sizeof(cg_vec4), hipMemcpyHostToDevice, c->stream), "h2d");
    RtFrame F;
    std::memset(&F, 0, sizeof(F));
    F.n_tris = c->n_tris;
    F.n_sph = c->n_sph;
    F.nbound = c->nbound;
    CG_TRY(c, launch_rt_probe_closest(F, (const cg_tri *)c->tris.p, (const RtSphere *)c->sph.p,
                                      (const cg_vec4 *)c->probe_a.p, (const cg_vec4 *)c->probe_b.p, n,
                                      (cg_isect *)c->probe_c.p, (int *)c->probe_d.p, c->stream), "probe");
    CG_TRY(c, hipMemcpyAsync(out, c->probe_c.p, (size_t)n * sizeof(cg_isect), hipMemcpyDeviceToHost, c->stream), "d2h");
    CG_TRY(c, hipMemcpyAsync(hit, c->probe_d.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h");
    CG_TRY(c, hipStreamSynchronize(c->stream), "probe sync");
    return CG_OK;
}

extern "C" int cg_rt_probe_direct_light(cg_ctx *c, const cg_isect *isects, const cg_light *light,
                                        int n, cg_vec3 *out)
{
    if (!c || !light || n < 0 || (n && (!isects || !out))) return CG_E_INVALID;
    if (c->n_tris < 0) return CG_E_NOSCENE;
    if (n == 0) return CG_OK;
    for (int i = 0; i < n; ++i) {
        int ti = isects[i].triangleIndex, si = isects[i].sphereIndex;
        if (ti != -1 ? (ti < 0 || ti >= c->n_tris) : (si < 0 || si >= c->n_sph)) return CG_E_INVALID;
    }
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    RtFrame F;
    std::memset(&F, 0, sizeof(F));
    F.n_tris = c->n_tris;
    F.n_sph = c->n_sph;
    F.nbound = c->nbound;
    int rc = set_lights(c, light, 1, c->stream, F);
    if (rc) return rc;
    // shadow rays use generic starts: RtTri constants are camera-independent
    // except s/detT/K2/K3, which the shadow path does not read.
    RtFrameCams zero{};
    zero.c[0][3] = 1.0f;
    CG_TRY(c, launch_rt_prepare((const cg_tri *)c->tris.p, (const RtGeo *)c->geo.p, c->n_tris, zero, 1,
                                (RtTri *)c->tc.p, c->stream, nullptr, nullptr, nullptr, nullptr), "prepare");
    CG_TRY(c, c->probe_c.ensure((size_t)n * sizeof(cg_isect)), "alloc");
    CG_TRY(c, c->probe_a.ensure((size_t)n * sizeof(cg_vec3) + 16), "alloc");
    CG_TRY(c, hipMemcpyAsync(c->probe_c.p, isects, (size_t)n * sizeof(cg_isect), hipMemcpyHostToDevice, c->stream), "h2d");
    CG_TRY(c, launch_rt_probe_direct_light(F, (const RtTri *)c->tc.p, (const RtShade *)c->shade.p,
                                           (const RtSphere *)c->sph.p, (const cg_isect *)c->probe_c.p,
                                           n, (cg_vec3 *)c->probe_a.p, c->stream), "probe");
    CG_TRY(c, hipMemcpyAsync(out, c->probe_a.p, (size_t)n * sizeof(cg_vec3), hipMemcpyDeviceToHost, c->stream), "d2h");
    CG_TRY(c, hipStreamSynchronize(c->stream), "probe sync");
    return CG_OK;
}
