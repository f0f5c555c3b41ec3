// cg_api_rast.hip -- the rasteriser's entry points: scene, routes, lanes, sequences, textures,
// buffers and picking, the float picture and exposed key scripts.  Host code only (kernels:
// cg_rast*.hip, cg_geometry.hip, cg_hdr.hip).
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "cg_bloom.h"
#include "cg_ctx.h"
#include "cg_hdr.h"

// bit k set: some triangle of the list carries texture k (1-3)
static int rast_tex_mask(const cg_rtri *t, int n)
{
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (t[i].color.x >= 0 && t[i].texture != 0)
            m |= (t[i].texture >= 1 && t[i].texture <= 3) ? 1 << t[i].texture : 1 << 4;   // 16: no such texture
    return m;
}

extern "C" int cg_rast_render_device(cg_ctx *c, const cg_rtri *d_tris, int n,
                                     const cg_rast_params *p, cg_vec4 light, uint32_t *d_argb,
                                     float *d_depth, int32_t *d_shadow, void *stream)
{
    if (!c || !p || !d_argb || n < 0 || (n && !d_tris)) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    // device lists are not inspected: textures run if any maps are loaded
    return rast_render_device(c, d_tris, n, p, light, d_argb, d_depth, d_shadow,
                              stream ? (hipStream_t)stream : c->stream, nullptr, c->tex_loaded);
}

extern "C" int cg_rast_render(cg_ctx *c, const cg_rtri *tris, int n, const cg_rast_params *p,
                              cg_vec4 light, uint32_t *argb, float *depth, int32_t *shadow,
                              cg_stats *stats)
{
    if (!c || !p || !argb || n < 0 || (n && !tris) || p->width <= 2 || p->height <= 2 ||
        p->height > kRastMaxH)
        return CG_E_INVALID;
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    size_t npx = (size_t)p->width * p->height;
    hipError_t e;
    cg_rtri *d_tris = (cg_rtri *)ctx_buf(c, kBufTris, (size_t)(n > 0 ? n : 1) * sizeof(cg_rtri), &e);
    if (!d_tris) return ctx_fail(c, e, "alloc rast tris");
    uint32_t *d_argb = (uint32_t *)ctx_buf(c, kBufArgb, npx * 4, &e);
    if (!d_argb) return ctx_fail(c, e, "alloc argb");
    float *d_depth = (float *)ctx_buf(c, kBufDepth, npx * 4, &e);
    if (!d_depth) return ctx_fail(c, e, "alloc depth");
    int32_t *d_shadow = (int32_t *)ctx_buf(c, kBufShadow, npx * 4, &e);
    if (!d_shadow) return ctx_fail(c, e, "alloc shadow");
    if (n) CG_TRY(c, hipMemcpyAsync(d_tris, tris, (size_t)n * sizeof(cg_rtri), hipMemcpyHostToDevice, c->stream), "upload tris");
    int rc = rast_render_device(c, d_tris, n, p, light, d_argb, d_depth, d_shadow, c->stream, stats,
                                rast_tex_mask(tris, n));
    if (rc) return rc;
    CG_TRY(c, hipMemcpyAsync(argb, d_argb, npx * 4, hipMemcpyDeviceToHost, c->stream), "d2h argb");
    if (depth) CG_TRY(c, hipMemcpyAsync(depth, d_depth, npx * 4, hipMemcpyDeviceToHost, c->stream), "d2h depth");
    if (shadow) CG_TRY(c, hipMemcpyAsync(shadow, d_shadow, npx * 4, hipMemcpyDeviceToHost, c->stream), "d2h shadow");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rast frame");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = n;
    }
    return CG_OK;
}

extern "C" int cg_rast_set_scene(cg_ctx *c, const cg_rtri *room, int n_room, const cg_rtri *boxes, int n_boxes)
{
    if (!c || n_room < 0 || n_boxes < 0 || (n_room && !room) || (n_boxes && !boxes)) return CG_E_INVALID;
    if ((long long)n_room + 7ll * n_boxes > kRastMaxInputs)
        return ctx_invalid(c, "cg_rast_set_scene: more than 4194304 input triangles (n_room + 7 * n_boxes)");
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, c->rroom.ensure((size_t)(n_room > 0 ? n_room : 1) * sizeof(cg_rtri)), "alloc room");
    CG_TRY(c, c->rboxes.ensure((size_t)(n_boxes > 0 ? n_boxes : 1) * sizeof(cg_rtri)), "alloc boxes");
    if (n_room)
        CG_TRY(c, hipMemcpyAsync(c->rroom.p, room, (size_t)n_room * sizeof(cg_rtri), hipMemcpyHostToDevice, c->stream), "upload room");
    if (n_boxes)
        CG_TRY(c, hipMemcpyAsync(c->rboxes.p, boxes, (size_t)n_boxes * sizeof(cg_rtri), hipMemcpyHostToDevice, c->stream), "upload boxes");
    CG_TRY(c, hipStreamSynchronize(c->stream), "scene upload");
    c->n_room = n_room;
    c->n_boxes = n_boxes;
    c->scene_tex = rast_tex_mask(room, n_room) | rast_tex_mask(boxes, n_boxes);
    ++c->scene_gen;
    return CG_OK;
}

extern "C" int cg_rast_route(long long list_capacity)
{
    return list_capacity <= kRastDenseList ? CG_RAST_ROUTE_DENSE : CG_RAST_ROUTE_COMPACT;
}

extern "C" int cg_rast_set_route(cg_ctx *c, int route)
{
    if (!c) return CG_E_INVALID;
    if (route < -1 || route > CG_RAST_ROUTE_COMPACT) return ctx_invalid(c, "cg_rast_set_route: -1, 0 or 1");
    c->rast_route = route;
    return CG_OK;
}

extern "C" int cg_rast_set_route_limit(cg_ctx *c, long long list_capacity)
{
    if (!c) return CG_E_INVALID;
    if (list_capacity < 0) return ctx_invalid(c, "cg_rast_set_route_limit: a list capacity, or 0 for the default");
    c->route_limit = list_capacity;
    return CG_OK;
}

extern "C" int cg_rast_span_segments(int lx, int rx, int width, int *first)
{
    int f = 0;
    const int k = rast_span_segments(lx, rx, width, &f);
    if (first) *first = f;
    return k;
}

extern "C" int cg_rast_row_blocks(int *batch, int *chunk)
{
    if (!batch || !chunk) return CG_E_INVALID;
    rast_big_blocks(batch, chunk);
    return CG_OK;
}

extern "C" int cg_rast_scratch_info(cg_ctx *c, uint64_t out[5])
{
    if (!c || !out) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const RastLast &L = c->rlast;
    if (L.route >= 0) CG_TRY(c, hipStreamSynchronize(L.st ? L.st : c->stream), "rast frame");
    auto held = [](const cg_ctx *x) {
        size_t b = x->rtris.bytes + x->rhdr.bytes + x->rspan.bytes + x->rpix.bytes + x->rcount.bytes + x->rrecs.bytes +
                   x->rgeo.bytes + x->rhdr_rgba.bytes;
        for (const DevBuf &d : x->rbig) b += d.bytes;
        b += x->rbuf[kBufOwner - kBufOwner].bytes + x->rbuf[kBufClipPre - kBufOwner].bytes;   // a buffers call's scratch
        return b;
    };
    out[0] = held(c);
    for (const auto &l : c->lanes)
        if (l) out[0] += held(l.get());
    out[1] = out[2] = out[3] = out[4] = 0;
    if (L.route < 0) return CG_OK;
    out[1] = (uint64_t)L.route;
    long long n = L.n, recs = L.recs;
    if (n < 0 && L.n_dev) {
        int v = 0;
        CG_TRY(c, hipMemcpy(&v, L.n_dev, sizeof(int), hipMemcpyDeviceToHost), "d2h count");
        n = v;
    }
    if (recs < 0 && L.count && L.H > 0) {
        std::vector<int> cnt((size_t)L.H);
        CG_TRY(c, hipMemcpy(cnt.data(), L.count, cnt.size() * sizeof(int), hipMemcpyDeviceToHost), "d2h counts");
        recs = 0;
        for (int v : cnt) recs += v;
    }
    out[2] = (uint64_t)std::max(n, 0ll);
    out[3] = (uint64_t)L.spans;
    out[4] = (uint64_t)std::max(recs, 0ll);
    return CG_OK;
}

static int rast_lanes_ready(cg_ctx *c, int L);

extern "C" int cg_rast_draw_frames_device(cg_ctx *c, const cg_rast_params *ps, int n_frames, uint32_t *d_argb,
                                          float *d_depth, int32_t *d_shadow, size_t frame_stride, void *stream)
{
    if (!c || n_frames < 0 || (n_frames && (!ps || !d_argb))) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    if (n_frames == 0) return CG_OK;
    const size_t px = (size_t)ps[0].width * ps[0].height;
    const size_t stride = frame_stride ? frame_stride : px;
    for (int f = 0; f < n_frames; ++f)
        if (ps[f].colour_mode != 0 || ps[f].width != ps[0].width || ps[f].height != ps[0].height || stride < px)
            return ctx_invalid(c, "draw_frames: colour mode 0 frames of one size (modes 1-2 chain rand offsets)");
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (ctx_rast_route(c, kGeomMaxLeaves * ((long long)c->n_room + 7ll * c->n_boxes), false) == CG_RAST_ROUTE_COMPACT) {
        // compact-route frames follow each other on `stream`: a lane would hold its own copy of the scratch
        for (int f = 0; f < n_frames; ++f) {
            const size_t o = (size_t)f * stride;
            const int rc = rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p,
                                            c->n_boxes, &ps[f], d_argb + o, d_depth ? d_depth + o : nullptr,
                                            d_shadow ? d_shadow + o : nullptr, st, nullptr, nullptr, c->scene_tex);
            if (rc) return rc;
        }
        return CG_OK;
    }
    // lanes in flight (CG_RAST_LANES for A/B runs): 6 -- C3 1080p, 64 frames per call, round 6:
    // 2 lanes 21.3-21.4k frames/s, 3 18.0k, 4 21.2k, 5 22.6-22.7k, 6 23.1-23.3k, 7 20.7-20.9k,
    // 8 21.3-22.4k (profiles/r06_ab_session2.json; round 1 had found 2 best).  The lanes' streams
    // share the process's 4 hardware queues, so the count sets how the frames' latency-bound
    // kernels interleave; 6 was best both alone and inside the default bench line
    static const int lanes = [] {
        const char *e = std::getenv("CG_RAST_LANES");
        const int v = e ? std::atoi(e) : 6;
        return std::max(1, std::min(v, (int)cg_ctx::kRastLanes));
    }();
    const int L = std::min(lanes, n_frames);
    const int rc_lanes = rast_lanes_ready(c, L);
    if (rc_lanes) return rc_lanes;
    CG_TRY(c, hipEventRecord(c->start_ev, st), "event");
    for (int k = 0; k < L; ++k) CG_TRY(c, hipStreamWaitEvent(c->lanes[k]->stream, c->start_ev, 0), "lane wait");
    for (int f = 0; f < n_frames; ++f) {
        cg_ctx *l = c->lanes[f % L].get();
        const size_t o = (size_t)f * stride;
        int rc = rast_draw_device(l, (const cg_rtri *)l->rroom.p, l->n_room, (const cg_rtri *)l->rboxes.p, l->n_boxes,
                                  &ps[f], d_argb + o, d_depth ? d_depth + o : nullptr, d_shadow ? d_shadow + o : nullptr,
                                  l->stream, nullptr, nullptr, l->scene_tex);
        if (rc) {
            c->err = std::string("lane: ") + l->err;
            return rc;
        }
    }
    for (int k = 0; k < L; ++k) {
        CG_TRY(c, hipEventRecord(c->lane_ev[k], c->lanes[k]->stream), "event");
        CG_TRY(c, hipStreamWaitEvent(st, c->lane_ev[k], 0), "lane join");
    }
    c->rlast = c->lanes[(n_frames - 1) % L]->rlast;   // the latest frame's counts live in its lane
    c->rlast.st = st;
    return CG_OK;
}

// The first L lane contexts with the parent's scene (created on first use; the scene is copied
// device to device when it changed, which waits).
static int rast_lanes_ready(cg_ctx *c, int L)
{
    CG_TRY(c, c->start_ev.ensure(), "event");
    for (int k = 0; k < L; ++k) {
        if (!c->lanes[k]) {
            cg_ctx *lane = nullptr;
            int rc = cg_create(c->device, &lane);
            if (rc) return ctx_invalid(c, "lane context");
            c->lanes[k].reset(lane);
            lane->tex_owner = c;
            CG_TRY(c, c->lane_ev[k].ensure(), "event");
            c->lane_gen[k] = c->scene_gen - 1;
        }
        cg_ctx *l = c->lanes[k].get();
        l->rast_route = c->rast_route;          // the lanes follow their parent
        l->route_limit = c->route_limit;
        if (c->lane_gen[k] != c->scene_gen) {   // the parent's scene, device to device
            CG_TRY(c, l->rroom.ensure(c->rroom.bytes), "alloc lane room");
            CG_TRY(c, l->rboxes.ensure(c->rboxes.bytes), "alloc lane boxes");
            CG_TRY(c, hipMemcpyAsync(l->rroom.p, c->rroom.p, c->rroom.bytes, hipMemcpyDeviceToDevice, c->stream),
                   "lane scene");
            CG_TRY(c, hipMemcpyAsync(l->rboxes.p, c->rboxes.p, c->rboxes.bytes, hipMemcpyDeviceToDevice, c->stream),
                   "lane scene");
            CG_TRY(c, hipStreamSynchronize(c->stream), "lane scene");
            l->n_room = c->n_room;
            l->n_boxes = c->n_boxes;
            l->scene_tex = c->scene_tex;
            c->lane_gen[k] = c->scene_gen;
        }
    }
    return CG_OK;
}

// Largest generator the tables are built for (chunks of 992 values; 31 words each).
static constexpr long long kRastSeqMaxChunks = 1ll << 22;

extern "C" int cg_rast_set_rand_capacity(cg_ctx *c, long long fragments)
{
    if (!c || fragments < 0 || fragments > (1ll << 40) || rast_rand_chunks(3 * fragments) > kRastSeqMaxChunks)
        return CG_E_INVALID;
    c->rand_cap = fragments;
    return CG_OK;
}

static int rast_sequence_device(cg_ctx *c, const cg_rast_params *ps, int n_frames, uint32_t *d_argb, float *d_depth,
                                int32_t *d_shadow, size_t frame_stride, cg_rast_seq_frame *d_info, void *stream,
                                bool resume, int lane_cap, int pix = CG_PIX_ARGB8888);

extern "C" int cg_rast_draw_sequence_device(cg_ctx *c, const cg_rast_params *ps, int n_frames, uint32_t *d_argb,
                                            float *d_depth, int32_t *d_shadow, size_t frame_stride,
                                            cg_rast_seq_frame *d_info, void *stream)
{
    return rast_sequence_device(c, ps, n_frames, d_argb, d_depth, d_shadow, frame_stride, d_info, stream, false, 0);
}

// cg_rast_draw_sequence_device, and a chunk of cg_rast_draw_sequence.  resume: the first frame
// starts at the index an earlier call on the same stream left in d_info[0] (its closing record),
// as every later frame does; ps[0].rand_offset is then ignored too.  lane_cap > 0: at most so
// many lanes.  pix: d_argb's pixel format (CG_PIX_RGBA_F32: float4 pixels, frame_stride in those).
static int rast_sequence_device(cg_ctx *c, const cg_rast_params *ps, int n_frames, uint32_t *d_argb, float *d_depth,
                                int32_t *d_shadow, size_t frame_stride, cg_rast_seq_frame *d_info, void *stream,
                                bool resume, int lane_cap, int pix)
{
    if (!c || n_frames < 0 || (n_frames && (!ps || !d_argb))) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    if (n_frames == 0) return CG_OK;
    if (!d_info) return ctx_invalid(c, "draw_sequence: d_info is required");
    if (ps[0].width <= 2 || ps[0].height <= 2) return ctx_invalid(c, "draw_sequence: frame size");
    const size_t px = (size_t)ps[0].width * ps[0].height;
    const size_t stride = frame_stride ? frame_stride : px;
    bool colour = false;
    for (int f = 0; f < n_frames; ++f) {
        if (ps[f].colour_mode < 0 || ps[f].colour_mode > 2 || ps[f].width != ps[0].width ||
            ps[f].height != ps[0].height || stride < px)
            return ctx_invalid(c, "draw_sequence: colour modes 0-2, frames of one size, frame_stride >= W * H");
        colour = colour || ps[f].colour_mode != 0;
    }
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    RastSeq q{};
    q.start = ps[0].rand_offset;
    q.cap = c->rand_cap > 0 ? c->rand_cap : 4 * (long long)px;
    const long long nb = rast_rand_chunks(3 * q.cap);
    if (nb > kRastSeqMaxChunks) return ctx_invalid(c, "draw_sequence: rand() stream capacity");
    q.nb_cap = (int)nb;
    // Lanes (CG_RAST_SEQ_LANES for A/B runs): a frame's front end up to its fragment count does
    // not depend on the call index, so the frames run round-robin on the context's lane streams
    // and only their chain steps follow each other (events): frame f + 1's front end runs beside
    // frame f's seek, generator, fill and post.  1: every frame on `stream` itself.  6 -- 1080p
    // colour mode 1, 64 frames per call (scripts/rast_sequence_rate.py, two runs each): 1 lane
    // 2.75k frames/s, 2 3.5-4.0k, 3 3.3-3.4k, 4 3.8k, 5 4.3-4.4k, 6 4.75-4.80k, 7 4.4k, 8 4.5-4.6k.
    static const int lanes = [] {
        const char *e = std::getenv("CG_RAST_SEQ_LANES");
        const int v = e ? std::atoi(e) : 6;
        return std::max(1, std::min(v, (int)cg_ctx::kRastLanes));
    }();
    // compact-route frames follow each other on `stream` (a lane would hold its own copy of the scratch)
    q.route = ctx_rast_route(c, kGeomMaxLeaves * ((long long)c->n_room + 7ll * c->n_boxes), colour);
    const bool compact = q.route == CG_RAST_ROUTE_COMPACT;
    const int L = compact ? 1 : std::min(lane_cap > 0 ? std::min(lanes, lane_cap) : lanes, n_frames);
    if (L > 1) {
        const int rc = rast_lanes_ready(c, L);
        if (rc) return rc;
    }
    // (the compact route sizes each frame's stream by the frame's own count: no tables, no capacity)
    if (colour && !compact) {
        const int rc = rast_seq_tables(c, nb, &c->rseq_chunks, &q.tables);
        if (rc) return rc;
    }
    uint32_t *win[cg_ctx::kRastLanes] = {};
    for (int k = 0; k < L; ++k) {
        cg_ctx *l = L > 1 ? c->lanes[k].get() : c;
        hipError_t e;
        if (L > 1) {
            CG_TRY(c, c->seq_ev[k].ensure(), "event");
            if (!(win[k] = (uint32_t *)ctx_buf(l, kBufSeq, 64 * sizeof(uint32_t), &e))) return ctx_fail(c, e, "alloc window");
        }
        if (!colour || compact) continue;
        // everything a colour frame sizes differently from a mode 0 frame, before the first
        // launch: the frames then find every buffer in place (a buffer that grows waits)
        if (!ctx_buf(l, kBufPix, px * sizeof(float4), &e)) return ctx_fail(c, e, "alloc state");
        if (!d_shadow && !ctx_buf(l, kBufShadow, px * sizeof(int32_t), &e)) return ctx_fail(c, e, "alloc shadow");
        if (!ctx_buf(l, kBufRnd, 3 * (size_t)q.cap * sizeof(int32_t), &e)) return ctx_fail(c, e, "alloc rand stream");
    }
    if (L > 1) {
        CG_TRY(c, hipEventRecord(c->start_ev, st), "event");
        for (int k = 0; k < L; ++k) CG_TRY(c, hipStreamWaitEvent(c->lanes[k]->stream, c->start_ev, 0), "lane wait");
    }
    const size_t wpp = pix == CG_PIX_RGBA_F32 ? 4 : 1;   // 4-byte words a pixel of d_argb takes
    for (int f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * stride;
        cg_ctx *l = L > 1 ? c->lanes[f % L].get() : c;
        q.info = d_info + f;
        q.first = f == 0 && !resume;
        q.win = win[f % L];
        q.wait_ev = L > 1 && f > 0 ? c->seq_ev[(f - 1) % L] : nullptr;
        q.done_ev = L > 1 ? c->seq_ev[f % L] : nullptr;
        const int rc = rast_draw_device(l, (const cg_rtri *)l->rroom.p, l->n_room, (const cg_rtri *)l->rboxes.p,
                                        l->n_boxes, &ps[f], d_argb + o * wpp, d_depth ? d_depth + o : nullptr,
                                        d_shadow ? d_shadow + o : nullptr, L > 1 ? l->stream : st, nullptr, nullptr,
                                        l->scene_tex, &q, pix);
        if (rc) {
            if (l != c) c->err = std::string("lane: ") + l->err;
            return rc;
        }
    }
    for (int k = 0; L > 1 && k < L; ++k) {
        CG_TRY(c, hipEventRecord(c->lane_ev[k], c->lanes[k]->stream), "event");
        CG_TRY(c, hipStreamWaitEvent(st, c->lane_ev[k], 0), "lane join");
    }
    if (L > 1) {
        c->rlast = c->lanes[(n_frames - 1) % L]->rlast;
        c->rlast.st = st;
    }
    return CG_OK;
}

extern "C" int cg_glibc_rand_device(cg_ctx *c, const uint64_t *d_offset, int n, int32_t *d_out, void *stream)
{
    if (!c || n < 0 || (n && (!d_offset || !d_out))) return CG_E_INVALID;
    if (n == 0) return CG_OK;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const long long nb = rast_rand_chunks(n);
    uint32_t *tables = nullptr;
    const int rc = rast_seq_tables(c, nb, &c->rseq_chunks, &tables);
    if (rc) return rc;
    return rast_rand_probe(c, tables, (int)nb, d_offset, n, d_out, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int cg_rast_opacity_map(const uint8_t *bgr, int n, uint8_t *out)
{
    if (n < 0 || (n && (!bgr || !out))) return CG_E_INVALID;
    for (int i = 0; i < n; ++i) {   // RGB2Gray<uchar> (blueIdx 0), then threshold(100, 255, BINARY)
        const int y = (bgr[3 * i] * 1868 + bgr[3 * i + 1] * 9617 + bgr[3 * i + 2] * 4899 + (1 << 13)) >> 14;
        out[i] = y > 100 ? 255 : 0;
    }
    return CG_OK;
}

extern "C" int cg_rast_set_textures(cg_ctx *c, const cg_rast_textures *t)
{
    if (!c) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, hipStreamSynchronize(c->stream), "sync");
    DevBuf *all[] = {&c->tmarble, &c->tnoise, &c->twoven, &c->twoven_ao, &c->twoven_op, &c->twoven_nrm,
                     &c->tgrill, &c->tgrill_op, &c->tgrill_nrm};
    for (DevBuf *b : all) b->release();
    c->tex_loaded = 0;
    if (!t) return CG_OK;
    const size_t tn = (size_t)kTexN * kTexN, mn = (size_t)kMarbleN * kMarbleN;
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        CG_TRY(c, b.ensure(bytes), "alloc texture");
        CG_TRY(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice), "upload texture");
        return CG_OK;
    };
    auto up_op = [&](DevBuf &b, const uint8_t *bgr) -> int {   // skeleton.cpp:149-155
        std::vector<uint8_t> op(tn);
        cg_rast_opacity_map(bgr, (int)tn, op.data());
        return up(b, op.data(), tn);
    };
    int rc = 0;
    if (t->grill && t->grill_opacity && t->grill_normal) {
        if ((rc = up(c->tgrill, t->grill, 3 * tn)) || (rc = up_op(c->tgrill_op, t->grill_opacity)) ||
            (rc = up(c->tgrill_nrm, t->grill_normal, 3 * tn)))
            return rc;
        c->tex_loaded |= 1 << 2;
    }
    if (t->woven && t->woven_ao && t->woven_opacity && t->woven_normal) {
        if ((rc = up(c->twoven, t->woven, 3 * tn)) || (rc = up(c->twoven_ao, t->woven_ao, 3 * tn)) ||
            (rc = up_op(c->twoven_op, t->woven_opacity)) || (rc = up(c->twoven_nrm, t->woven_normal, 3 * tn)))
            return rc;
        c->tex_loaded |= 1 << 3;
    }
    if (t->marble) {
        // normalMap_marble (:158-170): the process's first 3 * 2000 * 2000 rand() calls
        std::vector<int32_t> r(3 * mn);
        if ((rc = cg_glibc_rand(0, (int)r.size(), r.data()))) return rc;
        std::vector<float> noise(3 * mn);
        const float LO = -0.000002f, HI = 0.000002f;
        for (size_t i = 0; i < r.size(); ++i) noise[i] = LO + (float)r[i] / ((float)((float)RAND_MAX / HI - LO));
        if ((rc = up(c->tmarble, t->marble, 3 * mn)) || (rc = up(c->tnoise, noise.data(), noise.size() * 4))) return rc;
        c->tex_loaded |= 1 << 1;
    }
    return CG_OK;
}

extern "C" int cg_rast_draw_device(cg_ctx *c, const cg_rast_params *p, uint32_t *d_argb, float *d_depth,
                                   int32_t *d_shadow, void *stream)
{
    if (!c || !p || !d_argb) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    return rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p, c->n_boxes, p,
                            d_argb, d_depth, d_shadow, stream ? (hipStream_t)stream : c->stream, nullptr, nullptr,
                            c->scene_tex);
}

extern "C" int cg_rast_draw(cg_ctx *c, const cg_rast_params *p, uint32_t *argb, float *depth, int32_t *shadow,
                            cg_stats *stats)
{
    if (!c || !p || !argb || p->width <= 2 || p->height <= 2) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    size_t npx = (size_t)p->width * p->height;
    hipError_t e;
    uint32_t *d_argb = (uint32_t *)ctx_buf(c, kBufArgb, npx * 4, &e);
    if (!d_argb) return ctx_fail(c, e, "alloc argb");
    float *d_depth = (float *)ctx_buf(c, kBufDepth, npx * 4, &e);
    if (!d_depth) return ctx_fail(c, e, "alloc depth");
    int32_t *d_shadow = (int32_t *)ctx_buf(c, kBufShadow, npx * 4, &e);
    if (!d_shadow) return ctx_fail(c, e, "alloc shadow");
    int *d_n = nullptr;
    int rc = rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p, c->n_boxes, p,
                              d_argb, d_depth, d_shadow, c->stream, stats, &d_n, c->scene_tex);
    if (rc) return rc;
    int n = 0;
    CG_TRY(c, hipMemcpyAsync(&n, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h count");
    CG_TRY(c, hipMemcpyAsync(argb, d_argb, npx * 4, hipMemcpyDeviceToHost, c->stream), "d2h argb");
    if (depth) CG_TRY(c, hipMemcpyAsync(depth, d_depth, npx * 4, hipMemcpyDeviceToHost, c->stream), "d2h depth");
    if (shadow) CG_TRY(c, hipMemcpyAsync(shadow, d_shadow, npx * 4, hipMemcpyDeviceToHost, c->stream), "d2h shadow");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rast frame");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = n;
    }
    return CG_OK;
}

// ---- HDR shade buffers, owner ids, picking (kernels in cg_rast_buffers.hip) ----
static bool rast_buffers_any(const cg_rast_buffers *b)
{
    return b && (b->argb || b->depth || b->shadow || b->screen || b->low || b->high || b->clip || b->tri || b->pos);
}

// The frame of cg_rast_draw_device (tris == nullptr) or cg_rast_render_device, told to leave
// the owner's state words in every colour mode, then the buffers kernel.
static int rast_buffers_frame(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p, cg_vec4 light,
                              const cg_rast_buffers *d, hipStream_t st, cg_stats *stats, int **n_out, int tex_mask)
{
    c->rast_want_owner = true;
    c->rframe.valid = false;
    const int rc = d_tris || n >= 0
                       ? rast_render_device(c, d_tris, n, p, light, d->argb, d->depth, d->shadow, st, stats, tex_mask)
                       : rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p,
                                          c->n_boxes, p, d->argb, d->depth, d->shadow, st, stats, n_out, tex_mask);
    c->rast_want_owner = false;
    if (rc) return rc;
    return rast_buffers_device(c, d, n >= 0 ? -1 : c->n_room, st);
}

extern "C" int cg_rast_draw_buffers_device(cg_ctx *c, const cg_rast_params *p, const cg_rast_buffers *d, void *stream)
{
    if (!c || !p || !rast_buffers_any(d)) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    return rast_buffers_frame(c, nullptr, -1, p, cg_vec4{0, 0, 0, 1}, d, stream ? (hipStream_t)stream : c->stream, nullptr,
                              nullptr, c->scene_tex);
}

extern "C" int cg_rast_render_buffers_device(cg_ctx *c, const cg_rtri *d_tris, int n, const cg_rast_params *p,
                                             cg_vec4 light, const cg_rast_buffers *d, void *stream)
{
    if (!c || !p || !rast_buffers_any(d) || n < 0 || (n && !d_tris)) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    // device lists are not inspected: textures run if any maps are loaded
    return rast_buffers_frame(c, d_tris, n, p, light, d, stream ? (hipStream_t)stream : c->stream, nullptr, nullptr,
                              c->tex_loaded);
}

// Host planes: device planes for those asked for, the frame, the downloads.  tris == nullptr
// with n < 0: the context's scene (cg_rast_draw_buffers).
static int rast_buffers_host(cg_ctx *c, const cg_rtri *tris, int n, const cg_rast_params *p, cg_vec4 light,
                             const cg_rast_buffers *h, cg_stats *stats)
{
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t npx = (size_t)p->width * p->height;
    hipError_t e;
    cg_rast_buffers d = {};
    struct Plane { void *host; void **dev; int slot; size_t bytes; };
    const Plane planes[] = {
        {h->argb, (void **)&d.argb, kBufArgb, npx * 4},   {h->depth, (void **)&d.depth, kBufDepth, npx * 4},
        {h->shadow, (void **)&d.shadow, kBufShadow, npx * 4}, {h->screen, (void **)&d.screen, kBufScreen, npx * 12},
        {h->low, (void **)&d.low, kBufLow, npx * 12},     {h->high, (void **)&d.high, kBufHigh, npx * 12},
        {h->clip, (void **)&d.clip, kBufClipId, npx * 4}, {h->tri, (void **)&d.tri, kBufTriId, npx * 4},
        {h->pos, (void **)&d.pos, kBufPos, npx * 16},
    };
    for (const Plane &pl : planes)
        if (pl.host && !(*pl.dev = ctx_buf(c, pl.slot, pl.bytes, &e))) return ctx_fail(c, e, "alloc buffers plane");
    cg_rtri *d_tris = nullptr;
    if (n >= 0) {
        d_tris = (cg_rtri *)ctx_buf(c, kBufTris, (size_t)(n > 0 ? n : 1) * sizeof(cg_rtri), &e);
        if (!d_tris) return ctx_fail(c, e, "alloc rast tris");
        if (n) CG_TRY(c, hipMemcpyAsync(d_tris, tris, (size_t)n * sizeof(cg_rtri), hipMemcpyHostToDevice, c->stream), "upload tris");
    }
    int *d_n = nullptr;
    const int rc = rast_buffers_frame(c, d_tris, n, p, light, &d, c->stream, stats, &d_n,
                                      n >= 0 ? rast_tex_mask(tris, n) : c->scene_tex);
    if (rc) return rc;
    int nt = n;
    if (n < 0) CG_TRY(c, hipMemcpyAsync(&nt, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h count");
    for (const Plane &pl : planes)
        if (pl.host) CG_TRY(c, hipMemcpyAsync(pl.host, *pl.dev, pl.bytes, hipMemcpyDeviceToHost, c->stream), "d2h plane");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rast frame");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = nt;
    }
    return CG_OK;
}

extern "C" int cg_rast_draw_buffers(cg_ctx *c, const cg_rast_params *p, const cg_rast_buffers *h, cg_stats *stats)
{
    if (!c || !p || !rast_buffers_any(h) || p->width <= 2 || p->height <= 2) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    return rast_buffers_host(c, nullptr, -1, p, cg_vec4{0, 0, 0, 1}, h, stats);
}

extern "C" int cg_rast_render_buffers(cg_ctx *c, const cg_rtri *tris, int n, const cg_rast_params *p, cg_vec4 light,
                                      const cg_rast_buffers *h, cg_stats *stats)
{
    if (!c || !p || !rast_buffers_any(h) || n < 0 || (n && !tris) || p->width <= 2 || p->height <= 2 ||
        p->height > kRastMaxH)
        return CG_E_INVALID;
    return rast_buffers_host(c, tris, n, p, light, h, stats);
}

extern "C" int cg_rast_pick(cg_ctx *c, const cg_rast_params *p, int x, int y, int32_t *tri, int32_t *clip, cg_vec4 *pos,
                            int *hit)
{
    if (!c || !p || !hit) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    if (x < 0 || y < 0 || x >= p->width || y >= p->height) return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    // Setup, row records and the ordered z-buffer's fill, nothing else: no picture, no depth or
    // shadow plane.  Colour modes 1-2 never look at textures (:604), so their owner is what the
    // mode-0 walk over the untextured list decides, without a rand() stream.
    cg_rast_params q = *p;
    int tex = c->scene_tex;
    if (q.colour_mode != 0) {
        q.colour_mode = 0;
        tex = 0;
    }
    const cg_rast_buffers none = {};
    c->rast_want_owner = true;
    c->rframe.valid = false;
    const int rc = rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p, c->n_boxes,
                                    &q, none.argb, none.depth, none.shadow, c->stream, nullptr, nullptr, tex);
    c->rast_want_owner = false;
    if (rc) return rc;
    int out[8] = {};
    if (const int rc2 = rast_pick_device(c, c->n_room, x, y, c->stream, out)) return rc2;
    *hit = out[0];
    if (clip) *clip = out[1];
    if (tri) *tri = out[2];
    if (pos) std::memcpy(pos, out + 4, sizeof(cg_vec4));
    return CG_OK;
}

extern "C" int cg_rast_state_bytes(cg_ctx *c) { return c ? rast_frame_state_bytes(c) : CG_E_INVALID; }

// The latest frame's counts on the host (what cg_rast_scratch_info would read), so that they
// outlive other frames run through the same scratch.
static int rast_last_resolve(cg_ctx *c)
{
    RastLast &L = c->rlast;
    if (L.route < 0) return CG_OK;
    CG_TRY(c, hipStreamSynchronize(L.st ? L.st : c->stream), "rast frame");
    if (L.n < 0 && L.n_dev) {
        int v = 0;
        CG_TRY(c, hipMemcpy(&v, L.n_dev, sizeof(int), hipMemcpyDeviceToHost), "d2h count");
        L.n = v;
    }
    if (L.recs < 0 && L.count && L.H > 0) {
        std::vector<int> cnt((size_t)L.H);
        CG_TRY(c, hipMemcpy(cnt.data(), L.count, cnt.size() * sizeof(int), hipMemcpyDeviceToHost), "d2h counts");
        L.recs = 0;
        for (int v : cnt) L.recs += v;
    }
    L.n_dev = L.count = nullptr;
    return CG_OK;
}

// n_frames frames into host memory: chunks of `chunk` frames render through the device sequence
// into two sets of device slots; each chunk's download runs on `xfer` while the next chunk renders
// (rt_render_frames_host's scheme: chunk j's download is issued after chunk j + 1's render is
// enqueued).  The call's records are one device array: chunk j + 1 resumes at the record chunk j
// closed, so the rand() call index never visits the host between chunks.
extern "C" int cg_rast_draw_sequence(cg_ctx *c, const cg_rast_params *ps, int n_frames, uint32_t *argb, float *depth,
                                     int32_t *shadow, size_t frame_stride, int chunk, cg_rast_seq_frame *info,
                                     cg_stats *stats)
{
    if (!c || n_frames < 0 || (n_frames && (!ps || !argb))) return CG_E_INVALID;
    if (chunk < 0 || chunk > 64) return ctx_invalid(c, "draw_sequence: chunk 0 .. 64");
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    if (n_frames == 0) return CG_OK;
    if (ps[0].width <= 2 || ps[0].height <= 2) return ctx_invalid(c, "draw_sequence: frame size");
    const size_t px = (size_t)ps[0].width * ps[0].height;
    const size_t stride = frame_stride ? frame_stride : px;
    for (int f = 0; f < n_frames; ++f)
        if (ps[f].colour_mode < 0 || ps[f].colour_mode > 2 || ps[f].width != ps[0].width ||
            ps[f].height != ps[0].height || stride < px)
            return ctx_invalid(c, "draw_sequence: colour modes 0-2, frames of one size, frame_stride >= W * H");
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const int ch = std::min(chunk ? chunk : 8, n_frames);
    // Lanes of a chunk's render (CG_RAST_HOST_LANES for A/B runs): 2.  The process's streams share
    // its 4 hardware queues, so with the device form's 6 lanes the transfer stream's copy sits in
    // a queue behind a lane's kernels of the next chunk, which wait for the previous download:
    // the link idles for a chunk's render time per chunk.  1080p, 64 frames a call into pinned
    // memory, mode 0: 1 lane 6.26k frames/s, 2 6.35k, 3 6.29k, 4 6.27k, 6 5.0k (a third slot set
    // 5.8k, 16 hardware queues 5.5k); mode 1: 2 lanes 3.6k, 3 3.2k, 4 3.4k, 6 3.15k.
    static const int host_lanes = [] {
        const char *e = std::getenv("CG_RAST_HOST_LANES");
        return std::max(1, std::min(e ? std::atoi(e) : 2, (int)cg_ctx::kRastLanes));
    }();
    constexpr int NS = cg_ctx::kRastHostSlots;
    CG_TRY(c, c->xfer.ensure(hipStreamNonBlocking), "copy stream");
    for (int k = 0; k < 2; ++k) {
        CG_TRY(c, c->ev_rdone[k].ensure(), "copy event");
        CG_TRY(c, c->ev_cdone[k].ensure(), "copy event");
    }
    for (int k = 0; k < NS; ++k) {
        CG_TRY(c, c->rs_rdone[k].ensure(), "copy event");
        CG_TRY(c, c->rs_cdone[k].ensure(), "copy event");
    }
    // Every return below, error or not, leaves nothing of this call running (rt_render_frames_host).
    struct Drain {
        cg_ctx *c;
        ~Drain()
        {
            (void)hipStreamSynchronize(c->xfer);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain_on_exit{c};
    for (int k = 0; k < NS; ++k) {
        CG_TRY(c, c->rs_argb[k].ensure((size_t)ch * px * sizeof(uint32_t)), "alloc frame slots");
        if (depth) CG_TRY(c, c->rs_depth[k].ensure((size_t)ch * px * sizeof(float)), "alloc depth slots");
        if (shadow) CG_TRY(c, c->rs_shadow[k].ensure((size_t)ch * px * sizeof(int32_t)), "alloc shadow slots");
    }
    const size_t rec_bytes = ((size_t)n_frames + 1) * sizeof(cg_rast_seq_frame);
    CG_TRY(c, c->rs_info.ensure(rec_bytes), "alloc records");
    CG_TRY(c, c->rs_host.ensure(rec_bytes + sizeof(int)), "alloc host records");
    cg_rast_seq_frame *d_info = (cg_rast_seq_frame *)c->rs_info.p, *rec = (cg_rast_seq_frame *)c->rs_host.p;
    int *h_ntris = (int *)((char *)c->rs_host.p + rec_bytes);
    const int nchunks = (n_frames + ch - 1) / ch;
    auto plane = [&](void *dst, const void *src, int f0, int nf) -> hipError_t {   // 4-byte pixels
        if (stride == px)
            return hipMemcpyAsync((uint32_t *)dst + (size_t)f0 * px, src, (size_t)nf * px * 4, hipMemcpyDeviceToHost,
                                  c->xfer);
        for (int f = 0; f < nf; ++f) {
            const hipError_t e = hipMemcpyAsync((uint32_t *)dst + (size_t)(f0 + f) * stride,
                                                (const uint32_t *)src + (size_t)f * px, px * 4, hipMemcpyDeviceToHost,
                                                c->xfer);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    auto download = [&](int j) -> int {
        const int s = j % NS, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        CG_TRY(c, hipStreamWaitEvent(c->xfer, c->rs_rdone[s], 0), "copy wait");
        CG_TRY(c, plane(argb, c->rs_argb[s].p, f0, nf), "download frames");
        if (depth) CG_TRY(c, plane(depth, c->rs_depth[s].p, f0, nf), "download depth");
        if (shadow) CG_TRY(c, plane(shadow, c->rs_shadow[s].p, f0, nf), "download shadow");
        CG_TRY(c, hipEventRecord(c->rs_cdone[s], c->xfer), "copy event");
        return CG_OK;
    };
    CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
    for (int j = 0; j < nchunks; ++j) {
        const int s = j % NS, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        if (j >= NS) CG_TRY(c, hipStreamWaitEvent(c->stream, c->rs_cdone[s], 0), "slot wait");   // chunk j - NS downloaded
        int rc = rast_sequence_device(c, ps + f0, nf, (uint32_t *)c->rs_argb[s].p,
                                      depth ? (float *)c->rs_depth[s].p : nullptr,
                                      shadow ? (int32_t *)c->rs_shadow[s].p : nullptr, px, d_info + f0, c->stream, j > 0,
                                      host_lanes);
        if (rc) return rc;
        CG_TRY(c, hipEventRecord(c->rs_rdone[s], c->stream), "render event");
        if (j >= 1 && (rc = download(j - 1))) return rc;
    }
    CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
    if (int rc = download(nchunks - 1)) return rc;
    CG_TRY(c, hipMemcpyAsync(rec, d_info, rec_bytes, hipMemcpyDeviceToHost, c->stream), "d2h records");
    *h_ntris = (int)std::max(c->rlast.n, 0ll);
    if (stats && c->rlast.n < 0 && c->rlast.n_dev)
        CG_TRY(c, hipMemcpyAsync(h_ntris, c->rlast.n_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h count");
    CG_TRY(c, hipStreamSynchronize(c->xfer), "download frames");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rast frames");
    float kernel_ms = 0.f;
    (void)hipEventElapsedTime(&kernel_ms, c->ev0, c->ev1);
    // A frame the stream's capacity could not hold was flagged and left undrawn, the chain exact:
    // it renders alone from its record through the single-frame path, straight into its host slot.
    int rc_out = CG_OK;
    long long shaded = -1;
    bool kept = false;
    const bool last_flagged = rec[n_frames - 1].status != 0;   // then the last repair is the last frame
    RastLast last;
    for (int f = 0; f < n_frames; ++f) {
        if (ps[f].colour_mode != 0) shaded = std::max(shaded, 0ll) + rec[f].n_shaded;
        if (rec[f].status == 0 || rc_out) continue;
        if (rec[f].status == CG_E_CAPACITY) {
            if (!kept && !last_flagged) {   // cg_rast_scratch_info reports the call's last frame
                if (const int rc = rast_last_resolve(c)) return rc;
                last = c->rlast;
                kept = true;
            }
            cg_rast_params p = ps[f];
            p.rand_offset = rec[f].rand_offset;
            const int rc = cg_rast_draw(c, &p, argb + (size_t)f * stride, depth ? depth + (size_t)f * stride : nullptr,
                                        shadow ? shadow + (size_t)f * stride : nullptr, nullptr);
            if (rc == CG_OK) rec[f].status = 0;
            else rc_out = rc;
        } else {
            rc_out = rec[f].status;
        }
    }
    if (kept) c->rlast = last;
    if (info) std::memcpy(info, rec, rec_bytes);
    if (stats) {
        stats->kernel_ms = kernel_ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = *h_ntris;
        stats->n_spans = 0;
        stats->n_shaded = shaded;
    }
    return rc_out;
}

constexpr int kRastHdrChunkFrames = 8;   // frames of the float scratch (kBufRastHdr) of cg_rast_draw_exposed_device

// cg_rast_draw_sequence's frames delivered compressed: its chunks of the device sequence (ARGB only),
// each encoded on the context's stream behind its render and copied while the next chunk renders
// (JpegDelivery, cg_ctx.h).  The records and the rand() index chain are the device sequence's, so
// they equal cg_rast_draw_sequence's.  A frame the stream's capacity could not hold is repaired
// after the last chunk as there -- drawn alone from its record -- encoded, and put in its place
// among the files, which are laid out again behind it.
// JPEG files under jp, or PNG files under pp (`who` names the call in messages), or EXR files under
// ep: then a chunk is at most 8 frames of the float sequence (CG_PIX_RGBA_F32) in the exposed calls'
// scratch -- one set is enough, since a chunk's encoding stands on the stream before the next
// chunk's render -- and a repaired frame is drawn as a float picture.
static int rast_sequence_files(cg_ctx *c, const cg_rast_params *ps, int n_frames, const cg_jpeg_params *jp,
                               const cg_png_params *pp, const cg_exr_params *ep, uint8_t *out, size_t cap, size_t *offsets,
                               int chunk, cg_rast_seq_frame *info, cg_stats *stats, const char *who)
{
    if (!c || !offsets || n_frames < 0 || (n_frames && !ps) || (!out && cap)) return CG_E_INVALID;
    if (ep ? false : pp ? ((pp->colour != CG_PNG_RGB && pp->colour != CG_PNG_RGBA) ||
              (pp->filter != CG_PNG_FILTER_ADAPTIVE && (pp->filter < 0 || pp->filter > 4)))
           : (!jp || jp->quality < 1 || jp->quality > 100 || (jp->subsampling != CG_JPEG_444 && jp->subsampling != CG_JPEG_420)))
        return CG_E_INVALID;
    const std::string name(who);
    if (chunk < 0 || chunk > (ep ? kRastHdrChunkFrames : 64))
        return ctx_invalid(c, (name + (ep ? ": chunk 0 .. 8" : ": chunk 0 .. 64")).c_str());
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    offsets[0] = 0;
    if (n_frames == 0) return CG_OK;
    const int W = ps[0].width, H = ps[0].height;
    if (W <= 2 || H <= 2 || W > 65535 || H > 65535) return ctx_invalid(c, (name + ": frame size").c_str());
    const size_t px = (size_t)W * H;
    for (int f = 0; f < n_frames; ++f)
        if (ps[f].colour_mode < 0 || ps[f].colour_mode > 2 || ps[f].width != W || ps[f].height != H)
            return ctx_invalid(c, (name + ": colour modes 0-2, frames of one size").c_str());
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const int ch = std::min(chunk ? chunk : 8, n_frames);
    static const int host_lanes = [] {   // cg_rast_draw_sequence's
        const char *e = std::getenv("CG_RAST_HOST_LANES");
        return std::max(1, std::min(e ? std::atoi(e) : 2, (int)cg_ctx::kRastLanes));
    }();
    struct Drain {
        cg_ctx *c;
        ~Drain()
        {
            (void)hipStreamSynchronize(c->xfer);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain_on_exit{c};
    JpegDelivery D{c, W, H, n_frames, ch, jp ? *jp : cg_jpeg_params{}, out, cap, offsets};
    if (pp) D.png = true, D.pprm = *pp;
    if (ep) D.exr = true, D.eprm = *ep;
    if (int rc = D.begin()) return rc;
    float *rgba = nullptr;
    if (ep) {
        hipError_t e;
        rgba = (float *)ctx_buf(c, kBufRastHdr, kRastHdrChunkFrames * px * 16, &e);
        if (!rgba) return ctx_fail(c, e, "alloc picture frames");
    } else
        for (int k = 0; k < 2; ++k) CG_TRY(c, c->rs_argb[k].ensure((size_t)ch * px * sizeof(uint32_t)), "alloc frame slots");
    const size_t rec_bytes = ((size_t)n_frames + 1) * sizeof(cg_rast_seq_frame);
    CG_TRY(c, c->rs_info.ensure(rec_bytes), "alloc records");
    CG_TRY(c, c->rs_host.ensure(rec_bytes + sizeof(int)), "alloc host records");
    cg_rast_seq_frame *d_info = (cg_rast_seq_frame *)c->rs_info.p, *rec = (cg_rast_seq_frame *)c->rs_host.p;
    int *h_ntris = (int *)((char *)c->rs_host.p + rec_bytes);
    const int nchunks = (n_frames + ch - 1) / ch;
    CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
    for (int j = 0; j < nchunks; ++j) {
        const int s = j & 1, f0 = j * ch, nf = std::min(ch, n_frames - f0);
        int rc = D.slot_wait(j);
        if (rc) return rc;
        rc = rast_sequence_device(c, ps + f0, nf, ep ? (uint32_t *)rgba : (uint32_t *)c->rs_argb[s].p, nullptr, nullptr, px,
                                  d_info + f0, c->stream, j > 0, host_lanes, ep ? CG_PIX_RGBA_F32 : CG_PIX_ARGB8888);
        if (rc) return rc;
        if ((rc = D.encode(j, ep ? (const void *)rgba : c->rs_argb[s].p, px))) return rc;
        if (j >= 1 && (rc = D.deliver(j - 1))) return rc;
    }
    CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
    if (int rc = D.deliver(nchunks - 1)) return rc;
    CG_TRY(c, hipMemcpyAsync(rec, d_info, rec_bytes, hipMemcpyDeviceToHost, c->stream), "d2h records");
    *h_ntris = (int)std::max(c->rlast.n, 0ll);
    if (stats && c->rlast.n < 0 && c->rlast.n_dev)
        CG_TRY(c, hipMemcpyAsync(h_ntris, c->rlast.n_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h count");
    int rc_out = D.finish();
    if (rc_out != CG_OK && rc_out != CG_E_CAPACITY) return rc_out;
    float kernel_ms = 0.f;
    (void)hipEventElapsedTime(&kernel_ms, c->ev0, c->ev1);
    long long shaded = -1;
    bool flagged = false;
    for (int f = 0; f < n_frames; ++f) {
        if (ps[f].colour_mode != 0) shaded = std::max(shaded, 0ll) + rec[f].n_shaded;
        flagged = flagged || rec[f].status != 0;
    }
    if (flagged) {
        // what `out` holds of the first pass, then every file again in order: a repaired frame's from
        // its own encoding, the others' from the copy
        std::vector<size_t> old(offsets, offsets + n_frames + 1);
        size_t have = 0;   // frames of the first pass that are whole in `out`
        while (have < (size_t)n_frames && old[have + 1] <= cap) ++have;
        const std::vector<uint8_t> first(out, out + old[have]);
        const bool last_flagged = rec[n_frames - 1].status != 0;
        bool kept = false, stop = false;
        RastLast last;
        std::vector<uint32_t> frame(ep ? 4 * px : px);   // a float picture has four words a pixel
        std::vector<uint8_t> file;
        for (int f = 0; f < n_frames; ++f) {
            const uint8_t *src = (size_t)f < have ? first.data() + old[f] : nullptr;
            size_t len = old[f + 1] - old[f];
            if (rec[f].status == CG_E_CAPACITY) {
                if (!kept && !last_flagged) {   // cg_rast_scratch_info reports the call's last frame
                    if (const int rc = rast_last_resolve(c)) return rc;
                    last = c->rlast;
                    kept = true;
                }
                cg_rast_params p = ps[f];
                p.rand_offset = rec[f].rand_offset;
                int rc = ep ? cg_rast_draw_picture(c, &p, (float *)frame.data(), nullptr)
                            : cg_rast_draw(c, &p, frame.data(), nullptr, nullptr, nullptr);
                if (rc) return rc;
                file.resize((size_t)(ep   ? cg_image_exr_bound(W, H, ep->channels, ep->type)
                                     : pp ? cg_image_png_bound(W, H, pp->colour)
                                          : cg_image_jpeg_bound(W, H, jp->subsampling)));
                if ((rc = ep ? cg_image_encode_exr(c, (const float *)frame.data(), W, H, 0, ep, file.data(), file.size(), &len)
                        : pp ? cg_image_encode_png(c, frame.data(), W, H, 0, pp, file.data(), file.size(), &len)
                             : cg_image_encode_jpeg(c, frame.data(), W, H, 0, jp, file.data(), file.size(), &len)))
                    return rc;
                src = file.data();
                rec[f].status = 0;
            } else if (rec[f].status != 0) {
                return rec[f].status;
            }
            offsets[f + 1] = offsets[f] + len;
            stop = stop || !src || offsets[f + 1] > cap;
            if (!stop) std::memcpy(out + offsets[f], src, len);
        }
        if (kept) c->rlast = last;
        // a first pass that did not fit left files missing: the capacity asked for holds both passes
        if (have < (size_t)n_frames) offsets[n_frames] = std::max(offsets[n_frames], old[n_frames]);
        rc_out = offsets[n_frames] > cap ? CG_E_CAPACITY : CG_OK;
    }
    if (info) std::memcpy(info, rec, rec_bytes);
    if (stats) {
        stats->kernel_ms = kernel_ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = *h_ntris;
        stats->n_spans = 0;
        stats->n_shaded = shaded;
    }
    return rc_out;
}

extern "C" int cg_rast_draw_sequence_jpeg(cg_ctx *c, const cg_rast_params *ps, int n_frames,
                                          const cg_jpeg_params *params, uint8_t *out, size_t cap, size_t *offsets,
                                          int chunk, cg_rast_seq_frame *info, cg_stats *stats)
{
    return rast_sequence_files(c, ps, n_frames, params, nullptr, nullptr, out, cap, offsets, chunk, info, stats,
                               "draw_sequence_jpeg");
}

extern "C" int cg_rast_draw_sequence_png(cg_ctx *c, const cg_rast_params *ps, int n_frames, const cg_png_params *params,
                                         uint8_t *out, size_t cap, size_t *offsets, int chunk, cg_rast_seq_frame *info,
                                         cg_stats *stats)
{
    if (!params) return CG_E_INVALID;
    return rast_sequence_files(c, ps, n_frames, nullptr, params, nullptr, out, cap, offsets, chunk, info, stats,
                               "draw_sequence_png");
}

extern "C" int cg_rast_draw_sequence_exr(cg_ctx *c, const cg_rast_params *ps, int n_frames, const cg_exr_params *params,
                                         uint8_t *out, size_t cap, size_t *offsets, int chunk, cg_rast_seq_frame *info,
                                         cg_stats *stats)
{
    cg_exr_params prm;
    if (!exr_resolve_params(params, &prm)) return CG_E_INVALID;
    return rast_sequence_files(c, ps, n_frames, nullptr, nullptr, &prm, out, cap, offsets, chunk, info, stats,
                               "draw_sequence_exr");
}

// ---- the float picture (CG_PIX_RGBA_F32) and exposed frames (kernels: the post-pass's *_f32
// variants, cg_hdr.hip's rast_tonemap_pack_kernel) ----
extern "C" int cg_rast_draw_picture_device(cg_ctx *c, const cg_rast_params *p, float *d_rgba, float *d_depth,
                                           int32_t *d_shadow, void *stream)
{
    if (!c || !p || !d_rgba || ((uintptr_t)d_rgba & 15)) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    return rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p, c->n_boxes, p,
                            (uint32_t *)d_rgba, d_depth, d_shadow, stream ? (hipStream_t)stream : c->stream, nullptr,
                            nullptr, c->scene_tex, nullptr, CG_PIX_RGBA_F32);
}

extern "C" int cg_rast_draw_picture(cg_ctx *c, const cg_rast_params *p, float *rgba, cg_stats *stats)
{
    if (!c || !p || !rgba || p->width <= 2 || p->height <= 2) return CG_E_INVALID;
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t bytes = (size_t)p->width * p->height * 16;
    hipError_t e;
    float *d_rgba = (float *)ctx_buf(c, kBufRastHdr, bytes, &e);
    if (!d_rgba) return ctx_fail(c, e, "alloc picture");
    int *d_n = nullptr;
    const int rc = rast_draw_device(c, (const cg_rtri *)c->rroom.p, c->n_room, (const cg_rtri *)c->rboxes.p, c->n_boxes,
                                    p, (uint32_t *)d_rgba, nullptr, nullptr, c->stream, stats, &d_n, c->scene_tex,
                                    nullptr, CG_PIX_RGBA_F32);
    if (rc) return rc;
    int n = 0;
    CG_TRY(c, hipMemcpyAsync(&n, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream), "d2h count");
    CG_TRY(c, hipMemcpyAsync(rgba, d_rgba, bytes, hipMemcpyDeviceToHost, c->stream), "d2h picture");
    CG_TRY(c, hipStreamSynchronize(c->stream), "rast frame");
    if (stats) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = n;
    }
    return CG_OK;
}

extern "C" int cg_rast_draw_sequence_picture_device(cg_ctx *c, const cg_rast_params *ps, int n_frames, float *d_rgba,
                                                    float *d_depth, int32_t *d_shadow, size_t frame_stride,
                                                    cg_rast_seq_frame *d_info, void *stream)
{
    if ((uintptr_t)d_rgba & 15) return CG_E_INVALID;
    return rast_sequence_device(c, ps, n_frames, (uint32_t *)d_rgba, d_depth, d_shadow, frame_stride, d_info, stream,
                                false, 0, CG_PIX_RGBA_F32);
}

extern "C" int cg_rast_tonemap_pack_device(cg_ctx *c, const float *d_rgba, size_t n_pixels, int n_frames,
                                           size_t src_stride, const float *d_scales, int op, float white2,
                                           uint32_t *d_argb, size_t dst_stride, void *stream)
{
    if (!c || n_frames < 0 || !hdr_tone_ok(op, white2) || n_pixels >= ((size_t)1 << 32)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const size_t ss = src_stride ? src_stride : n_pixels, ds = dst_stride ? dst_stride : n_pixels;
    if (!d_scales || ((uintptr_t)d_scales & 3) || (n_pixels && (!d_rgba || !d_argb)) || ((uintptr_t)d_rgba & 15) ||
        ((uintptr_t)d_argb & 3) || ss < n_pixels || ds < n_pixels)
        return CG_E_INVALID;
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    CG_TRY(c, launch_rast_tonemap_pack(d_rgba, n_pixels, n_frames, ss, d_scales, op, white2, d_argb, ds,
                                       stream ? (hipStream_t)stream : c->stream),
           "tonemap pack launch");
    return CG_OK;
}

// what both forms of cg_rast_draw_exposed check before anything is enqueued (the sequence checks the rest)
static int rast_exposed_check(cg_ctx *c, const cg_rast_params *ps, int n_frames, const cg_hdr_exposure_params *params,
                              int op, float white2, size_t frame_stride, const cg_hdr_bloom_params *bloom)
{
    if (!c || n_frames < 0 || (n_frames && !ps)) return CG_E_INVALID;
    if (!hdr_params_ok(params)) return ctx_invalid(c, "draw_exposed: exposure parameters");
    if (bloom && !bloom_params_ok(bloom)) return ctx_invalid(c, "draw_exposed: bloom parameters");
    if (!hdr_tone_ok(op, white2)) return ctx_invalid(c, "draw_exposed: tone curve");
    if (c->n_room < 0) {
        c->err = "draw before cg_rast_set_scene";
        return CG_E_NOSCENE;
    }
    if (n_frames == 0) return CG_OK;
    if (ps[0].width <= 2 || ps[0].height <= 2) return ctx_invalid(c, "draw_exposed: frame size");
    const size_t px = (size_t)ps[0].width * ps[0].height;
    for (int f = 0; f < n_frames; ++f)
        if (ps[f].colour_mode < 0 || ps[f].colour_mode > 2 || ps[f].width != ps[0].width ||
            ps[f].height != ps[0].height || (frame_stride && frame_stride < px))
            return ctx_invalid(c, "draw_exposed: colour modes 0-2, frames of one size, frame_stride >= W * H");
    return CG_OK;
}

// Frames f0 .. f0 + nf - 1 (nf <= kRastHdrChunkFrames) of an exposed call: the float sequence into
// the context's scratch (resuming at d_info[0] when f0 > 0), then histogram, exposure (previous
// scale *d_prev) and pack, all on st.  d_info: the chunk's first record.  With bloom: the chunk's
// pyramids into scratch after the exposure, and the composite (rule RAST) for the pack.
static int rast_exposed_chunk(cg_ctx *c, const cg_rast_params *ps, int f0, int nf,
                              const cg_hdr_exposure_params &params, const float *d_prev, int op, float white2,
                              const cg_hdr_bloom_params *bloom, uint32_t *d_argb, size_t stride, float *d_scales, cg_rast_seq_frame *d_info,
                              hipStream_t st)
{
    const size_t px = (size_t)ps[0].width * ps[0].height;
    hipError_t e;
    float *rgba = (float *)ctx_buf(c, kBufRastHdr, kRastHdrChunkFrames * px * 16, &e);
    if (!rgba) return ctx_fail(c, e, "alloc exposure frames");
    CG_TRY(c, c->hdr_hist.ensure(kRastHdrChunkFrames * CG_HDR_BINS * sizeof(uint32_t)), "alloc exposure histograms");
    const int rc = rast_sequence_device(c, ps + f0, nf, (uint32_t *)rgba, nullptr, nullptr, px, d_info, st, f0 > 0, 0,
                                        CG_PIX_RGBA_F32);
    if (rc) return rc;
    uint32_t *hist = (uint32_t *)c->hdr_hist.p;
    CG_TRY(c, launch_hdr_histogram(rgba, 4, px, nf, px, hist, nullptr, st), "histogram launch");
    CG_TRY(c, launch_hdr_exposure(hist, nf, params, d_prev, d_scales, st), "exposure launch");
    if (bloom) {
        BloomLayout L;
        if (!bloom_layout(ps[0].width, ps[0].height, bloom->levels, &L)) return CG_E_INVALID;
        CG_TRY(c, c->bloom_planes.ensure(kRastHdrChunkFrames * L.total * 16), "alloc bloom planes");
        CG_TRY(c, c->bloom_pyr.ensure(kRastHdrChunkFrames * L.total * 16), "alloc bloom pyramids");
        float *pyr = (float *)c->bloom_pyr.p;
        CG_TRY(c, launch_bloom_pyramid(rgba, L, nf, px, d_scales, *bloom, (float *)c->bloom_planes.p, pyr, L.total, st),
               "bloom launch");
        CG_TRY(c, launch_bloom_pack(rgba, pyr, L, nf, px, L.total, d_scales, *bloom, CG_BLOOM_RULE_RAST, op, white2,
                                    d_argb, stride, st),
               "bloom pack launch");
        return CG_OK;
    }
    CG_TRY(c, launch_rast_tonemap_pack(rgba, px, nf, px, d_scales, op, white2, d_argb, stride, st), "tonemap pack launch");
    return CG_OK;
}

extern "C" int cg_rast_draw_exposed_bloom_device(cg_ctx *c, const cg_rast_params *ps, int n_frames,
                                                 const cg_hdr_exposure_params *params, const float *d_prev, int op,
                                                 float white2, const cg_hdr_bloom_params *bloom, uint32_t *d_argb,
                                                 size_t frame_stride, float *d_scales, cg_rast_seq_frame *d_info,
                                                 void *stream)
{
    if (int rc = rast_exposed_check(c, ps, n_frames, params, op, white2, frame_stride, bloom)) return rc;
    if (n_frames == 0) return CG_OK;
    if (!d_argb || ((uintptr_t)d_argb & 3) || !d_scales || ((uintptr_t)d_scales & 3) || ((uintptr_t)d_prev & 3))
        return CG_E_INVALID;
    if (!d_info) return ctx_invalid(c, "draw_exposed: d_info is required");
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t stride = frame_stride ? frame_stride : (size_t)ps[0].width * ps[0].height;
    for (int f0 = 0; f0 < n_frames; f0 += kRastHdrChunkFrames) {
        const int nf = std::min(kRastHdrChunkFrames, n_frames - f0);
        if (int rc = rast_exposed_chunk(c, ps, f0, nf, *params, f0 ? d_scales + f0 - 1 : d_prev, op, white2, bloom,
                                        d_argb + (size_t)f0 * stride, stride, d_scales + f0, d_info + f0, st))
            return rc;
    }
    return CG_OK;
}

extern "C" int cg_rast_draw_exposed_device(cg_ctx *c, const cg_rast_params *ps, int n_frames,
                                           const cg_hdr_exposure_params *params, const float *d_prev, int op,
                                           float white2, uint32_t *d_argb, size_t frame_stride, float *d_scales,
                                           cg_rast_seq_frame *d_info, void *stream)
{
    return cg_rast_draw_exposed_bloom_device(c, ps, n_frames, params, d_prev, op, white2, nullptr, d_argb, frame_stride,
                                             d_scales, d_info, stream);
}

// Host-memory form: the device form's chunks into context scratch, each chunk's frames downloaded
// after its render; the scales (and the caller's previous scale) live in one device array,
// [0] the previous scale, [1 + f] frame f's; the records in the host sequence's device array.
extern "C" int cg_rast_draw_exposed_bloom(cg_ctx *c, const cg_rast_params *ps, int n_frames,
                                          const cg_hdr_exposure_params *params, const float *prev, int op, float white2,
                                          const cg_hdr_bloom_params *bloom, uint32_t *argb, size_t frame_stride,
                                          float *scales, cg_rast_seq_frame *info, cg_stats *stats)
{
    if (int rc = rast_exposed_check(c, ps, n_frames, params, op, white2, frame_stride, bloom)) return rc;
    if (n_frames == 0) return CG_OK;
    if (!argb || !scales) return CG_E_INVALID;
    auto t0 = std::chrono::steady_clock::now();
    CG_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t px = (size_t)ps[0].width * ps[0].height;
    const size_t stride = frame_stride ? frame_stride : px;
    CG_TRY(c, c->hdr_argb.ensure(kRastHdrChunkFrames * px * sizeof(uint32_t)), "alloc exposed frames");
    CG_TRY(c, c->hdr_scales.ensure(((size_t)n_frames + 1) * sizeof(float)), "alloc scales");
    const size_t rec_bytes = ((size_t)n_frames + 1) * sizeof(cg_rast_seq_frame);
    CG_TRY(c, c->rs_info.ensure(rec_bytes), "alloc records");
    float *d_s = (float *)c->hdr_scales.p;
    uint32_t *d_a = (uint32_t *)c->hdr_argb.p;
    cg_rast_seq_frame *d_info = (cg_rast_seq_frame *)c->rs_info.p;
    if (prev) CG_TRY(c, hipMemcpyAsync(d_s, prev, sizeof(float), hipMemcpyHostToDevice, c->stream), "upload scale");
    float ms_sum = 0.f;
    for (int f0 = 0; f0 < n_frames; f0 += kRastHdrChunkFrames) {
        const int nf = std::min(kRastHdrChunkFrames, n_frames - f0);
        CG_TRY(c, hipEventRecord(c->ev0, c->stream), "event");
        if (int rc = rast_exposed_chunk(c, ps, f0, nf, *params, f0 || prev ? d_s + f0 : nullptr, op, white2, bloom, d_a, px,
                                        d_s + 1 + f0, d_info + f0, c->stream))
            return rc;
        CG_TRY(c, hipEventRecord(c->ev1, c->stream), "event");
        for (int f = 0; f < nf; ++f)
            CG_TRY(c, hipMemcpyAsync(argb + (size_t)(f0 + f) * stride, d_a + (size_t)f * px, px * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost, c->stream),
                   "download frames");
        CG_TRY(c, hipStreamSynchronize(c->stream), "exposed frames");
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        ms_sum += ms;
    }
    CG_TRY(c, hipMemcpy(scales, d_s + 1, (size_t)n_frames * sizeof(float), hipMemcpyDeviceToHost), "download scales");
    std::vector<cg_rast_seq_frame> rec((size_t)n_frames + 1);
    CG_TRY(c, hipMemcpy(rec.data(), d_info, rec_bytes, hipMemcpyDeviceToHost), "download records");
    if (info) std::memcpy(info, rec.data(), rec_bytes);
    int rc_out = CG_OK;
    long long shaded = -1;
    for (int f = 0; f < n_frames; ++f) {
        if (ps[f].colour_mode != 0) shaded = std::max(shaded, 0ll) + rec[f].n_shaded;
        if (rec[f].status != 0 && rc_out == CG_OK) rc_out = rec[f].status;
    }
    if (stats) {
        stats->kernel_ms = ms_sum;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->n_tris = (int)std::max(c->rlast.n, 0ll);
        stats->n_spans = 0;
        stats->n_shaded = shaded;
    }
    return rc_out;
}

extern "C" int cg_rast_draw_exposed(cg_ctx *c, const cg_rast_params *ps, int n_frames,
                                    const cg_hdr_exposure_params *params, const float *prev, int op, float white2,
                                    uint32_t *argb, size_t frame_stride, float *scales, cg_rast_seq_frame *info,
                                    cg_stats *stats)
{
    return cg_rast_draw_exposed_bloom(c, ps, n_frames, params, prev, op, white2, nullptr, argb, frame_stride, scales,
                                      info, stats);
}
