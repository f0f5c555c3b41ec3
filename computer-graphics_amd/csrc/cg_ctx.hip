// cg_ctx.hip -- the context behind the extern "C" boundary (include/cg_render.h): creation,
// destruction, error text and the accessors the kernel files use.  Nothing throws across the
// ABI; HIP failures become CG_E_HIP with the HIP message kept for cg_last_error().
#include "cg_ctx.h"

namespace cg {
int ctx_device(const cg_ctx *c) { return c->device; }
hipStream_t ctx_stream(const cg_ctx *c) { return c->stream; }
void ctx_set_error(cg_ctx *c, const std::string &e) { c->err = e; }
// cg_rt_frame_columns over the context's scene (the full width without one)
void ctx_rt_columns(const cg_ctx *c, const cg_rt_camera *cam, int *c0, int *c1)
{
    *c0 = 0;
    *c1 = cam->width;
    if (c->n_tris >= 0 && cam->width > 0) rt_box_columns(c->box_lo, c->box_hi, cam, c0, c1);
}
// exposed to the rasteriser's, the starfield's and the image decoder's files: slot `which`
// (kBuf*, cg_host.h) grown to at least `bytes`
void *ctx_buf(cg_ctx *c, int which, size_t bytes, hipError_t *e)
{
    static DevBuf cg_ctx::*const fields[] = {
        &cg_ctx::rtris, &cg_ctx::rhdr,   &cg_ctx::rspan,  &cg_ctx::rpix,   &cg_ctx::rargb,    &cg_ctx::rdepth, &cg_ctx::rshadow,
        &cg_ctx::rcount, &cg_ctx::rrecs, &cg_ctx::rgeo,   &cg_ctx::rpc,    &cg_ctx::rtl,      &cg_ctx::rrnd,   &cg_ctx::rjt,
        &cg_ctx::sstars, &cg_ctx::sframe, &cg_ctx::rtexel, &cg_ctx::iscratch, &cg_ctx::rseq,
        &cg_ctx::rhdr_rgba, &cg_ctx::jpeg_enc, &cg_ctx::jpeg_enc_io};
    static_assert(sizeof(fields) / sizeof(fields[0]) == kBufFieldsEnd && kBufFieldsEnd <= kBufBig0, "named slots");
    static_assert(sizeof(c->rbig) / sizeof(c->rbig[0]) == kBufBigEnd - kBufBig0 && kBufBigEnd <= kBufOwner, "rbig slots");
    static_assert(sizeof(c->rbuf) / sizeof(c->rbuf[0]) == kBufOwnerEnd - kBufOwner, "rbuf slots");
    DevBuf *b = nullptr;
    if (which >= 0 && which < kBufFieldsEnd) b = &(c->*fields[which]);
    else if (which >= kBufBig0 && which < kBufBigEnd) b = &c->rbig[which - kBufBig0];
    else if (which >= kBufOwner && which < kBufOwnerEnd) b = &c->rbuf[which - kBufOwner];
    if (!b) {
        *e = hipErrorInvalidValue;
        return nullptr;
    }
    *e = b->ensure(bytes);
    return *e == hipSuccess ? b->p : nullptr;
}
void *ctx_png_buf(cg_ctx *c, int which, size_t bytes, hipError_t *e)
{
    if (which != 0 && which != 1) {
        *e = hipErrorInvalidValue;
        return nullptr;
    }
    DevBuf &b = which ? c->png_enc_io : c->png_enc;
    *e = b.ensure(bytes);
    return *e == hipSuccess ? b.p : nullptr;
}
void *ctx_exr_buf(cg_ctx *c, int which, size_t bytes, hipError_t *e)
{
    if (which != 0 && which != 1) {
        *e = hipErrorInvalidValue;
        return nullptr;
    }
    DevBuf &b = which ? c->exr_enc_io : c->exr_enc;
    *e = b.ensure(bytes);
    return *e == hipSuccess ? b.p : nullptr;
}
StarState *ctx_star(cg_ctx *c) { return &c->star; }
int ctx_invalid(cg_ctx *c, const char *what)
{
    c->err = what;
    return CG_E_INVALID;
}
int ctx_fail(cg_ctx *c, hipError_t e, const char *what)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return CG_E_HIP;
}
void ctx_events(cg_ctx *c, hipEvent_t *a, hipEvent_t *b)
{
    *a = c->ev0;
    *b = c->ev1;
}
int ctx_rast_route(cg_ctx *c, long long cap, bool colour)
{
    if (c->rast_route >= 0) return c->rast_route;
    if (c->route_limit > 0) return cap <= c->route_limit ? CG_RAST_ROUTE_DENSE : CG_RAST_ROUTE_COMPACT;
    if (colour && cap > kRastDenseColourList) return CG_RAST_ROUTE_COMPACT;
    return cg_rast_route(cap);
}
bool ctx_rast_forced_compact(cg_ctx *c) { return c->rast_route == CG_RAST_ROUTE_COMPACT; }
RastLast *ctx_rast_last(cg_ctx *c) { return &c->rlast; }
RastFrame *ctx_rast_frame(cg_ctx *c) { return &c->rframe; }
bool ctx_rast_want_owner(cg_ctx *c) { return c->rast_want_owner; }
// the device texture maps and which textures are renderable (bit k: texture k)
int rast_tex_maps(cg_ctx *c, RastTexMaps *m)
{
    if (c->tex_owner) c = c->tex_owner;
    m->marble = (const uint8_t *)c->tmarble.p;
    m->marble_noise = (const float *)c->tnoise.p;
    m->woven = (const uint8_t *)c->twoven.p;
    m->woven_ao = (const uint8_t *)c->twoven_ao.p;
    m->woven_op = (const uint8_t *)c->twoven_op.p;
    m->woven_nrm = (const uint8_t *)c->twoven_nrm.p;
    m->grill = (const uint8_t *)c->tgrill.p;
    m->grill_op = (const uint8_t *)c->tgrill_op.p;
    m->grill_nrm = (const uint8_t *)c->tgrill_nrm.p;
    return c->tex_loaded;
}
}  // namespace cg

extern "C" int cg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int cg_create(int device, cg_ctx **out)
{
    if (!out) return CG_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CG_E_NODEVICE;
    if (device < 0 || device >= n) return CG_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return CG_E_NODEVICE;
    cg_ctx *c = new (std::nothrow) cg_ctx;
    if (!c) return CG_E_INVALID;
    c->device = device;
    if (c->stream.ensure(hipStreamNonBlocking) != hipSuccess || c->ev0.ensure(hipEventDefault) != hipSuccess ||
        c->ev1.ensure(hipEventDefault) != hipSuccess) {
        delete c;
        return CG_E_HIP;
    }
    *out = c;
    return CG_OK;
}

// Waits for everything the context still has in flight, so that the members free nothing under
// a running kernel or copy; the lanes do the same in their own destructors.
cg_ctx::~cg_ctx()
{
    (void)hipSetDevice(device);
    for (const Stream *st : {&stream, &aux, &xfer, &star.xfer})
        if (*st) (void)hipStreamSynchronize(*st);
    // on a caller's stream, perhaps: the frames' demand read-backs and the starfield's latest work
    if (big_ev_live) (void)hipEventSynchronize(big_ev);
    for (ExtraSlot &x : xs) {
        if (x.st) (void)hipStreamSynchronize(x.st);
        if (x.ev_live) (void)hipEventSynchronize(x.ev);
    }
    if (hits.ev_live) (void)hipEventSynchronize(hits.ev);
    if (star.pending) (void)hipEventSynchronize(star.last);
}

extern "C" void cg_destroy(cg_ctx *c)
{
    if (c) delete c;
}

extern "C" int cg_debug_live(long long out[4])
{
    if (!out) return CG_E_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = own_live[k].load();
    return CG_OK;
}

extern "C" const char *cg_last_error(const cg_ctx *c) { return c ? c->err.c_str() : "no context"; }
