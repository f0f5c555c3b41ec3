// cg_ctx.h -- struct cg_ctx and what it is made of, for cg_ctx.hip and the cg_api_*.hip files
// alone: kernel files see the context through cg_host.h's accessors.  Every device buffer,
// pinned block, event and stream of the context is a member of an owning type (cg_own.h) and
// is freed by that member's destructor; ~cg_ctx only waits for the work still in flight.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include "cg_host.h"
#include "cg_rast_dev.h"
#include "cg_rt_grid.h"

using namespace cg;

// Host threads that store the certified-black columns of frames delivered
// into host memory (cg_rt_render / cg_rt_render_frames): a frame's 3.2 MB of
// black columns (C2) take one thread longer than the PCIe copy of its
// window, so the rows are shared by the workers and the caller.  run() hands
// out a job; wait() helps and returns when every row is stored.
class HostFill {
  public:
    struct Frame {
        uint32_t *dst;   // W x rows pixels, row pitch W
    };
    explicit HostFill(int n)
    {
        for (int i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
    }
    ~HostFill()
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void run(std::vector<Frame> frames, int W, int rows, int c0, int c1)
    {
        wait();
        {
            std::lock_guard<std::mutex> g(mu_);
            fr_ = std::move(frames);
            W_ = W;
            rows_ = rows;
            c0_ = c0;
            c1_ = c1;
            total_ = (int)fr_.size() * rows;
            next_.store(0);
            busy_ = (int)th_.size();
            ++gen_;
        }
        cv_.notify_all();
    }
    void wait()
    {
        work();
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return busy_ == 0; });
    }

  private:
    static constexpr int kRowsPerGrab = 32;
    void work()
    {
        for (;;) {
            const int r0 = next_.fetch_add(kRowsPerGrab);
            if (r0 >= total_) return;
            const int r1 = std::min(total_, r0 + kRowsPerGrab);
            for (int r = r0; r < r1; ++r) {
                uint32_t *row = fr_[r / rows_].dst + (size_t)(r % rows_) * W_;
                std::fill(row, row + c0_, 0x80000000u);   // PutPixelSDL(0, 0, 0)
                std::fill(row + c1_, row + W_, 0x80000000u);
            }
        }
    }
    void loop()
    {
        unsigned seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return quit_ || gen_ != seen; });
                if (quit_) return;
                seen = gen_;
            }
            work();
            std::lock_guard<std::mutex> g(mu_);
            if (--busy_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    bool quit_ = false;
    unsigned gen_ = 0;
    int busy_ = 0;
    std::vector<Frame> fr_;
    int W_ = 0, rows_ = 1, c0_ = 0, c1_ = 0, total_ = 0;
    std::atomic<int> next_{0};
};

struct cg_ctx {
    // Members are destroyed in reverse order of declaration, after ~cg_ctx has waited for the
    // work in flight.  So a stream is declared before the buffers and events used on it (it goes
    // last), and a member that reads another at destruction is declared after that other.
    ~cg_ctx();
    int device = 0;
    Stream stream;
    // Batched lattice launches pipeline their certificate kernels on `aux`:
    // call j+1's certificates run beside call j's lattice kernel, each call
    // with its own slot of buffers (rt_enqueue_lattice_batch).
    Stream aux;
    // cg_rt_render_frames, cg_rast_draw_sequence (host output): chunks render into two device
    // slots and download on `xfer` while the next chunk renders
    Stream xfer;
    Event ev0, ev1;   // timing events
    std::string err;
    // RT scene
    int n_tris = -1, n_sph = 0;
    float nbound = 0.f;   // largest |normal component| of the scene (shadow certificate)
    DevBuf tris, geo, tc, shade, sph, frame, probe_a, probe_b, probe_c, probe_d, lights, big, gstart, gtris;
    DevBuf latmask;                     // lattice tiles' certificates (two masks per tile)
    DevBuf supmask;                     // their super-tiles' certificates (two-level path)
    DevBuf umask;                       // light sets: the tiles' per-unit shadow masks
    DevBuf objmask, pobj[2];            // one-light lattice: shadow masks per object (kObjSlots a tile), as latmask / plat
    // the latest lattice call's certificates, for cg_rt_tile_masks (null: none since the scene changed)
    struct {
        const unsigned long long *lat = nullptr, *obj = nullptr;
        int tiles_x = 0, tiles_y = 0, frames = 0;
        int col0 = 0, col1 = 0;   // the tile columns the call certified (a windowed launch: its super-tiles')
        hipStream_t st = nullptr;
    } last_masks;
    // how the latest batched lattice call was launched, for cg_rt_lattice_path
    int last_path[4] = {0, 0, 0, 0};   // measured order, published certificates, forced uncertified, workgroups
    Event ev_cert[2], ev_lat[2];      // the aux pipeline's, per slot
    int slot = 0;
    DevBuf ptc[2], plat[2], psup[2], pumask[2];
    // measured lattice order (LatOrder, cg_internal.h): per slot, the recording
    // of its last lattice launch (class per tile) and the order sorted for it
    DevBuf lcost[2], lflat[2];
    int umask_frames = 0;                            // light sets: frames the unit-mask slots are sized for
    DevBuf pflag[2];                  // published-certificate words per slot (LatPublish / LatReady)
    uint32_t cert_gen = 0u;           // generation of the latest published call
    unsigned long long lrec_key[2] = {0ull, 0ull};   // geometry key of the slot's recording (0: none)
    unsigned rt_scene_gen = 0;                       // cg_rt_set_scene count (part of the key)
    // cg_rt_render_frames (host output): the two device slots and their events on `xfer`
    Event ev_rdone[2], ev_cdone[2];
    DevBuf hslot[2];
    // cg_rt_render_exposed_device: a chunk's CG_PIX_RGBA_F32 frames and histograms; the host form's
    // chunk of ARGB frames, its scales and previous scale
    DevBuf hdr_rgba, hdr_hist, hdr_argb, hdr_scales;
    // the bloom calls (cg_hdr_bloom_device, cg_*_exposed_bloom*): the unblurred planes B_k of up to 8
    // frames, and the exposed calls' pyramids of a chunk
    DevBuf bloom_planes, bloom_pyr;
    // their black columns (created on first use); declared after hslot: the threads end first
    std::unique_ptr<HostFill> hfill;
    RtGrid grid{};                      // large scenes only (n_tris > 64)
    GridBuild gbuild;                   // cg_rt_set_scene_device: the device builder's scratch and counts
    uint64_t grid_entries = 0;          // entries of the installed grid (either builder)
    long long grid_cap_entries = 0, grid_cap_cands = 0;   // cg_rt_set_grid_caps (0 = default)
    int pend_cap = 0;                   // cg_rt_set_pending_cap (0 = default)
    // large-scene pools (cg_rt_big.hip): capacities in entries, sized on the
    // scene's first frame, then grown from the demand later frames report
    BigCaps big_caps{};
    bool big_sized = false;
    long long big_key = -1;                     // frame shape / path the pools were sized for
    bool big_fixed = false;                     // cg_rt_set_pool_caps: capacities pinned (test hook)
    PinnedBuf big_demand;                       // unsigned long long [4]: the latest frame's demand
    Event big_ev;
    bool big_ev_live = false;
    unsigned long long big_last[4] = {};
    bool big_last_hits = false;                 // big_last came from a hits-only pass (its own capacities)
    long long big_overflows = 0;
    // Large scenes, several frames in flight (rt_render_frames): slots 1 ..
    // kBigSlots - 1 with their own buffers, stream and demand read-back; slot 0
    // is tc / shade / big / frame / big_demand / big_ev above.  A frame's list
    // building and walks are latency-bound phases; independent frames fill
    // each other's gaps.
    static constexpr int kBigSlots = 4;
    struct ExtraSlot {
        Stream st;
        DevBuf tc, big, frame;
        PinnedBuf demand;
        Event ev, done;
        bool ev_live = false;
    } xs[kBigSlots - 1];
    Event bev_start;
    // Hit planes (cg_rt_hits_device, cg_rt_pick).  A hits-only pass of a large scene has buffers of
    // its own -- the pass's RtTri, scratch, demand read-back -- so it never touches what a frame in
    // flight on another stream reads, and pool capacities and a sizing state of its own, so frames
    // and hit planes that alternate do not size the pools again each time.
    struct HitsSlot {
        DevBuf tc, big, planes, pick;
        BigCaps caps{};
        bool sized = false;
        long long key = -1;
        PinnedBuf demand;
        Event ev;
        bool ev_live = false;
    } hits;
    // the scene's box (rt_scene_box, once per cg_rt_set_scene): cg_dist's column
    // window of any camera from it in O(1) per frame -- no per-camera pass over
    // the scene (1M triangles: ~6 ms on the host) and no per-camera cache
    double box_lo[3] = {1e300, 1e300, 1e300}, box_hi[3] = {-1e300, -1e300, -1e300};
    std::vector<RtLight> lights_host;   // what `lights` holds (re-uploaded only on change)
    // Frame sequences (cg_rt_render_sequence_device): a call's n_frames x n_lights lights and its
    // RtFrameRec table, uploaded once through pinned staging memory into one of two slots, so that
    // two calls queued back to back read their own (ev_lat's discipline): `up` after the slot's
    // upload (the staging memory is free again), `done` after the call's last kernel (the device
    // copy is).  Both slots grow together, so only the first call of a size allocates.
    struct SeqSlot {
        DevBuf dev;
        PinnedBuf host;
        Event up, done;
    } seq[2];
    int seq_slot = 0;
    // RAST scratch (owned by cg_rast.hip)
    DevBuf rtris, rhdr, rspan, rpix, rargb, rdepth, rshadow, rcount, rrecs, rgeo, rroom, rboxes;
    DevBuf rpc, rtl, rrnd, rjt;          // colour modes 1-2 (cg_rast_colour.hip)
    DevBuf rbig[15];                     // the compact route's own buffers (cg_rast_big.hip)
    int rast_route = -1;                 // cg_rast_set_route: -1 automatic, else the forced route
    long long route_limit = 0;           // cg_rast_set_route_limit: 0 = cg_rast_route's 131072
    RastLast rlast;                      // the latest rasteriser frame (cg_rast_scratch_info)
    // cg_rast_draw_buffers*, cg_rast_pick (cg_rast_buffers.hip): what the latest frame left in
    // scratch, whether a buffers call is running it, and the calls' own buffers (kBufOwner ..)
    RastFrame rframe;
    bool rast_want_owner = false;
    DevBuf rbuf[9];
    // cg_rast_draw_sequence_device: the generator's tables (windows, seed words, J_b for
    // rseq_chunks chunks) and the stream's capacity in fragments (0: 4 * W * H)
    DevBuf rseq;
    // cg_rast_draw_exposed*: a chunk of 8 CG_PIX_RGBA_F32 frames (kBufRastHdr); the histograms, the
    // host form's ARGB chunk and scales are the raytracer chain's (hdr_hist, hdr_argb, hdr_scales)
    DevBuf rhdr_rgba;
    long long rseq_chunks = 0, rand_cap = 0;
    // cg_rast_draw_sequence (host output): two sets of plane slots of `chunk` frames (downloaded on
    // `xfer` as hslot is, with events of their own), the call's n_frames + 1 device records, and their
    // pinned host copy followed by one int for the last frame's clipped count
    static constexpr int kRastHostSlots = 2;
    DevBuf rs_argb[kRastHostSlots], rs_depth[kRastHostSlots], rs_shadow[kRastHostSlots], rs_info;
    Event rs_rdone[kRastHostSlots], rs_cdone[kRastHostSlots];
    PinnedBuf rs_host;
    DevBuf sstars, sframe;               // starfield (cg_starfield.hip)
    StarState star;                      // resident stars and frame runs (cg_starfield.hip)
    DevBuf iscratch;                     // JPEG decode (cg_image.hip)
    // JPEG encode (cg_jpeg_enc.hip): the coefficients, interval lengths, offsets and staged intervals
    // of up to 8 frames; the host-memory form's uploaded frame, file slot and length
    DevBuf jpeg_enc, jpeg_enc_io;
    // cg_rt_render_sequence_jpeg, cg_rast_draw_sequence_jpeg (JpegDelivery below): per slot set a
    // chunk's lengths and file slots, the slot of a frame encoded again alone, the lengths' pinned
    // host copy, and the events of the copies on `xfer`
    DevBuf jpeg_out[2], jpeg_big;
    PinnedBuf jpeg_len_host;
    Event jpeg_rdone[2], jpeg_cdone[2];
    // PNG encode (cg_png_enc.hip): the filtered rows, band lengths, Adler sums, offsets and staged bands
    // of up to 8 frames; the host-memory form's uploaded frame, file slot and length
    DevBuf png_enc, png_enc_io;
    // EXR encode (cg_exr_enc.hip): the predicted bytes, chunk lengths, offsets and staged streams of up
    // to 8 frames; the host-memory form's uploaded frame, file slot and length
    DevBuf exr_enc, exr_enc_io;
    int n_room = -1, n_boxes = 0;
    int scene_tex = 0;                   // bit k: the uploaded room/boxes carry texture k
    // texture modes 1-3 (cg_rast_set_textures): device copies of the maps
    DevBuf tmarble, tnoise, twoven, twoven_ao, twoven_op, twoven_nrm, tgrill, tgrill_op, tgrill_nrm, rtexel;
    int tex_loaded = 0;                  // bit k: texture k renderable
    cg_ctx *tex_owner = nullptr;         // a lane reads its parent's maps
    // cg_rast_draw_frames_device: frames overlap on `lanes` (child contexts,
    // each with its own stream and scratch; scene copied device to device)
    static constexpr int kRastLanes = 8;
    // declared after the texture maps above: a lane reads its parent's and is destroyed first
    std::unique_ptr<cg_ctx> lanes[kRastLanes];
    Event lane_ev[kRastLanes];
    Event seq_ev[kRastLanes];   // cg_rast_draw_sequence_device: a lane's latest chain step
    Event start_ev;
    unsigned scene_gen = 0, lane_gen[kRastLanes] = {};
};

// cg_api_rt.hip's, called by cg_api_rt_host.hip too: a frame's RtFrame from the caller's arguments
// (lights uploaded on st), and its kernels enqueued on st
int fill_frame(cg_ctx *c, const cg_light *lights, int n_lights, const cg_rt_camera *cam, const cg_rt_shard *shard,
               hipStream_t st, RtFrame &F);
int rt_enqueue(cg_ctx *c, const RtFrame &Fin, void *d_out_v, hipStream_t st, int slot = 0);

// cg_api_rt_host.hip's, used by cg_api_rast.hip too: the compressed delivery of a frame sequence.
// Chunks of `ch` frames are rendered by the caller into device memory on the context's stream;
// encode(j, ..) enqueues chunk j's encoding into slot set j & 1 (a frame's slot is W * H bytes),
// deliver(j) waits for it, reads the chunk's lengths and copies exactly those bytes into `out` back
// to back on `xfer` -- called after chunk j + 1 is enqueued, it overlaps that chunk's render.  A
// frame that did not fit its slot is encoded again alone into a slot of cg_image_jpeg_bound.
// With `png` set the files are PNGs under `pprm` (cg_*_sequence_png): a frame's slot is
// cg_image_png_bound, so no file is encoded twice.  With `exr` set the chunk is CG_PIX_RGBA_F32
// pictures and the files are EXRs under `eprm` (cg_*_sequence_exr), in slots of cg_image_exr_bound.
// offsets[f] .. offsets[f + 1] is frame f's file; once a frame does not fit below `cap` nothing
// more is copied and the offsets count on, so offsets[n_frames] is the capacity needed.
struct JpegDelivery {
    cg_ctx *c;
    int W, H, n_frames, ch;
    cg_jpeg_params prm;
    uint8_t *out;
    size_t cap, *offsets;
    size_t slot_bytes = 0;
    bool full = false;                       // a frame did not fit: nothing more is copied
    const void *frames[2] = {};              // the slot sets' rendered chunks, for the frames encoded again
    size_t fstride[2] = {};
    bool png = false;
    cg_png_params pprm = {};
    bool exr = false;
    cg_exr_params eprm = {};
    int begin();
    int slot_wait(int j);                    // before chunk j >= 2 is rendered: chunk j - 2 is copied
    int encode(int j, const void *d_frames, size_t frame_stride);   // uint32 pixels; float4 ones with `exr`
    int deliver(int j);
    int finish();                            // waits for the copies; CG_E_CAPACITY if `out` was short
};
