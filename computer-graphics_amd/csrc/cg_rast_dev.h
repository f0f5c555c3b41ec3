// cg_rast_dev.h -- rasteriser structures and device helpers shared by the
// colour-mode-0 pipeline (cg_rast.hip), colour modes 1-2 (cg_rast_colour.hip)
// and the compact route for large scenes (cg_rast_big.hip).
// Reference: rasteriser/Source/skeleton.cpp.
#pragma once

#include <float.h>
#include <limits.h>

#include "cg_internal.h"

namespace cg {

// Texture maps on the device (cg_rast_set_textures): the BGR maps as
// cv::imread returns them, the opacity maps already gray + thresholded
// (skeleton.cpp:149-155), the marble normal noise as xyz floats (:158-170).
// A null pointer = not loaded.
struct RastTexMaps {
    const uint8_t *marble;                       // 2000 x 2000 x 3
    const float *marble_noise;                   // 2000 x 2000 x 3
    const uint8_t *woven, *woven_ao, *woven_op, *woven_nrm;   // 1024^2 x 3 (op: x 1)
    const uint8_t *grill, *grill_op, *grill_nrm;
};
constexpr int kTexN = 1024, kMarbleN = 2000;

struct RastArgs {
    int W, H, n;
    float focal;
    float light[3];
    float lp[3];            // lightPower
    float ind_first;        // indirectLightPowerPerArea at frame start
    int want_first;         // ind_first differs from the steady-state 0.2
    const cg_vec4 *d_light; // if set, the light comes from the device geometry
    // texture modes 1-3 (skeleton.cpp:588-645): only read by the TEX kernel variants
    int textured;           // some triangle may carry texture 1-3
    int use_inv;            // yaw != 0: findU/findV go through inverse(R) (:1761-1765)
    float cam[4];           // cameraPos
    float Rinv[16];         // glm::inverse(R), column-major
    RastTexMaps tx;
    int state16;            // colour mode 0: fill -> post state in 2 bytes per pixel (n < 32768)
    const cg_rtri *tris;    // the clipped triangles (normals for the shading)
};

struct RastHdr {
    int ylo, yhi;           // visible rows [ylo, yhi] (ylo > yhi: none)
    int fy, fx;             // first shadeable fragment (if want_first), fy = INT_MAX none
    unsigned t_sh;          // what the row records carry of the triangle: index | shadow volume << 31,
    int tex, index, pad;    // texture, object index
};

// One frame of cg_rast_draw_sequence_device as the pipeline sees it: where the
// frame's record lives, where the rand() call index comes from, and the
// generator's capacity and tables (cg_rast_colour.hip).
struct RastSeq {
    cg_rast_seq_frame *info;   // d_info + f; info[1] receives the next frame's start
    int first;                 // the call's first frame: it starts at `start`, not at info[0].rand_offset
    uint64_t start;
    long long cap;             // fragments the materialised stream holds
    uint32_t *tables;          // the context's generator tables for nb_cap chunks
    int nb_cap;
    uint32_t *win;             // the 61-word window of this frame's lane (null: the tables' own slot)
    // frames on several lanes: the frame's chain step waits for the previous frame's (wait_ev,
    // null for the first) and announces itself (done_ev); null on one stream
    hipEvent_t wait_ev, done_ev;
    int route;                 // the route of every frame of the call (ctx_rast_route with the call's colour frames)
};

// ---- routes (cg_rast_route): the dense pipeline of cg_rast.hip, the compact one of cg_rast_big.hip ----
constexpr int kRastDenseInputs = 4096;                                  // input triangles the dense Draw accepts
constexpr long long kRastDenseList = (long long)kGeomMaxLeaves * kRastDenseInputs;   // 131072: its list capacity
// Colour modes 1-2 on the dense route count fragments per list slot in LDS (rast_count_kernel 4 B,
// rast_fill_rand_kernel 8 B a slot): what gfx950's 160 KiB a workgroup holds.  A longer list in
// those modes takes the compact route.
constexpr long long kRastDenseColourList = 160 * 1024 / 8;              // 20480
constexpr long long kRastMaxInputs = 4194304;                           // cg_rast_set_scene's limit
// What cg_rast_scratch_info reports of the latest frame.  The dense route leaves its counts on
// the device (n_dev, count[H]); the compact route knows them on the host.
struct RastLast {
    int route = -1;                 // -1: no frame yet
    long long n = -1;               // clipped triangles (-1: read *n_dev)
    long long spans = 0;            // spans the setup stored (dense: not counted)
    long long recs = -1;            // row records (-1: sum of count[0 .. H))
    const int *n_dev = nullptr, *count = nullptr;
    int H = 0;
    hipStream_t st = nullptr;
};
struct RowRec;
// What the latest frame left in context scratch, for the buffers kernel (cg_rast_buffers.hip):
// the ordered z-buffer's state words and the row records they name.  Host bookkeeping only.
struct RastFrame {
    bool valid = false;
    int route = 0, mode = 0;
    RastArgs A;                          // as the fill saw them (state16: the form of `words`)
    const void *words = nullptr;         // record + 1 | shadow mark in the top bit, per pixel
    const float4 *direct = nullptr;      // colour modes 1-2: the colour fill's state
    const RowRec *recs = nullptr;
    const unsigned long long *row_off = nullptr;   // compact route; null: row y's records at y * A.n
    unsigned long long rec_cap = 0;
    // cg_rast_draw*: the clip's per-input counts and (compact route) their prefix; null: the
    // caller's list is the clipped list
    const int *counts = nullptr;
    const unsigned long long *pre = nullptr;
    int n_in = 0;
    hipStream_t st = nullptr;
};

// Ordered per-row records (one wave per screen row): for every triangle in
// order whose span on this row has a fragment on screen, a 48-byte record
// with everything the fill needs -- no dependent loads in the fill loop (the
// shading reads the normal from the triangle, A.tris).
struct alignas(16) RowRec {
    int lx, rx;
    float lz, sz, lX, sX, lY, sY;
    unsigned t_sh;           // triangle index | shadow-volume triangle (colour.x < 0) << 31
    int first_x;             // x of the frame's first shaded fragment on this row, else -1
    int tex, index;          // the triangle's texture (0-3) and object index (findU/findV)
};
static_assert(sizeof(RowRec) == 48, "RowRec");
__device__ __forceinline__ int rec_t(const RowRec &r) { return (int)(r.t_sh & 0x7fffffffu); }
__device__ __forceinline__ int rec_shadow(const RowRec &r) { return (int)(r.t_sh >> 31); }

// calculateIllumination's direct term D (:674-683); the post-pass rebuilds
// screen/low/high = colour * (D + indirect) from it with the same ops.
__device__ __forceinline__ vec3 illum_D(const RastArgs &A, float zinv, float X, float Y, vec3 N)
{
    // Interpolate pos3d (:546-548)
    float pz = 1 / zinv;
    float px = X / zinv;
    float py = Y / zinv;
    vec3 r = v3(A.light[0] - px, A.light[1] - py, A.light[2] - pz);               // :675
    double a = (double)r.x * (double)r.x, b = (double)r.y * (double)r.y,
           c = (double)r.z * (double)r.z;
    float r2 = (float)((a + b) + c);                                              // :677
    float vp = dot(r, N);                                                         // :681
    float m = gmax(vp, 0.0f);
    float area = (float)((double)4.0f * M_PI * (double)r2);                       // :682
    return v3((A.lp[0] * m) / area, (A.lp[1] * m) / area, (A.lp[2] * m) / area);
}

// findU / findV (skeleton.cpp:1756-1825) for a fragment with zinv and the
// interpolated pos3d numerators Xn, Yn (:546-548, the same ops as illum_D):
// texel row u, column v of a size x size map.  A negative remainder (the
// reference indexes the Mat out of bounds) wraps to [0, size).
__device__ __forceinline__ void rast_find_uv(const RastArgs &A, int index, int size, float zinv, float Xn, float Yn,
                                             int &u, int &v)
{
    float pz = 1 / zinv;
    float px = Xn / zinv;
    float py = Yn / zinv;
    float ox, oy, oz;
    if (A.use_inv) {   // inverse(R) * pos3d (w = 1), type_mat4x4.inl:615-661, then + cameraPos
        float r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float a0 = A.Rinv[k] * px, a1 = A.Rinv[4 + k] * py;
            float a2 = A.Rinv[8 + k] * pz, a3 = A.Rinv[12 + k] * 1.0f;
            r[k] = (a0 + a1) + (a2 + a3);
        }
        ox = r[0] + A.cam[0]; oy = r[1] + A.cam[1]; oz = r[2] + A.cam[2];
    } else {
        ox = px + A.cam[0]; oy = py + A.cam[1]; oz = pz + A.cam[2];
    }
    const float nh = (float)(-size / 2), h = (float)(size / 2);
    float fu = 0.0f, fv = 0.0f;
    switch (index) {
    case 3: fu = (nh * oy) + h; fv = (h * oz) + h; break;
    case 1: fu = (nh * ox) + h; fv = (nh * oz) + h; break;
    case 4: fu = (nh * oy) + h; fv = (nh * oz) + h; break;
    case 2: fu = (nh * ox) + h; fv = (nh * oz) + h; break;
    case 0: fu = (nh * ox) + h; fv = (nh * oy) + h; break;
    default: break;
    }
    int iu = 0, iv = 0;
    if (index >= 0 && index <= 4) {
        iu = f2i_x86(fu);
        iv = f2i_x86(fv);
    }
    iu %= size;
    iv %= size;
    u = iu < 0 ? iu + size : iu;
    v = iv < 0 ? iv + size : iv;
}

// Opacity test of textures 2 and 3 (:602, :624); textures 0-1 always shade.
// Whether texture tex's maps are on the device.  The host entries refuse a
// list with a texture whose maps are missing; a device list is not inspected
// (cg_rast_render_device), so the kernels never read a missing map: such a
// fragment shades as texture 0.
__device__ __forceinline__ bool rast_tex_present(const RastArgs &A, int tex)
{
    if (tex == 1) return A.tx.marble && A.tx.marble_noise;
    if (tex == 2) return A.tx.grill && A.tx.grill_op && A.tx.grill_nrm;
    if (tex == 3) return A.tx.woven && A.tx.woven_ao && A.tx.woven_op && A.tx.woven_nrm;
    return false;
}

__device__ __forceinline__ bool rast_opaque(const RastArgs &A, int tex, int index, float zinv, float Xn, float Yn)
{
    if ((tex != 2 && tex != 3) || !rast_tex_present(A, tex)) return true;
    int u, v;
    rast_find_uv(A, index, kTexN, zinv, Xn, Yn, u, v);
    return (tex == 2 ? A.tx.grill_op : A.tx.woven_op)[(size_t)u * kTexN + v] == 255;
}

// What a shading fragment of texture tex >= 1 reads (:588-645), for an opaque
// one: the normal calculateIllumination takes and the texel word
// B | G << 8 | R << 16 | occlusion << 24 (texture 3; textureColour and
// occlusion are rebuilt from the bytes as the reference forms them).
__device__ __forceinline__ vec3 rast_tex_normal(const RastArgs &A, int tex, int index, float zinv, float Xn, float Yn,
                                                int x, int y, vec3 Ntri, uint32_t &texel)
{
    int u, v;
    if (tex == 1) {
        rast_find_uv(A, index, kMarbleN, zinv, Xn, Yn, u, v);
        const uint8_t *m = A.tx.marble + 3 * ((size_t)u * kMarbleN + v);
        texel = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16);
        const float *nz = A.tx.marble_noise + 3 * ((size_t)y * kMarbleN + x);   // normalMap_marble[p.y*rows + p.x]
        return v3(Ntri.x + nz[0], Ntri.y + nz[1], Ntri.z + nz[2]);              // currentNormal + noise (w + 0)
    }
    rast_find_uv(A, index, kTexN, zinv, Xn, Yn, u, v);
    const size_t k = (size_t)u * kTexN + v;
    const uint8_t *nm = (tex == 2 ? A.tx.grill_nrm : A.tx.woven_nrm) + 3 * k;
    const uint8_t *cm = (tex == 2 ? A.tx.grill : A.tx.woven) + 3 * k;
    const uint32_t occ = tex == 3 ? A.tx.woven_ao[(size_t)u * 3 * kTexN + v] : 0u;   // at<uchar> on the BGR Mat
    texel = (uint32_t)cm[0] | ((uint32_t)cm[1] << 8) | ((uint32_t)cm[2] << 16) | (occ << 24);
    // normalize(vec4(valx, valy, valz, 1)) (:607-609, :631-634): v * (1 / sqrt(dot4))
    const float vx = (float)nm[0] / 255.0f, vy = (float)nm[1] / 255.0f, vz = (float)nm[2] / 255.0f, vw = 1.0f;
    const float d4 = ((vx * vx) + (vy * vy)) + ((vz * vz) + (vw * vw));
    const float inv = 1.0f / sqrtf(d4);
    return v3(vx * inv, vy * inv, vz * inv);
}

// LO + rand() / (RAND_MAX/HI - LO), all float (skeleton.cpp:563-565, :649-651)
__device__ __forceinline__ float rand_unit(int32_t v)
{
    const float LO = 0.2f, HI = 0.5f;
    const float den = (float)2147483647 / HI - LO;        // RAND_MAX / HI - LO
    return LO + (float)v / den;
}

__device__ __forceinline__ RastArgs with_device_light(RastArgs A)
{
    if (A.d_light) {                                      // light from the device geometry (:223)
        const cg_vec4 L = *A.d_light;
        A.light[0] = L.x; A.light[1] = L.y; A.light[2] = L.z;
    }
    return A;
}

// Shade state bit: the pixel's screen colour is stored directly in .yzw
// (colour modes 1-2; low/high buffers stay cleared), instead of a triangle
// index whose colour the post-pass multiplies by (D + k).
constexpr int kStateDirect = 1 << 29;

// ---- shared by the dense pipeline (cg_rast.hip) and the compact route (cg_rast_big.hip) ----
constexpr int kSetupThreads = 256;
constexpr int kRastMaxRows = 4096;   // LDS rows per triangle in span setup (H <= 4096)

// Workgroups are dispatched round-robin over the 8 XCDs, each with its own L2.
// The row-ordered kernels renumber them so that each group of kXcdRows rows
// is handled by one XCD (a row's records are then fetched into one L2, not
// all eight), with the groups dealt round-robin to keep the XCDs balanced
// (row cost varies a lot over the frame).  A kernel whose row group is
// `per_group` workgroups wide launches xcd_grid(H, per_group) of them.
constexpr int kXcds = 8, kXcdRows = 8;
__host__ __device__ constexpr int xcd_grid(int H, int per_group)
{
    return kXcds * ((((H + kXcdRows - 1) / kXcdRows) + kXcds - 1) / kXcds) * per_group;
}
// -> row group of this workgroup (-1: idle padding) and its index m within the group
__device__ __forceinline__ int xcd_group(int H, int per_group, int &m)
{
    const int k = (int)(blockIdx.x % kXcds), l = (int)(blockIdx.x / kXcds);
    m = l % per_group;
    const int g = k + kXcds * (l / per_group);
    return g < (H + kXcdRows - 1) / kXcdRows ? g : -1;
}

struct Pix {                // rasteriser Pixel (:88-94) minus w
    int x, y;
    float zinv, X, Y;
};

__device__ __forceinline__ Pix vertex_shader(const RastArgs &A, cg_vec4 v)
{
    // :512-521
    float x = (A.focal * (v.x / v.z)) + (float)(A.W / 2);
    float y = (A.focal * (v.y / v.z)) + (float)(A.H / 2);
    Pix p;
    p.x = f2i_x86(x);
    p.y = f2i_x86(y);
    p.zinv = 1 / v.z;
    p.X = v.x;
    p.Y = v.y;
    return p;
}

// Interpolate (:524-551) prepared for one edge a -> b with N samples.
struct Edge {
    float ax, ay, az, aX, aY;     // a.x, a.y as float; a.zinv; a.pos3d.xy * a.zinv
    float stx, sty, stz, sX, sY;
    int n;
};

__device__ __forceinline__ Edge make_edge(Pix a, Pix b)
{
    Edge e;
    float aX = a.X * a.zinv, aY = a.Y * a.zinv;   // :526-527
    float bX = b.X * b.zinv, bY = b.Y * b.zinv;   // :529-530
    int dx = a.x - b.x, dy = a.y - b.y;
    dx = dx < 0 ? -dx : dx;
    dy = dy < 0 ? -dy : dy;
    e.n = (dx > dy ? dx : dy) + 1;                // :473-475
    float den = (float)(e.n - 1 > 1 ? e.n - 1 : 1);
    e.ax = (float)a.x;
    e.ay = (float)a.y;
    e.az = a.zinv;
    e.aX = aX;
    e.aY = aY;
    e.stx = (float)(b.x - a.x) / den;             // :533-538
    e.sty = (float)(b.y - a.y) / den;
    e.stz = (b.zinv - a.zinv) / den;
    e.sX = (bX - aX) / den;
    e.sY = (bY - aY) / den;
    return e;
}

__device__ __forceinline__ int edge_x(const Edge &e, int j) { return f2i_x86(floorf(e.ax + (e.stx * (float)j))); }
__device__ __forceinline__ int edge_y(const Edge &e, int j) { return f2i_x86(floorf(e.ay + (e.sty * (float)j))); }

// sample j's zinv and pos3d.xy (:543-548)
__device__ __forceinline__ void edge_attr(const Edge &e, int j, float &zinv, float &X, float &Y)
{
    float fj = (float)j;
    zinv = e.az + (e.stz * fj);
    X = (e.aX + (e.sX * fj)) / zinv;
    Y = (e.aY + (e.sY * fj)) / zinv;
}

__device__ __forceinline__ unsigned long long key_left(int x, unsigned seq)
{
    return ((unsigned long long)((unsigned)x ^ 0x80000000u) << 32) | (unsigned long long)(~seq);
}
__device__ __forceinline__ unsigned long long key_right(int x, unsigned seq)
{
    return ((unsigned long long)((unsigned)x ^ 0x80000000u) << 32) | (unsigned long long)seq;
}

// Colour mode 0: fill -> post state, 4 bytes per pixel: 1 + the row record of
// the last shading fragment (0 none) | the shadow mark << 31; 2 bytes (the
// mark in bit 15) when a row holds fewer than 32768 records (A.state16).  The post-pass
// rebuilds that fragment from the record -- zinv = lz + sz * i (:543) and the
// pos3d numerators with the same float ops, the normal, the texels -- and
// evaluates calculateIllumination there, so the fill keeps only what its
// ordered walk decides.
constexpr uint32_t kStShadow = 0x80000000u;

// One wave per kFillPx-pixel row segment, one pixel per lane, state in
// registers; records walked in triangle order (the reference's ordered
// z-buffer), one uniform overlap test per record.
constexpr int kFillPx = 64;   // pixels per wave; 128 / 256 measured 3 % / 10 % slower (C3, round 1)

// cg_rast_span_segments: the fill segments that the visible extent [max(lx, 0), min(rx, W)) of a
// span overlaps -- their number (0: no fragment on screen) and the first one.
__host__ __device__ inline int rast_span_segments(int lx, int rx, int W, int *first)
{
    const int a = lx > 0 ? lx : 0, b = rx < W ? rx : W;
    *first = a / kFillPx;
    return b > a ? (b - 1) / kFillPx - a / kFillPx + 1 : 0;
}

// shade buffers of one pixel as they stand after the fill (:580-585), from its
// state and its triangle's colour
__device__ __forceinline__ void shade3c(const RastArgs &A, float4 st, cg_vec3 col, vec3 &sc, vec3 &lo, vec3 &hi,
                                        int tex = 0, uint32_t texel = 0u)
{
    const int tb = __float_as_int(st.x);
    if (tb < 0) {
        sc = lo = hi = v3(0.f, 0.f, 0.f);
        return;
    }
    if (tb & kStateDirect) {                               // colour modes 1-2 (:652, :660)
        sc = v3(st.y, st.z, st.w);
        lo = hi = v3(0.f, 0.f, 0.f);                       // cleared buffers (:250-257)
        return;
    }
    const float ind = (tb & (1 << 30)) ? A.ind_first : 0.2f * 1;
    const vec3 D = v3(st.y, st.z, st.w);
    if (tex != 0) {
        // textureColour (:590, :611, :636) and, texture 3, the occlusion (:626-627)
        const vec3 c = v3((float)((texel >> 16) & 255u) / 255.0f, (float)((texel >> 8) & 255u) / 255.0f,
                          (float)(texel & 255u) / 255.0f);
        if (tex == 3) {
            float occ = (float)(texel >> 24);
            occ /= 255.0f;
            sc = c * ((D + v3(ind, ind, ind)) * occ);                                // :638
            lo = c * ((D + v3(0.0f * 1, 0.0f * 1, 0.0f * 1)) * occ);                 // :640
            hi = c * ((D + v3(0.4f * 1, 0.4f * 1, 0.4f * 1)) * occ);                 // :642
        } else {
            sc = c * (D + v3(ind, ind, ind));
            lo = c * (D + v3(0.0f * 1, 0.0f * 1, 0.0f * 1));
            hi = c * (D + v3(0.4f * 1, 0.4f * 1, 0.4f * 1));
        }
        return;
    }
    const vec3 c = v3(col.x, col.y, col.z);
    sc = c * (D + v3(ind, ind, ind));                      // :580
    lo = c * (D + v3(0.0f * 1, 0.0f * 1, 0.0f * 1));       // :582
    hi = c * (D + v3(0.4f * 1, 0.4f * 1, 0.4f * 1));       // :584
}

// soft-shadow darkening amount of a pixel whose 3x3 shadow neighbourhood is
// sh[cy-1..cy+1][cx-1..cx+1] (row stride ld), 0 if not shadowed
// (:286-303, :1725-1733; [y+1][x-1] counted twice, [y+1][x+1] omitted)
// (sh: the marks as ints, or the post state words with the mark in bit 31)
template <class T>
__device__ __forceinline__ float darken_at(const T *sh, int ld, int cy, int cx)
{
    const T *p = sh + cy * ld + cx;
    auto c = [&](int o) { return sizeof(T) == 4 && (T)-1 > (T)0 ? (int)((uint32_t)p[o] >> 31) : (int)p[o]; };
    if (c(0) != 1) return 0.0f;
    int k = c(0) + c(-ld) + c(-ld - 1) + c(-ld + 1) + c(ld - 1) + c(ld) + c(ld - 1) + c(-1) + c(1);
    float val = div_const((float)k, 9.0f, 1.0f / 9.0f);                 // val /= 9.0f
    if ((double)val < 0.6) return 0.05f;
    if ((double)val < 0.7) return 0.08f;
    if ((double)val < 0.8) return 0.1f;
    if ((double)val < 0.9) return 0.12f;
    return 0.3f;
}

// Post-pass tile (rast_post_kernel): 64x8 pixels, shade halo 1, shadow halo 2.
constexpr int kPostTW = 64, kPostTH = 8;
constexpr int kPostHW = kPostTW + 2, kPostHH = kPostTH + 2;      // shade halo 1
constexpr int kPostSW = kPostTW + 4, kPostSH = kPostTH + 4;      // shadow halo 2

}  // namespace cg
