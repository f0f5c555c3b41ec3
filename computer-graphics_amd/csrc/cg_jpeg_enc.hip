// cg_jpeg_enc.hip -- the baseline JPEG encoder: the host-only restatement
// (cg_image_encode_jpeg_host, cg_image_jpeg_header, cg_image_jpeg_bound) and the device encoder
// (cg_image_encode_jpeg_device, cg_image_encode_jpeg).  The arithmetic is cg_jpeg_enc.h's, the
// contract include/cg_render.h's: the bytes are those Pillow over libjpeg-turbo writes with
// restart_marker_rows = 1.
//
// The device encoder is four kernels a chunk of up to 8 frames:
//   jpeg_enc_transform_kernel  8 lanes a block: colour conversion, the chroma mean, both FDCT
//                              passes through LDS, quantisation; int16 coefficients in zig-zag
//                              order, blocks in scan order
//   jpeg_enc_entropy_kernel    one workgroup per (frame, restart interval): a lane sizes a block,
//                              a workgroup scan gives its bit offset, the lanes deposit their codes
//                              into a window of the interval's bit string in LDS, full windows are
//                              byte-stuffed and flushed to the interval's staging area
//   jpeg_enc_scan_kernel       a frame's interval lengths to offsets, its length into d_bytes
//   jpeg_enc_gather_kernel     header, intervals, RST markers and EOI into the frame's slot
// A DC predictor is the stored DC of the previous block of the component, so nothing in a frame
// is serial beyond one interval's scans.
#include <algorithm>
#include <cstring>

#include "cg_host.h"
#include "cg_jpeg_enc.h"

namespace {

using namespace cg;

constexpr JpegHuff kHuff = jpeg_make_huff();
__constant__ JpegHuff d_jpeg_huff = jpeg_make_huff();

// zig-zag position of a row-major index
struct JpegZpos {
    uint8_t p[64];
};
constexpr JpegZpos jpeg_make_zpos()
{
    JpegZpos z{};
    for (int k = 0; k < 64; ++k) z.p[kJpegZigzag[k]] = (uint8_t)k;
    return z;
}
__constant__ JpegZpos d_jpeg_zpos = jpeg_make_zpos();

// 8 q per table entry, row-major: table 0 luminance, 1 chrominance
struct JpegQuant {
    uint16_t q8[2][64];
};
struct JpegHeader {
    uint8_t b[kJpegHeaderBytes + 3];
};

bool params_ok(int w, int h, const cg_jpeg_params *p)
{
    return p && w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && p->quality >= 1 && p->quality <= 100 &&
           (p->subsampling == CG_JPEG_444 || p->subsampling == CG_JPEG_420);
}

JpegQuant make_quant(int quality)
{
    JpegQuant q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q.q8[t][i] = (uint16_t)(8 * jpeg_quant(kJpegBaseQ[t][i], quality));
    return q;
}

// SOI .. SOS: exactly kJpegHeaderBytes
void write_header(const JpegShape &s, const JpegQuant &q, uint8_t *out)
{
    uint8_t *o = out;
    auto put = [&](std::initializer_list<int> v) {
        for (int x : v) *o++ = (uint8_t)x;
    };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 0x4A, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01,
         0x00, 0x00});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xDB, 0x00, 0x43, t});
        for (int k = 0; k < 64; ++k) *o++ = (uint8_t)(q.q8[t][kJpegZigzag[k]] >> 3);
    }
    put({0xFF, 0xC0, 0x00, 0x11, 0x08, s.h >> 8, s.h & 255, s.w >> 8, s.w & 255, 0x03, 0x01,
         s.sub == CG_JPEG_420 ? 0x22 : 0x11, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xC4, 0x00, 0x1F, t});
        for (int i = 0; i < 16; ++i) *o++ = kJpegDcBits[t][i];
        for (int i = 0; i < 12; ++i) *o++ = (uint8_t)i;
        put({0xFF, 0xC4, 0x00, 0xB5, 0x10 | t});
        for (int i = 0; i < 16; ++i) *o++ = kJpegAcBits[t][i];
        for (int i = 0; i < 162; ++i) *o++ = kJpegAcVals[t][i];
    }
    put({0xFF, 0xDD, 0x00, 0x04, s.mx >> 8, s.mx & 255});
    put({0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00});
}

// The longest code of one block.  DC: a code of at most 11 bits (the chrominance table's longest
// of its 12) and 11 value bits, 22.  AC: a coefficient other than zero costs at most a 16-bit
// code and 10 value bits, 26; a zero costs nothing by itself, the ZRL that 16 of them may need is
// 11 bits for what 16 coefficients would have cost 416, and an EOB (at most 4 bits) is only sent
// when the last coefficient is zero and so saves 26.  63 * 26 + 22 = 1660 bits.
static_assert(kJpegMaxBlockBits == 63 * 26 + 22, "block bound");
// An interval of nb blocks: its bits rounded up to a byte, and every byte may be FF and get a
// stuffed 00 after it.
size_t interval_bound(size_t nb) { return 2 * ((nb * kJpegMaxBlockBits + 7) / 8); }
// The file: header, MY intervals, an RST marker before all but the first, EOI.
size_t file_bound(const JpegShape &s)
{
    return kJpegHeaderBytes + (size_t)s.my * interval_bound((size_t)s.mx * s.bpm) + 2 * (size_t)(s.my - 1) + 2;
}

// one block's 64 quantised coefficients in zig-zag order, on the host
void host_block(const uint32_t *px, size_t stride, const JpegShape &s, const JpegQuant &q, int mcu_x, int mcu_y, int k,
                int16_t zz[64])
{
    int comp, bx, by, d[64];
    bool dummy;
    jpeg_block_source(s, mcu_x, mcu_y, k, &comp, &bx, &by, &dummy);
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) d[r * 8 + c] = jpeg_sample(px, stride, s, comp, bx * 8 + c, by * 8 + r) - 128;
    for (int r = 0; r < 8; ++r) {
        int *v = d + r * 8;
        jpeg_fdct8<true>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    }
    for (int c = 0; c < 8; ++c) {
        int *v = d + c;
        jpeg_fdct8<false>(v[0], v[8], v[16], v[24], v[32], v[40], v[48], v[56]);
    }
    for (int j = 0; j < 64; ++j) {
        const int i = kJpegZigzag[j];
        zz[j] = (int16_t)(dummy && j ? 0 : jpeg_quantise(d[i], q.q8[comp ? 1 : 0][i]));
    }
}

// a byte sink that counts past its capacity without writing there
struct HostBits {
    uint8_t *out;
    size_t cap, n = 0;
    uint32_t acc = 0;
    int fill = 0;
    void byte(int b)
    {
        if (n < cap) out[n] = (uint8_t)b;
        ++n;
    }
    void put(uint32_t bits, int len)
    {
        for (int i = len - 1; i >= 0; --i) {
            acc = (acc << 1) | ((bits >> i) & 1u);
            if (++fill == 8) {
                byte((int)acc);
                if (acc == 0xFFu) byte(0);
                acc = 0, fill = 0;
            }
        }
    }
    void pad()
    {
        if (fill) put((1u << (8 - fill)) - 1u, 8 - fill);
    }
};

// ---- kernels --------------------------------------------------------------------------------

constexpr int kEncThreads = 256;
constexpr int kEncXfBlocks = kEncThreads / 8;        // blocks a transform workgroup takes
constexpr int kEncStageBytes = 16384;                // an entropy workgroup's window of its interval
constexpr int kEncStageWords = kEncStageBytes / 4;
constexpr int kEncStageBits = kEncStageBytes * 8;
constexpr int kEncChunkFrames = 8;                   // frames the context's scratch holds

// Exclusive sum of v over the workgroup (kEncThreads lanes, wave 64), *total the whole sum.
// Ends with a barrier: wsum may be reused at once.
__device__ __forceinline__ uint32_t enc_scan(uint32_t v, uint32_t *total, uint32_t *wsum, int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kEncThreads / 64; ++i) {
        const uint32_t w = wsum[i];
        base += i < wv ? w : 0u;
        tot += w;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// Blocks in scan order, 8 lanes each: lane r of a block transforms row r, then column r.
__global__ __launch_bounds__(kEncThreads) void jpeg_enc_transform_kernel(const uint32_t *__restrict__ argb,
                                                                        size_t frame_stride, JpegShape s, JpegQuant q,
                                                                        int16_t *__restrict__ coef, unsigned n_blocks)
{
    // a block's 8 x 8 ints at pitch 9 and 73 a block: row r's stores and column c's loads of the 8
    // lanes of a block fall into different banks
    __shared__ int tile[kEncXfBlocks * 73];
    __shared__ __align__(16) int16_t zz[kEncXfBlocks * 64];
    __shared__ uint16_t q8[128];
    __shared__ uint8_t zpos[64];
    const int tid = (int)threadIdx.x;
    if (tid < 128) q8[tid] = q.q8[tid >> 6][tid & 63];
    if (tid < 64) zpos[tid] = d_jpeg_zpos.p[tid];
    const int blk = tid >> 3, r = tid & 7;
    const unsigned g0 = blockIdx.x * (unsigned)kEncXfBlocks, g = g0 + (unsigned)blk;
    const bool have = g < n_blocks;
    const uint32_t *px = argb + (size_t)blockIdx.y * frame_stride;
    int comp = 0;
    bool dummy = false;
    int *t = tile + blk * 73;
    if (have) {
        const unsigned mcu = g / (unsigned)s.bpm;
        const int k = (int)(g - mcu * (unsigned)s.bpm);
        const int mcu_y = (int)(mcu / (unsigned)s.mx), mcu_x = (int)(mcu - (unsigned)mcu_y * (unsigned)s.mx);
        int bx, by;
        jpeg_block_source(s, mcu_x, mcu_y, k, &comp, &bx, &by, &dummy);
        const int x = bx * 8, y = by * 8 + r;
        int d0 = jpeg_sample(px, (size_t)s.w, s, comp, x + 0, y) - 128;
        int d1 = jpeg_sample(px, (size_t)s.w, s, comp, x + 1, y) - 128;
        int d2 = jpeg_sample(px, (size_t)s.w, s, comp, x + 2, y) - 128;
        int d3 = jpeg_sample(px, (size_t)s.w, s, comp, x + 3, y) - 128;
        int d4 = jpeg_sample(px, (size_t)s.w, s, comp, x + 4, y) - 128;
        int d5 = jpeg_sample(px, (size_t)s.w, s, comp, x + 5, y) - 128;
        int d6 = jpeg_sample(px, (size_t)s.w, s, comp, x + 6, y) - 128;
        int d7 = jpeg_sample(px, (size_t)s.w, s, comp, x + 7, y) - 128;
        jpeg_fdct8<true>(d0, d1, d2, d3, d4, d5, d6, d7);
        int *row = t + r * 9;
        row[0] = d0, row[1] = d1, row[2] = d2, row[3] = d3, row[4] = d4, row[5] = d5, row[6] = d6, row[7] = d7;
    }
    __syncthreads();
    if (have) {
        const int c = r;
        int d0 = t[0 * 9 + c], d1 = t[1 * 9 + c], d2 = t[2 * 9 + c], d3 = t[3 * 9 + c];
        int d4 = t[4 * 9 + c], d5 = t[5 * 9 + c], d6 = t[6 * 9 + c], d7 = t[7 * 9 + c];
        jpeg_fdct8<false>(d0, d1, d2, d3, d4, d5, d6, d7);
        const uint16_t *qt = q8 + (comp ? 64 : 0);
        int16_t *z = zz + blk * 64;
        const bool ac0 = dummy;   // a dummy block keeps its source's quantised DC alone
        z[zpos[0 * 8 + c]] = (int16_t)(ac0 && c ? 0 : jpeg_quantise(d0, qt[0 * 8 + c]));
        z[zpos[1 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d1, qt[1 * 8 + c]));
        z[zpos[2 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d2, qt[2 * 8 + c]));
        z[zpos[3 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d3, qt[3 * 8 + c]));
        z[zpos[4 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d4, qt[4 * 8 + c]));
        z[zpos[5 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d5, qt[5 * 8 + c]));
        z[zpos[6 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d6, qt[6 * 8 + c]));
        z[zpos[7 * 8 + c]] = (int16_t)(ac0 ? 0 : jpeg_quantise(d7, qt[7 * 8 + c]));
    }
    __syncthreads();
    // the workgroup's blocks are contiguous: 16 bytes a lane
    const unsigned here = n_blocks - g0 < (unsigned)kEncXfBlocks ? n_blocks - g0 : (unsigned)kEncXfBlocks;
    if ((unsigned)tid * 8u < here * 64u) {
        uint4 *dst = (uint4 *)(coef + ((size_t)blockIdx.y * n_blocks + g0) * 64);
        dst[tid] = ((const uint4 *)zz)[tid];
    }
}

// `bits` (len of them, len <= 26) at bit p of the interval, into the window that starts at bit
// win0: the parts that fall outside the window are another round's
__device__ __forceinline__ void enc_deposit(uint32_t *win, int win0, int p, uint32_t bits, int len)
{
    const int rp = p - win0;
    const int wi = rp >> 5, sh = rp & 31;
    const unsigned long long v = (unsigned long long)bits << (64 - len - sh);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (hi && wi >= 0 && wi < kEncStageWords) atomicOr(&win[wi], hi);
    if (lo && wi + 1 >= 0 && wi + 1 < kEncStageWords) atomicOr(&win[wi + 1], lo);
}

// The first nbytes of the window to out[*outpos ..], a 00 after every FF; nothing at or past cap
// is written, and *outpos counts on regardless.  1024 bytes a pass, a word a lane.
__device__ __forceinline__ void enc_flush(const uint32_t *win, int nbytes, uint8_t *__restrict__ out, size_t cap,
                                          uint32_t *outpos, uint32_t *wsum, int tid)
{
    for (int base = 0; base < nbytes; base += 4 * kEncThreads) {
        const int at = base + 4 * tid;
        int n = nbytes - at;
        n = n < 0 ? 0 : n > 4 ? 4 : n;
        const uint32_t wd = n ? win[at >> 2] : 0u;
        uint32_t ff = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) ff += (j < n && ((wd >> (24 - 8 * j)) & 255u) == 255u) ? 1u : 0u;
        uint32_t tot;
        const uint32_t ex = enc_scan(ff, &tot, wsum, tid);
        size_t p = (size_t)*outpos + (size_t)(4 * tid) + ex;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                const uint32_t b = (wd >> (24 - 8 * j)) & 255u;
                if (p < cap) out[p] = (uint8_t)b;
                ++p;
                if (b == 255u) {
                    if (p < cap) out[p] = 0;
                    ++p;
                }
            }
        const int chunk = nbytes - base < 4 * kEncThreads ? nbytes - base : 4 * kEncThreads;
        *outpos += (uint32_t)chunk + tot;
    }
}

// One workgroup per (restart interval, frame).  Rounds of kEncThreads blocks; the window of
// kEncStageBytes moves along the interval's bit string as it fills, whatever the round.
__global__ __launch_bounds__(kEncThreads) void jpeg_enc_entropy_kernel(const int16_t *__restrict__ coef, JpegShape s,
                                                                      unsigned n_blocks, uint8_t *__restrict__ stage,
                                                                      size_t stage_cap, uint32_t *__restrict__ lens)
{
    __shared__ uint32_t win[kEncStageWords];
    __shared__ JpegHuff hf;
    __shared__ uint32_t wsum[kEncThreads / 64];
    const int tid = (int)threadIdx.x;
    const int interval = (int)blockIdx.x, f = (int)blockIdx.y;
    {
        uint32_t *dst = (uint32_t *)&hf;
        const uint32_t *src = (const uint32_t *)&d_jpeg_huff;
        for (int i = tid; i < (int)(sizeof(JpegHuff) / 4); i += kEncThreads) dst[i] = src[i];
    }
    for (int i = tid; i < kEncStageWords; i += kEncThreads) win[i] = 0u;
    const int nb = s.mx * s.bpm;
    const int16_t *ic = coef + ((size_t)f * n_blocks + (size_t)interval * (size_t)nb) * 64;
    uint8_t *out = stage + ((size_t)f * (size_t)s.my + (size_t)interval) * stage_cap;
    int win0 = 0, carry = 0;   // bits: where the window starts, where the round's first block does
    uint32_t outpos = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += kEncThreads) {
        const int b = b0 + tid;
        const bool have = b < nb;
        int len = 0, pred = 0, tab = 0;
        const int16_t *zz = ic + (size_t)b * 64;
        if (have) {
            const int k = b % s.bpm;
            tab = (s.sub == CG_JPEG_420 ? k >= 4 : k >= 1) ? 1 : 0;
            const int pb = jpeg_pred_block(s, b);
            pred = pb < 0 ? 0 : (int)ic[(size_t)pb * 64];
            jpeg_code_block(hf, tab, pred, [&](int j) { return (int)zz[j]; }, [&](uint32_t, int l) { len += l; });
        }
        uint32_t tot;
        const int off = carry + (int)enc_scan((uint32_t)len, &tot, wsum, tid);
        const int total = carry + (int)tot;
        for (;;) {
            if (have && off < win0 + kEncStageBits && off + len > win0) {
                int p = off;
                jpeg_code_block(hf, tab, pred, [&](int j) { return (int)zz[j]; }, [&](uint32_t bits, int l) {
                    enc_deposit(win, win0, p, bits, l);
                    p += l;
                });
            }
            __syncthreads();
            if (total - win0 < kEncStageBits) break;
            enc_flush(win, kEncStageBytes, out, stage_cap, &outpos, wsum, tid);
            for (int i = tid; i < kEncStageWords; i += kEncThreads) win[i] = 0u;
            win0 += kEncStageBits;
            __syncthreads();
        }
        carry = total;
    }
    // the last byte's 1-bits, and what is left of the window
    if (tid == 0 && (carry & 7)) enc_deposit(win, win0, carry, (1u << (8 - (carry & 7))) - 1u, 8 - (carry & 7));
    __syncthreads();
    enc_flush(win, (carry - win0 + 7) >> 3, out, stage_cap, &outpos, wsum, tid);
    if (tid == 0) lens[(size_t)f * (size_t)s.my + (size_t)interval] = outpos;
}

// One workgroup a frame: offs[i] = the bytes of intervals 0 .. i - 1; d_bytes = the file's length,
// or CG_E_CAPACITY when the slot is shorter.
__global__ __launch_bounds__(kEncThreads) void jpeg_enc_scan_kernel(const uint32_t *__restrict__ lens, int my,
                                                                   size_t slot_bytes,
                                                                   unsigned long long *__restrict__ offs,
                                                                   int64_t *__restrict__ d_bytes)
{
    __shared__ uint32_t wsum[kEncThreads / 64];
    const int tid = (int)threadIdx.x;
    const size_t f = blockIdx.x;
    unsigned long long carry = 0;
    for (int i0 = 0; i0 < my; i0 += kEncThreads) {
        const int i = i0 + tid;
        // 256 intervals of at most 10.2 MB (24576 blocks): the sum fits 32 bits
        const uint32_t v = i < my ? lens[f * (size_t)my + i] : 0u;
        uint32_t tot;
        const uint32_t ex = enc_scan(v, &tot, wsum, tid);
        if (i < my) offs[f * (size_t)my + i] = carry + ex;
        carry += tot;
    }
    const unsigned long long total = (unsigned long long)kJpegHeaderBytes + carry + 2ull * (unsigned)(my - 1) + 2ull;
    if (tid == 0) d_bytes[f] = total <= (unsigned long long)slot_bytes ? (int64_t)total : (int64_t)CG_E_CAPACITY;
}

// One workgroup per (interval, frame): the interval's bytes to their place in the slot, the RST
// marker before it, the header with the first and EOI with the last.  A frame that does not fit
// writes nothing.
__global__ __launch_bounds__(kEncThreads) void jpeg_enc_gather_kernel(const uint8_t *__restrict__ stage, size_t stage_cap,
                                                                     const uint32_t *__restrict__ lens,
                                                                     const unsigned long long *__restrict__ offs, int my,
                                                                     JpegHeader hdr, uint8_t *__restrict__ d_out,
                                                                     size_t slot_bytes, const int64_t *__restrict__ d_bytes)
{
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x;
    const size_t f = blockIdx.y;
    if (d_bytes[f] < 0) return;
    uint8_t *o = d_out + f * slot_bytes;
    if (i == 0)
        for (int j = tid; j < kJpegHeaderBytes; j += kEncThreads) o[j] = hdr.b[j];
    const size_t at = (size_t)kJpegHeaderBytes + (size_t)offs[f * (size_t)my + i] + 2 * (size_t)i;
    const uint32_t len = lens[f * (size_t)my + i];
    const uint8_t *src = stage + (f * (size_t)my + (size_t)i) * stage_cap;
    if (i > 0 && tid == 0) {
        o[at - 2] = 0xFF;
        o[at - 1] = (uint8_t)(0xD0 + ((i - 1) & 7));
    }
    for (uint32_t j = (uint32_t)tid; j < len; j += kEncThreads) o[at + j] = src[j];
    if (i == my - 1 && tid == 0) {
        o[at + len] = 0xFF;
        o[at + len + 1] = 0xD9;
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

using namespace cg;

// ---- host-only (no device, no context) ------------------------------------------------------
extern "C" long long cg_image_jpeg_bound(int width, int height, int subsampling)
{
    const cg_jpeg_params p{50, subsampling};
    if (!params_ok(width, height, &p)) return CG_E_INVALID;
    return (long long)file_bound(jpeg_shape(width, height, subsampling));
}

extern "C" int cg_image_jpeg_header(int width, int height, const cg_jpeg_params *params, uint8_t *out, size_t cap)
{
    if (!params_ok(width, height, params) || !out) return CG_E_INVALID;
    if (cap < (size_t)kJpegHeaderBytes) return CG_E_CAPACITY;
    write_header(jpeg_shape(width, height, params->subsampling), make_quant(params->quality), out);
    return kJpegHeaderBytes;
}

extern "C" int cg_image_jpeg_enc_limits(int *threads, int *stage_bytes)
{
    if (threads) *threads = kEncThreads;
    if (stage_bytes) *stage_bytes = kEncStageBytes;
    return CG_OK;
}

extern "C" int cg_image_encode_jpeg_host(const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                                         const cg_jpeg_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!params_ok(width, height, params) || !argb || !n || (!out && cap)) return CG_E_INVALID;
    const size_t stride = row_stride_pixels ? row_stride_pixels : (size_t)width;
    if (stride < (size_t)width) return CG_E_INVALID;
    const JpegShape s = jpeg_shape(width, height, params->subsampling);
    const JpegQuant q = make_quant(params->quality);
    uint8_t hdr[kJpegHeaderBytes];
    write_header(s, q, hdr);
    HostBits w{out, cap};
    for (int i = 0; i < kJpegHeaderBytes; ++i) w.byte(hdr[i]);
    int16_t zz[64];
    for (int my = 0; my < s.my; ++my) {
        if (my) {
            w.pad();
            w.byte(0xFF);
            w.byte(0xD0 + ((my - 1) & 7));
        }
        int pred[3] = {0, 0, 0};
        for (int mx = 0; mx < s.mx; ++mx)
            for (int k = 0; k < s.bpm; ++k) {
                host_block(argb, stride, s, q, mx, my, k, zz);
                const int comp = s.sub == CG_JPEG_420 ? (k < 4 ? 0 : k - 3) : k;
                jpeg_code_block(kHuff, comp ? 1 : 0, pred[comp], [&](int j) { return (int)zz[j]; },
                                [&](uint32_t bits, int len) { w.put(bits, len); });
                pred[comp] = zz[0];
            }
    }
    w.pad();
    w.byte(0xFF);
    w.byte(0xD9);
    *n = w.n;
    return w.n > cap ? CG_E_CAPACITY : CG_OK;
}

// ---- device ---------------------------------------------------------------------------------
extern "C" int cg_image_encode_jpeg_device(cg_ctx *c, const uint32_t *d_argb, int width, int height, int n_frames,
                                           size_t frame_stride, const cg_jpeg_params *params, uint8_t *d_out,
                                           size_t slot_bytes, int64_t *d_bytes, void *stream)
{
    if (!c || n_frames < 0 || !params_ok(width, height, params)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const size_t px = (size_t)width * height;
    if (!frame_stride) frame_stride = px;
    if (!d_argb || ((uintptr_t)d_argb & 3) || !d_out || !d_bytes || ((uintptr_t)d_bytes & 7) || frame_stride < px)
        return CG_E_INVALID;
    const JpegShape s = jpeg_shape(width, height, params->subsampling);
    const JpegQuant q = make_quant(params->quality);
    JpegHeader hdr{};
    write_header(s, q, hdr.b);
    const size_t nb = (size_t)s.mx * s.bpm, n_blocks = nb * s.my;
    // an interval longer than the slot belongs to a frame that does not fit: its staging area need
    // not hold more than the slot (the entropy kernel stops storing at stage_cap and counts on)
    const size_t stage_cap = align256(std::max<size_t>(std::min(interval_bound(nb), slot_bytes), 1));
    const int chunk = std::min(n_frames, kEncChunkFrames);
    const size_t coef_b = align256((size_t)chunk * n_blocks * 128), lens_b = align256((size_t)chunk * s.my * 4),
                 offs_b = align256((size_t)chunk * s.my * 8), stage_b = (size_t)chunk * s.my * stage_cap;
    CG_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipError_t e = hipSuccess;
    uint8_t *scratch = static_cast<uint8_t *>(ctx_buf(c, kBufJpegEnc, coef_b + lens_b + offs_b + stage_b, &e));
    if (!scratch) return ctx_fail(c, e, "alloc jpeg encoder scratch");
    int16_t *coef = (int16_t *)scratch;
    uint32_t *lens = (uint32_t *)(scratch + coef_b);
    unsigned long long *offs = (unsigned long long *)(scratch + coef_b + lens_b);
    uint8_t *stage = scratch + coef_b + lens_b + offs_b;
    hipStream_t st = stream ? (hipStream_t)stream : ctx_stream(c);
    for (int f0 = 0; f0 < n_frames; f0 += kEncChunkFrames) {
        const unsigned nf = (unsigned)std::min(kEncChunkFrames, n_frames - f0);
        hipLaunchKernelGGL(jpeg_enc_transform_kernel,
                           dim3((unsigned)((n_blocks + kEncXfBlocks - 1) / kEncXfBlocks), nf), dim3(kEncThreads), 0, st,
                           d_argb + (size_t)f0 * frame_stride, frame_stride, s, q, coef, (unsigned)n_blocks);
        hipLaunchKernelGGL(jpeg_enc_entropy_kernel, dim3((unsigned)s.my, nf), dim3(kEncThreads), 0, st,
                           (const int16_t *)coef, s, (unsigned)n_blocks, stage, stage_cap, lens);
        hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3(nf), dim3(kEncThreads), 0, st, (const uint32_t *)lens, s.my,
                           slot_bytes, offs, d_bytes + f0);
        hipLaunchKernelGGL(jpeg_enc_gather_kernel, dim3((unsigned)s.my, nf), dim3(kEncThreads), 0, st,
                           (const uint8_t *)stage, stage_cap, (const uint32_t *)lens, (const unsigned long long *)offs,
                           s.my, hdr, d_out + (size_t)f0 * slot_bytes, slot_bytes, (const int64_t *)(d_bytes + f0));
    }
    CG_TRY(c, hipGetLastError(), "jpeg encoder launch");
    return CG_OK;
}

extern "C" int cg_image_encode_jpeg(cg_ctx *c, const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                                    const cg_jpeg_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!c || !params_ok(width, height, params) || !argb || !n || (!out && cap)) return CG_E_INVALID;
    const size_t stride = row_stride_pixels ? row_stride_pixels : (size_t)width;
    if (stride < (size_t)width) return CG_E_INVALID;
    const size_t px_b = align256((size_t)width * height * 4);
    const size_t bound = file_bound(jpeg_shape(width, height, params->subsampling));
    CG_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipError_t e = hipSuccess;
    uint8_t *io = static_cast<uint8_t *>(ctx_buf(c, kBufJpegEncIo, px_b + 256 + bound, &e));
    if (!io) return ctx_fail(c, e, "alloc jpeg encoder frame");
    hipStream_t st = ctx_stream(c);
    CG_TRY(c, hipMemcpy2DAsync(io, (size_t)width * 4, argb, stride * 4, (size_t)width * 4, (size_t)height,
                               hipMemcpyHostToDevice, st),
           "jpeg frame upload");
    int64_t *d_bytes = (int64_t *)(io + px_b);
    uint8_t *d_file = io + px_b + 256;
    if (int rc = cg_image_encode_jpeg_device(c, (const uint32_t *)io, width, height, 1, 0, params, d_file, bound, d_bytes, st))
        return rc;
    int64_t len = 0;
    CG_TRY(c, hipMemcpyAsync(&len, d_bytes, 8, hipMemcpyDeviceToHost, st), "jpeg length download");
    CG_TRY(c, hipStreamSynchronize(st), "jpeg encode");
    if (len < 0) return ctx_invalid(c, "jpeg encoder: a file longer than its bound");
    *n = (size_t)len;
    if ((size_t)len > cap) return CG_E_CAPACITY;
    CG_TRY(c, hipMemcpy(out, d_file, (size_t)len, hipMemcpyDeviceToHost), "jpeg file download");
    return CG_OK;
}
