// cg_exr_enc.hip -- the OpenEXR encoder for CG_PIX_RGBA_F32 pictures: the host-only restatement
// (cg_image_encode_exr_host, cg_image_exr_bound, cg_image_exr_header, cg_image_exr_half) and the
// device encoder (cg_image_encode_exr_device, cg_image_encode_exr).  The arithmetic is
// cg_exr_enc.h's and, for a ZIP chunk's deflate stream, cg_png_enc.h's; the contract is
// include/cg_render.h's: a single-part scanline file whose ZIP chunks of 16 scanlines are each one
// zlib stream of one dynamic Huffman block, or the raw bytes when that is not shorter.
//
// The device encoder is four kernels a chunk of up to 8 frames (ZIP; NONE runs the last two):
//   exr_enc_plane_kernel   a lane makes four bytes of a chunk's reordered, predicted bytes d straight
//                          from the source floats: it converts its own samples and the sample of
//                          the byte before its first, so no lane waits on another
//   exr_enc_chunk_kernel   one workgroup per (chunk, frame) deflates d with the PNG band kernel's
//                          method (cg_deflate.h) into the chunk's staging area, 78 01 in front and
//                          the Adler-32 behind; a chunk whose stream is not shorter is marked raw
//   exr_enc_scan_kernel    a frame's chunk lengths to file offsets, the length to d_bytes
//   exr_enc_gather_kernel  header, offset table entry, chunk header and data into the slot; a raw
//                          chunk's samples are made again from the source floats
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cg_deflate.h"
#include "cg_exr_enc.h"
#include "cg_host.h"
#include "cg_internal.h"

namespace {

using namespace cg;

constexpr cg_exr_params kExrDefault = {CG_EXR_RGBA, CG_EXR_HALF, CG_EXR_ZIP, 1.0f};

bool params_ok(int w, int h, const cg_exr_params *p)
{
    return w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && (p->channels == CG_EXR_RGB || p->channels == CG_EXR_RGBA) &&
           (p->type == CG_EXR_HALF || p->type == CG_EXR_FLOAT) && (p->compression == CG_EXR_NONE || p->compression == CG_EXR_ZIP) &&
           std::isfinite(p->alpha_scale);
}

size_t file_bound(const ExrShape &s)
{
    return (size_t)s.hdr + 16 * (size_t)s.nc + (size_t)s.h * s.rowb;   // a table entry and a chunk header: 8 + 8
}

// ---- kernels --------------------------------------------------------------------------------

constexpr int kExrPlaneThreads = 256;
constexpr int kExrPlaneBytes = 4;                 // bytes of d a lane of the plane kernel makes
constexpr int kExrGatherThreads = 256;
constexpr int kExrChunkFrames = 8;                // frames the context's scratch holds
constexpr uint32_t kExrRaw = 0x80000000u;         // in a chunk's length: its data is the raw bytes

// grid (pieces of a chunk, chunks, frames)
__global__ __launch_bounds__(kExrPlaneThreads) void exr_enc_plane_kernel(const float *__restrict__ rgba, size_t frame_stride,
                                                                        ExrShape s, uint8_t *__restrict__ pred,
                                                                        size_t frame_bytes)
{
    const int k = (int)blockIdx.y;
    const uint32_t n = exr_chunk_bytes(s, k);
    const uint32_t i0 = ((uint32_t)blockIdx.x * kExrPlaneThreads + threadIdx.x) * kExrPlaneBytes;
    if (i0 >= n) return;
    const int cnt = n - i0 < (uint32_t)kExrPlaneBytes ? (int)(n - i0) : kExrPlaneBytes;
    const float *rows = rgba + ((size_t)blockIdx.z * frame_stride + (size_t)k * s.lines * (size_t)s.w) * 4;
    uint8_t d[kExrPlaneBytes] = {0, 0, 0, 0};
    exr_predicted(s, rows, (size_t)s.w, n, i0, cnt, d);
    // frame_bytes is a multiple of 256 and a chunk of 16 scanlines of 4: the word is aligned
    uint8_t *dst = pred + (size_t)blockIdx.z * frame_bytes + (size_t)k * s.lines * (size_t)s.rowb + i0;
    if (cnt == kExrPlaneBytes) *(uint32_t *)dst = (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
    else
        for (int j = 0; j < cnt; ++j) dst[j] = d[j];
}

// One workgroup per (chunk, frame): png_enc_band_kernel's walk over d, framed as a whole zlib stream.
__global__ __launch_bounds__(kPngThreads) void exr_enc_chunk_kernel(const uint8_t *__restrict__ pred, size_t frame_bytes,
                                                                   ExrShape s, uint8_t *__restrict__ stage, size_t stage_cap,
                                                                   uint32_t *__restrict__ lens)
{
    __shared__ uint32_t win[kPngWinWords];
    __shared__ uint32_t hist[kPngLitLen];
    __shared__ PngPlan plan;
    __shared__ PngHuffWork work;
    __shared__ PngBandShared sh;
    __shared__ uint32_t wsum[kPngWaves];
    __shared__ uint32_t asum[2];
    __shared__ int n_used;
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x;
    const size_t f = blockIdx.y;
    const uint32_t n = exr_chunk_bytes(s, k);
    const uint8_t *src = pred + f * frame_bytes + (size_t)k * s.lines * (size_t)s.rowb;
    const size_t slot = f * (size_t)s.nc + (size_t)k;
    uint8_t *out = stage + slot * stage_cap;

    for (int i = tid; i < kPngLitLen; i += kPngThreads) hist[i] = i == 256 ? 1u : 0u;
    if (tid == 0) sh.carry = 0u, asum[0] = 0u, asum[1] = 0u, n_used = 0;
    __syncthreads();
    // pass 1: the symbols' frequencies and the Adler sums
    unsigned long long s1 = 0, s2 = 0;
    for (uint32_t pos0 = 0; pos0 < n; pos0 += kPngThreads) {
        int byte, len;
        const int kind = png_piece_token(src, n, pos0, tid, sh, &byte, &len);
        if (kind == 1) atomicAdd(&hist[byte], 1u);
        if (kind == 2) {
            int eb, ev;
            atomicAdd(&hist[png_len_symbol(len, &eb, &ev)], 1u);
        }
        const uint32_t i = pos0 + (uint32_t)tid;
        if (i < n) s1 += (unsigned)byte, s2 += (unsigned long long)(n - i) * (unsigned)byte;
    }
    atomicAdd(&asum[0], (uint32_t)(s1 % kAdlerMod));
    atomicAdd(&asum[1], (uint32_t)(s2 % kAdlerMod));
    __syncthreads();
    // the used symbols by (frequency, symbol): a lane ranks its own
    if (tid < kPngLitLen && hist[tid]) {
        const uint32_t fq = hist[tid];
        int rank = 0;
        for (int t = 0; t < kPngLitLen; ++t) {
            const uint32_t g = hist[t];
            rank += (g && (g < fq || (g == fq && t < tid))) ? 1 : 0;
        }
        work.order[rank] = (uint16_t)tid;
        atomicAdd(&n_used, 1);
    }
    __syncthreads();
    if (tid == 0) png_make_plan(hist, n_used, plan, work);
    __syncthreads();

    // 78 01, the block, zero bits to the byte, the Adler-32; stored blocks are longer than n
    const uint32_t zlen = 2u + ((plan.dyn_bits + 7u) >> 3) + 4u;
    if (plan.dyn_bits >= png_stored_bits(n) || zlen >= n) {
        if (tid == 0) lens[slot] = n | kExrRaw;
        return;
    }

    for (int i = tid; i < kPngWinWords; i += kPngThreads) win[i] = 0u;
    if (tid == 0) sh.carry = 0u;
    __syncthreads();
    int win0 = 0;                                   // bit where the window starts
    int carry = (int)(16u + plan.header_bits);      // bit where the next token starts
    size_t outpos = 0;
    if (tid == 0) {
        int p = 0;
        auto put = [&](uint32_t bits, int l) {
            if (l) png_deposit(win, 0, p, bits, l);
            p += l;
        };
        put(0x78u, 8), put(0x01u, 8);
        png_put_header(plan, 1, put);
    }
    __syncthreads();
    // rounds: the pieces of d, then one round of the end-of-block and its pad on lane 0
    const uint32_t rounds = (n + kPngThreads - 1) / kPngThreads;
    for (uint32_t r = 0; r <= rounds; ++r) {
        uint32_t bits = 0;
        int nbits = 0;
        if (r < rounds) {
            int byte, len;
            const int kind = png_piece_token(src, n, r * kPngThreads, tid, sh, &byte, &len);
            if (kind == 1) bits = png_literal_bits(plan, byte, &nbits);
            if (kind == 2) bits = png_match_bits(plan, len, &nbits);
        } else if (tid == 0) {
            bits = png_literal_bits(plan, 256, &nbits);
            nbits = ((carry + nbits + 7) & ~7) - carry;
        }
        uint32_t tot;
        const int off = carry + (int)png_scan((uint32_t)nbits, &tot, wsum, tid);
        const int total = carry + (int)tot;
        for (;;) {
            if (nbits && off < win0 + kPngWinBits && off + nbits > win0) png_deposit(win, win0, off, bits, nbits);
            __syncthreads();
            if (total - win0 < kPngWinBits) break;
            png_flush(win, kPngWinBytes, out, stage_cap, outpos, tid);
            outpos += kPngWinBytes;
            __syncthreads();
            for (int i = tid; i < kPngWinWords; i += kPngThreads) win[i] = 0u;
            win0 += kPngWinBits;
            __syncthreads();
        }
        carry = total;
    }
    png_flush(win, (carry - win0) >> 3, out, stage_cap, outpos, tid);
    if (tid == 0) {
        const uint32_t a = (1u + asum[0]) % kAdlerMod, b = (n % kAdlerMod + asum[1]) % kAdlerMod;
        const uint32_t ad = (b << 16) | a;
        const size_t at = (size_t)(carry >> 3);
        for (int j = 0; j < 4; ++j)
            if (at + j < stage_cap) out[at + j] = (uint8_t)(ad >> (8 * (3 - j)));
        lens[slot] = (uint32_t)(carry >> 3) + 4u;
    }
}

// One workgroup a frame: offs[k] = where chunk k starts in the file, d_bytes = the file's length
// or CG_E_CAPACITY when the slot is shorter.  lens == NULL (NONE): every chunk is its raw bytes.
__global__ __launch_bounds__(kPngThreads) void exr_enc_scan_kernel(const uint32_t *__restrict__ lens, ExrShape s,
                                                                  size_t slot_bytes, unsigned long long *__restrict__ offs,
                                                                  int64_t *__restrict__ d_bytes)
{
    __shared__ uint32_t wsum[kPngWaves];
    const int tid = (int)threadIdx.x;
    const size_t f = blockIdx.x;
    unsigned long long carry = (unsigned long long)s.hdr + 8ull * (unsigned long long)s.nc;
    for (int k0 = 0; k0 < s.nc; k0 += kPngThreads) {
        const int k = k0 + tid;
        // a chunk is at most 16.8 MB and 1024 of them pass 32 bits: the quarters and the rests are summed apart
        const uint32_t v = k < s.nc ? 8u + (lens ? lens[f * (size_t)s.nc + k] & ~kExrRaw : exr_chunk_bytes(s, k)) : 0u;
        uint32_t tot;
        const uint32_t ex = png_scan(v >> 2, &tot, wsum, tid);
        uint32_t tot2;
        const uint32_t ex2 = png_scan(v & 3u, &tot2, wsum, tid);
        if (k < s.nc) offs[f * (size_t)s.nc + k] = carry + 4ull * ex + ex2;
        carry += 4ull * tot + tot2;
    }
    if (tid == 0) d_bytes[f] = carry <= (unsigned long long)slot_bytes ? (int64_t)carry : (int64_t)CG_E_CAPACITY;
}

struct ExrHeader {
    uint8_t b[336];   // 331 at most
};

// One workgroup per (chunk, frame): the chunk to its place in the slot -- its table entry, first
// y, data length and data -- and the header with the first.  A frame that does not fit writes nothing.
__global__ __launch_bounds__(kExrGatherThreads) void exr_enc_gather_kernel(
    const float *__restrict__ rgba, size_t frame_stride, ExrShape s, const uint8_t *__restrict__ stage, size_t stage_cap,
    const uint32_t *__restrict__ lens, const unsigned long long *__restrict__ offs, ExrHeader hdr, uint8_t *__restrict__ d_out,
    size_t slot_bytes, const int64_t *__restrict__ d_bytes)
{
    const int tid = (int)threadIdx.x;
    const int k = (int)blockIdx.x;
    const size_t f = blockIdx.y;
    if (d_bytes[f] < 0) return;
    uint8_t *o = d_out + f * slot_bytes;
    if (k == 0)
        for (int j = tid; j < s.hdr; j += kExrGatherThreads) o[j] = hdr.b[j];
    const size_t slot = f * (size_t)s.nc + (size_t)k;
    const uint32_t n = exr_chunk_bytes(s, k);
    const uint32_t word = lens ? lens[slot] : n | kExrRaw;
    const uint32_t dl = word & ~kExrRaw;
    const unsigned long long at = offs[slot];
    if (tid < 8) o[(size_t)s.hdr + 8 * (size_t)k + tid] = (uint8_t)(at >> (8 * tid));
    if (tid >= 8 && tid < 16) {
        const uint32_t v = tid < 12 ? (uint32_t)(k * s.lines) : dl;
        o[at + (tid - 8)] = (uint8_t)(v >> (8 * (tid & 3)));
    }
    uint8_t *data = o + at + 8;
    if (word & kExrRaw) {
        const float *rows = rgba + (f * frame_stride + (size_t)k * s.lines * (size_t)s.w) * 4;
        const uint32_t per_line = (uint32_t)s.w * (uint32_t)s.nch, ns = n / (uint32_t)s.bps;
        for (uint32_t i = (uint32_t)tid; i < ns; i += kExrGatherThreads) {
            const uint32_t line = i / per_line, q = i - line * per_line;
            const uint32_t ch = q / (uint32_t)s.w, x = q - ch * (uint32_t)s.w;
            const uint32_t v = exr_sample(rows + ((size_t)line * s.w + x) * 4, s, (int)ch);
            uint8_t *p = data + (size_t)i * s.bps;
            for (int b = 0; b < s.bps; ++b) p[b] = (uint8_t)(v >> (8 * b));
        }
    } else {
        const uint8_t *src = stage + slot * stage_cap;
        for (uint32_t j = (uint32_t)tid; j < dl; j += kExrGatherThreads) data[j] = src[j];
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

uint32_t host_adler(const uint8_t *d, size_t n)
{
    uint32_t a = 1u, b = 0u;
    for (size_t i = 0; i < n; ++i) {
        a = (a + d[i]) % kAdlerMod;
        b = (b + a) % kAdlerMod;
    }
    return (b << 16) | a;
}

}  // namespace

namespace cg {
bool exr_resolve_params(const cg_exr_params *in, cg_exr_params *out)
{
    *out = in ? *in : kExrDefault;
    return params_ok(1, 1, out);
}
}  // namespace cg

using namespace cg;

// ---- host-only (no device, no context) ------------------------------------------------------
extern "C" long long cg_image_exr_bound(int width, int height, int channels, int type)
{
    const cg_exr_params p{channels, type, CG_EXR_NONE, 1.0f};
    if (!params_ok(width, height, &p)) return CG_E_INVALID;
    return (long long)file_bound(exr_shape(width, height, p));
}

extern "C" int cg_image_exr_enc_limits(int *threads, int *window_bytes)
{
    if (threads) *threads = kPngThreads;
    if (window_bytes) *window_bytes = kPngWinBytes;
    return CG_OK;
}

extern "C" int cg_image_exr_half(const float *values, int n, uint16_t *halves)
{
    if (n < 0 || (n && (!values || !halves))) return CG_E_INVALID;
    for (int i = 0; i < n; ++i) halves[i] = (uint16_t)exr_half_bits(exr_float_bits(values[i]));
    return CG_OK;
}

extern "C" int cg_image_exr_header(int width, int height, const cg_exr_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!params) params = &kExrDefault;
    if (!params_ok(width, height, params) || !n || (!out && cap)) return CG_E_INVALID;
    const ExrShape s = exr_shape(width, height, *params);
    uint8_t b[kExrMaxHeader];
    const int len = exr_put_header(s, b);
    *n = (size_t)len;
    if ((size_t)len > cap) return CG_E_CAPACITY;
    std::memcpy(out, b, (size_t)len);
    return CG_OK;
}

extern "C" int cg_image_encode_exr_host(const float *rgba, int width, int height, size_t row_stride_pixels,
                                        const cg_exr_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!params) params = &kExrDefault;
    if (!params_ok(width, height, params) || !rgba || !n || (!out && cap)) return CG_E_INVALID;
    const size_t stride = row_stride_pixels ? row_stride_pixels : (size_t)width;
    if (stride < (size_t)width) return CG_E_INVALID;
    const ExrShape s = exr_shape(width, height, *params);
    // every chunk's data first: the table in front needs their lengths
    std::vector<std::vector<uint8_t>> data((size_t)s.nc);
    std::vector<uint8_t> raw, d;
    std::vector<uint32_t> freq(kPngLitLen);
    PngPlan plan;
    PngHuffWork work;
    for (int k = 0; k < s.nc; ++k) {
        const uint32_t nk = exr_chunk_bytes(s, k);
        const float *rows = rgba + (size_t)k * s.lines * stride * 4;
        raw.resize(nk);
        ExrCursor c;
        for (uint32_t p = 0; p < nk; ++p) {
            c.seek(s, p);
            raw[p] = (uint8_t)c.byte(s, rows, stride);
        }
        std::vector<uint8_t> &z = data[(size_t)k];
        if (s.zip) {
            d.resize(nk);
            for (uint32_t i = 0; i < nk; i += 4) exr_predicted(s, rows, stride, nk, i, (int)std::min<uint32_t>(4u, nk - i), d.data() + i);
            std::fill(freq.begin(), freq.end(), 0u);
            freq[256] = 1;
            host_tokens(d.data(), nk, [&](int kind, int byte, int len) {
                int eb, ev;
                ++freq[kind == 1 ? byte : png_len_symbol(len, &eb, &ev)];
            });
            const int m = png_sort_symbols(freq.data(), kPngLitLen, work.order);
            png_make_plan(freq.data(), m, plan, work);
            // stored blocks (rule 7) make a stream longer than nk: only a dynamic block can be the data
            if (plan.dyn_bits < png_stored_bits(nk) && 2u + ((plan.dyn_bits + 7u) >> 3) + 4u < nk) {
                z.push_back(0x78), z.push_back(0x01);
                HostBits w{z};
                png_put_header(plan, 1, [&](uint32_t bits, int l) { w.put(bits, l); });
                host_tokens(d.data(), nk, [&](int kind, int byte, int len) {
                    int nb2;
                    const uint32_t bits = kind == 1 ? png_literal_bits(plan, byte, &nb2) : png_match_bits(plan, len, &nb2);
                    w.put(bits, nb2);
                });
                w.put(plan.ll_code[256], plan.ll_len[256]);
                w.align();
                const uint32_t ad = host_adler(d.data(), nk);
                for (int j = 3; j >= 0; --j) z.push_back((uint8_t)(ad >> (8 * j)));
            }
        }
        if (z.empty()) z = raw;
    }
    HostSink sink{out, cap};
    uint8_t hdr[kExrMaxHeader];
    exr_put_header(s, hdr);
    for (int i = 0; i < s.hdr; ++i) sink.byte(hdr[i]);
    auto le = [&](unsigned long long v, int bytes) {
        for (int j = 0; j < bytes; ++j) sink.byte((int)(v >> (8 * j)) & 255);
    };
    unsigned long long at = (unsigned long long)s.hdr + 8ull * (unsigned long long)s.nc;
    for (int k = 0; k < s.nc; ++k) le(at, 8), at += 8 + data[(size_t)k].size();
    for (int k = 0; k < s.nc; ++k) {
        le((unsigned long long)(k * s.lines), 4), le(data[(size_t)k].size(), 4);
        for (uint8_t v : data[(size_t)k]) sink.byte(v);
    }
    *n = sink.n;
    return sink.n > cap ? CG_E_CAPACITY : CG_OK;
}

// ---- device ---------------------------------------------------------------------------------
extern "C" int cg_image_encode_exr_device(cg_ctx *c, const float *d_rgba, int width, int height, int n_frames,
                                          size_t frame_stride, const cg_exr_params *params, uint8_t *d_out, size_t slot_bytes,
                                          int64_t *d_bytes, void *stream)
{
    if (!params) params = &kExrDefault;
    if (!c || n_frames < 0 || !params_ok(width, height, params)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const size_t px = (size_t)width * height;
    if (!frame_stride) frame_stride = px;
    if (!d_rgba || ((uintptr_t)d_rgba & 15) || !d_out || !d_bytes || ((uintptr_t)d_bytes & 7) || frame_stride < px)
        return CG_E_INVALID;
    const ExrShape s = exr_shape(width, height, *params);
    ExrHeader hdr{};
    exr_put_header(s, hdr.b);
    const uint32_t n0 = exr_chunk_bytes(s, 0);
    // only a stream shorter than its chunk is staged, and one longer than the slot belongs to a
    // frame that does not fit (the chunk kernel stops storing at stage_cap and counts on)
    const size_t stage_cap = align256(std::max<size_t>(std::min<size_t>(n0, slot_bytes), 1));
    const int chunk = std::min(n_frames, kExrChunkFrames);
    const size_t frame_bytes = align256((size_t)s.h * s.rowb);
    const size_t nchunks = (size_t)chunk * s.nc;
    const size_t pred_b = s.zip ? (size_t)chunk * frame_bytes : 0, lens_b = align256(nchunks * 4), offs_b = align256(nchunks * 8),
                 stage_b = s.zip ? nchunks * stage_cap : 0;
    CG_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipError_t e = hipSuccess;
    uint8_t *scratch = static_cast<uint8_t *>(ctx_exr_buf(c, 0, pred_b + lens_b + offs_b + stage_b, &e));
    if (!scratch) return ctx_fail(c, e, "alloc exr encoder scratch");
    uint8_t *pred = scratch;
    uint32_t *lens = (uint32_t *)(scratch + pred_b);
    unsigned long long *offs = (unsigned long long *)(scratch + pred_b + lens_b);
    uint8_t *stage = scratch + pred_b + lens_b + offs_b;
    hipStream_t st = stream ? (hipStream_t)stream : ctx_stream(c);
    for (int f0 = 0; f0 < n_frames; f0 += kExrChunkFrames) {
        const unsigned nf = (unsigned)std::min(kExrChunkFrames, n_frames - f0);
        const float *src = d_rgba + (size_t)f0 * frame_stride * 4;
        if (s.zip) {
            const unsigned pieces = (n0 + kExrPlaneThreads * kExrPlaneBytes - 1) / (kExrPlaneThreads * kExrPlaneBytes);
            kt_launch(KT_EXR_PLANE, exr_enc_plane_kernel, dim3(pieces, (unsigned)s.nc, nf), dim3(kExrPlaneThreads), 0, st, src,
                      frame_stride, s, pred, frame_bytes);
            kt_launch(KT_EXR_CHUNK, exr_enc_chunk_kernel, dim3((unsigned)s.nc, nf), dim3(kPngThreads), 0, st, (const uint8_t *)pred,
                      frame_bytes, s, stage, stage_cap, lens);
        }
        kt_launch(KT_EXR_SCAN, exr_enc_scan_kernel, dim3(nf), dim3(kPngThreads), 0, st, s.zip ? (const uint32_t *)lens : nullptr, s,
                  slot_bytes, offs, d_bytes + f0);
        kt_launch(KT_EXR_GATHER, exr_enc_gather_kernel, dim3((unsigned)s.nc, nf), dim3(kExrGatherThreads), 0, st, src, frame_stride,
                  s, (const uint8_t *)stage, stage_cap, s.zip ? (const uint32_t *)lens : nullptr,
                  (const unsigned long long *)offs, hdr, d_out + (size_t)f0 * slot_bytes, slot_bytes,
                  (const int64_t *)(d_bytes + f0));
    }
    CG_TRY(c, hipGetLastError(), "exr encoder launch");
    return CG_OK;
}

extern "C" int cg_image_encode_exr(cg_ctx *c, const float *rgba, int width, int height, size_t row_stride_pixels,
                                   const cg_exr_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!params) params = &kExrDefault;
    if (!c || !params_ok(width, height, params) || !rgba || !n || (!out && cap)) return CG_E_INVALID;
    const size_t stride = row_stride_pixels ? row_stride_pixels : (size_t)width;
    if (stride < (size_t)width) return CG_E_INVALID;
    const size_t px_b = align256((size_t)width * height * 16);
    const size_t bound = file_bound(exr_shape(width, height, *params));
    CG_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipError_t e = hipSuccess;
    uint8_t *io = static_cast<uint8_t *>(ctx_exr_buf(c, 1, px_b + 256 + bound, &e));
    if (!io) return ctx_fail(c, e, "alloc exr encoder frame");
    hipStream_t st = ctx_stream(c);
    CG_TRY(c, hipMemcpy2DAsync(io, (size_t)width * 16, rgba, stride * 16, (size_t)width * 16, (size_t)height,
                               hipMemcpyHostToDevice, st),
           "exr frame upload");
    int64_t *d_bytes = (int64_t *)(io + px_b);
    uint8_t *d_file = io + px_b + 256;
    if (int rc = cg_image_encode_exr_device(c, (const float *)io, width, height, 1, 0, params, d_file, bound, d_bytes, st))
        return rc;
    int64_t len = 0;
    CG_TRY(c, hipMemcpyAsync(&len, d_bytes, 8, hipMemcpyDeviceToHost, st), "exr length download");
    CG_TRY(c, hipStreamSynchronize(st), "exr encode");
    if (len < 0) return ctx_invalid(c, "exr encoder: a file longer than its bound");
    *n = (size_t)len;
    if ((size_t)len > cap) return CG_E_CAPACITY;
    CG_TRY(c, hipMemcpy(out, d_file, (size_t)len, hipMemcpyDeviceToHost), "exr file download");
    return CG_OK;
}
