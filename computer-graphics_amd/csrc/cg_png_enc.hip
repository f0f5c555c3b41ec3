// cg_png_enc.hip -- the lossless PNG encoder: the host-only restatement
// (cg_image_encode_png_host, cg_image_png_bound, cg_image_png_code_lengths) and the device encoder
// (cg_image_encode_png_device, cg_image_encode_png).  The arithmetic is cg_png_enc.h's, the
// contract include/cg_render.h's: a standard PNG whose IDAT chunks are bands of 16 rows, each
// deflated on its own with distance-1 matches and one dynamic Huffman block.
//
// The device encoder is four kernels a chunk of up to 8 frames:
//   png_enc_filter_kernel  one workgroup a row: the five filters' sums of |int8|, the chosen
//                          filter's bytes into scratch
//   png_enc_band_kernel    one workgroup per (band, frame), walking the band in pieces of one byte
//                          a lane: a ballot marks the runs, LDS atomics count the symbols, one
//                          lane builds the two codes (the sort is a parallel rank), then the
//                          tokens are sized, scanned and deposited into a window of the band's bit
//                          string in LDS, full windows flushed to the band's staging area; or the
//                          band is copied as stored blocks.  Also the band's Adler sums.
//   png_enc_scan_kernel    a frame's band lengths to offsets, the Adler-32, the length to d_bytes
//   png_enc_gather_kernel  signature, IHDR, the band's chunk with its CRC-32, IEND into the slot
#include <algorithm>
#include <cstring>
#include <vector>

#include "cg_host.h"
#include "cg_internal.h"
#include "cg_deflate.h"
#include "cg_png_enc.h"

namespace {

using namespace cg;

bool params_ok(int w, int h, const cg_png_params *p)
{
    return p && w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && (p->colour == CG_PNG_RGB || p->colour == CG_PNG_RGBA) &&
           (p->filter == CG_PNG_FILTER_ADAPTIVE || (p->filter >= 0 && p->filter <= 4));
}

constexpr int kPngFixedBytes = 8 + 25 + 12;   // signature, IHDR, IEND

// a band's bytes at most: its stored form, the zlib header before the first, the empty stored
// block after all but the last (the Adler-32 after the last is the gather's)
size_t band_bound(uint32_t n) { return (size_t)n + 5 * (size_t)png_stored_blocks(n) + 5; }
size_t file_bound(const PngShape &s)
{
    size_t b = kPngFixedBytes + 2 + 4;
    for (int k = 0; k < s.nb; ++k) {
        const uint32_t n = png_band_bytes(s, k);
        b += 12 + (size_t)n + 5 * (size_t)png_stored_blocks(n) + (k + 1 < s.nb ? 5 : 0);
    }
    return b;
}

void write_fixed(const PngShape &s, uint8_t sig_ihdr[33])
{
    static const uint8_t head[16] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    std::memcpy(sig_ihdr, head, 16);
    uint8_t *o = sig_ihdr + 16;
    const uint32_t wh[2] = {(uint32_t)s.w, (uint32_t)s.h};
    for (uint32_t v : wh)
        for (int k = 3; k >= 0; --k) *o++ = (uint8_t)(v >> (8 * k));
    *o++ = 8, *o++ = (uint8_t)(s.colour == CG_PNG_RGBA ? 6 : 2), *o++ = 0, *o++ = 0, *o++ = 0;
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) c = png_crc_byte(c, sig_ihdr[i]);
    c ^= 0xFFFFFFFFu;
    for (int k = 3; k >= 0; --k) *o++ = (uint8_t)(c >> (8 * k));
}
constexpr uint8_t kIend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};

// ---- kernels (the band walk is cg_deflate.h's) ------------------------------------------

// a * b mod the CRC polynomial, bits reflected (x^0 = 0x80000000): 32 steps whatever the operands
constexpr CG_HD uint32_t png_multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(2^k) mod the polynomial, for joining the CRCs of pieces
struct PngX2n {
    uint32_t t[32];
};
constexpr PngX2n png_make_x2n()
{
    PngX2n x{};
    uint32_t p = 1u << 30;   // x^1
    x.t[0] = p;
    for (int k = 1; k < 32; ++k) x.t[k] = p = png_multmodp(p, p);
    return x;
}
__constant__ PngX2n d_png_x2n = png_make_x2n();
constexpr uint32_t cx_crc_idat()
{
    uint32_t c = 0xFFFFFFFFu;
    const char t[4] = {'I', 'D', 'A', 'T'};
    for (int i = 0; i < 4; ++i) {
        c ^= (uint32_t)(uint8_t)t[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}
constexpr uint32_t kCrcIdat = cx_crc_idat();

// crc of (A then n more bytes) from crc(A), when the n bytes' own crc is xor-ed in afterwards
__device__ __forceinline__ uint32_t png_crc_shift(uint32_t crc, uint32_t n, const uint32_t *x2n)
{
    uint32_t p = 1u << 31;
    for (unsigned k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = png_multmodp(x2n[k & 31u], p);
    return png_multmodp(p, crc);
}


// One workgroup per (row, frame).
__global__ __launch_bounds__(kPngFilterThreads) void png_enc_filter_kernel(const uint32_t *__restrict__ argb,
                                                                          size_t frame_stride, PngShape s, int filter,
                                                                          uint8_t *__restrict__ filt, size_t frame_bytes)
{
    __shared__ uint32_t tot[5];
    const int tid = (int)threadIdx.x;
    const int y = (int)blockIdx.x;
    const uint32_t *cur = argb + (size_t)blockIdx.y * frame_stride + (size_t)y * (size_t)s.w;
    const uint32_t *up = y ? cur - s.w : nullptr;
    const int nbytes = s.w * s.bpp;
    int type = filter;
    if (filter == CG_PNG_FILTER_ADAPTIVE) {
        if (tid < 5) tot[tid] = 0u;
        __syncthreads();
        uint32_t sum[5] = {0u, 0u, 0u, 0u, 0u};
        for (int x = tid; x < nbytes; x += kPngFilterThreads) {
            int f[5];
            png_filter_all(cur, up, x, s.bpp, f);
#pragma unroll
            for (int t = 0; t < 5; ++t) sum[t] += png_abs8(f[t]);
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            uint32_t v = sum[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((tid & 63) == 0) atomicAdd(&tot[t], v);
        }
        __syncthreads();
        type = 0;
#pragma unroll
        for (int t = 1; t < 5; ++t)
            if (tot[t] < tot[type]) type = t;
    }
    uint8_t *out = filt + (size_t)blockIdx.y * frame_bytes + (size_t)y * (size_t)s.rb;
    if (tid == 0) out[0] = (uint8_t)type;
    for (int x = tid; x < nbytes; x += kPngFilterThreads) out[1 + x] = (uint8_t)png_filter_byte(type, cur, up, x, s.bpp);
}


// One workgroup per (band, frame).
__global__ __launch_bounds__(kPngThreads) void png_enc_band_kernel(const uint8_t *__restrict__ filt, size_t frame_bytes,
                                                                  PngShape s, uint8_t *__restrict__ stage,
                                                                  size_t stage_cap, uint32_t *__restrict__ lens,
                                                                  uint32_t *__restrict__ adler)
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
    const int band = (int)blockIdx.x;
    const size_t f = blockIdx.y;
    const uint32_t n = png_band_bytes(s, band);
    const bool last = band == s.nb - 1;
    const uint8_t *src = filt + f * frame_bytes + (size_t)band * kPngBandRows * (size_t)s.rb;
    const size_t slot = f * (size_t)s.nb + (size_t)band;
    uint8_t *out = stage + slot * stage_cap;
    const uint32_t prefix = band == 0 ? 2u : 0u;   // the zlib header 78 01

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
    if (tid == 0) adler[2 * slot] = asum[0] % kAdlerMod, adler[2 * slot + 1] = asum[1] % kAdlerMod;
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

    const uint32_t nblk = png_stored_blocks(n);
    if (plan.dyn_bits >= png_stored_bits(n)) {
        // stored blocks of at most 65535 bytes
        for (uint32_t i = (uint32_t)tid; i < n; i += kPngThreads) {
            const size_t o = (size_t)prefix + 5 * (size_t)(i / kPngMaxStored + 1u) + i;
            if (o < stage_cap) out[o] = src[i];
        }
        for (uint32_t b = (uint32_t)tid; b < nblk; b += kPngThreads) {
            const uint32_t l = n - b * kPngMaxStored < (uint32_t)kPngMaxStored ? n - b * kPngMaxStored : (uint32_t)kPngMaxStored;
            const size_t o = (size_t)prefix + (size_t)b * (kPngMaxStored + 5);
            const uint8_t h[5] = {(uint8_t)(last && b == nblk - 1 ? 1 : 0), (uint8_t)(l & 255u), (uint8_t)(l >> 8),
                                  (uint8_t)(~l & 255u), (uint8_t)((~l >> 8) & 255u)};
            for (int k = 0; k < 5; ++k)
                if (o + k < stage_cap) out[o + k] = h[k];
        }
        size_t total = (size_t)prefix + n + 5 * (size_t)nblk;
        if (tid == 0) {
            if (prefix) {
                if (0 < stage_cap) out[0] = 0x78;
                if (1 < stage_cap) out[1] = 0x01;
            }
            if (!last) {
                const uint8_t e[5] = {0, 0, 0, 0xFF, 0xFF};
                for (int k = 0; k < 5; ++k)
                    if (total + k < stage_cap) out[total + k] = e[k];
            }
            lens[slot] = (uint32_t)(total + (last ? 0 : 5));
        }
        return;
    }

    // the dynamic block: the header by one lane, then the tokens through the window
    for (int i = tid; i < kPngWinWords; i += kPngThreads) win[i] = 0u;
    if (tid == 0) sh.carry = 0u;
    __syncthreads();
    int win0 = 0;                                         // bit where the window starts
    int carry = (int)(8u * prefix + plan.header_bits);    // bit where the next token starts
    size_t outpos = 0;
    if (tid == 0) {
        int p = 0;
        auto put = [&](uint32_t bits, int l) {
            if (l) png_deposit(win, 0, p, bits, l);
            p += l;
        };
        if (prefix) put(0x78u, 8), put(0x01u, 8);
        png_put_header(plan, last ? 1 : 0, put);
    }
    __syncthreads();
    // rounds: the pieces of the band, then one round of the block's end on lane 0
    const uint32_t rounds = (n + kPngThreads - 1) / kPngThreads;
    for (uint32_t r = 0; r <= rounds; ++r) {
        uint32_t bits = 0;
        int nbits = 0;
        uint32_t tail_at = 0;   // the end round: where FFFF of the empty stored block goes, relative to the round
        if (r < rounds) {
            int byte, len;
            const int kind = png_piece_token(src, n, r * kPngThreads, tid, sh, &byte, &len);
            if (kind == 1) bits = png_literal_bits(plan, byte, &nbits);
            if (kind == 2) bits = png_match_bits(plan, len, &nbits);
        } else if (tid == 0) {
            bits = png_literal_bits(plan, 256, &nbits);
            const int e = carry + nbits;   // past the end-of-block code
            if (last) nbits = ((e + 7) & ~7) - carry;
            else {
                // 000, the pad, 00 00 FF FF
                tail_at = (uint32_t)(((e + 3 + 7) & ~7) + 16 - carry);
                nbits = (int)tail_at + 16;
            }
        }
        uint32_t tot;
        const int off = carry + (int)png_scan((uint32_t)nbits, &tot, wsum, tid);
        const int total = carry + (int)tot;
        for (;;) {
            if (nbits && off < win0 + kPngWinBits && off + nbits > win0) {
                if (r < rounds) png_deposit(win, win0, off, bits, nbits);
                else {
                    png_deposit(win, win0, off, bits, 0);
                    if (tail_at) png_deposit(win, win0, off + (int)tail_at, 0xFFFFu, 16);
                }
            }
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
    if (tid == 0) lens[slot] = (uint32_t)(carry >> 3);
}

// One workgroup a frame: offs[b] = the chunk bytes of bands 0 .. b - 1, the frame's Adler-32
// from the bands' sums, d_bytes = the file's length or CG_E_CAPACITY when the slot is shorter.
__global__ __launch_bounds__(kPngThreads) void png_enc_scan_kernel(const uint32_t *__restrict__ lens,
                                                                  const uint32_t *__restrict__ adler, PngShape s,
                                                                  size_t slot_bytes, unsigned long long *__restrict__ offs,
                                                                  uint32_t *__restrict__ adler32,
                                                                  int64_t *__restrict__ d_bytes)
{
    __shared__ uint32_t wsum[kPngWaves];
    const int tid = (int)threadIdx.x;
    const size_t f = blockIdx.x;
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < s.nb; b0 += kPngThreads) {
        const int b = b0 + tid;
        // a chunk is at most 4.2 MB and 1024 of them pass 32 bits: the quarters and the rests are summed apart
        const uint32_t v = b < s.nb ? lens[f * (size_t)s.nb + b] + 12u + (b == s.nb - 1 ? 4u : 0u) : 0u;
        uint32_t tot;
        const uint32_t ex = png_scan(v >> 2, &tot, wsum, tid);
        uint32_t tot2;
        const uint32_t ex2 = png_scan(v & 3u, &tot2, wsum, tid);
        if (b < s.nb) offs[f * (size_t)s.nb + b] = carry + 4ull * ex + ex2;
        carry += 4ull * tot + tot2;
    }
    if (tid == 0) {
        uint32_t a = 1u, b = 0u;
        for (int k = 0; k < s.nb; ++k) {
            const uint32_t nk = png_band_bytes(s, k) % kAdlerMod;
            const uint32_t s1 = adler[2 * (f * (size_t)s.nb + k)], s2 = adler[2 * (f * (size_t)s.nb + k) + 1];
            b = (uint32_t)((b + (unsigned long long)nk * a + s2) % kAdlerMod);
            a = (a + s1) % kAdlerMod;
        }
        adler32[f] = (b << 16) | a;
        const unsigned long long total = (unsigned long long)kPngFixedBytes + carry;
        d_bytes[f] = total <= (unsigned long long)slot_bytes ? (int64_t)total : (int64_t)CG_E_CAPACITY;
    }
}

struct PngFixed {
    uint8_t b[36];   // signature and IHDR (33)
};

// One workgroup per (band, frame): the band's chunk to its place in the slot -- length, IDAT, the
// staged bytes (the Adler-32 after the last band's), the CRC-32 -- the signature and IHDR with the
// first and IEND with the last.  A lane takes the CRC of a run of the staged bytes; the runs'
// CRCs are joined by multiplying each by x^(8 * the bytes after it).  A frame that does not fit
// writes nothing.
__global__ __launch_bounds__(kPngThreads) void png_enc_gather_kernel(const uint8_t *__restrict__ stage, size_t stage_cap,
                                                                    const uint32_t *__restrict__ lens,
                                                                    const unsigned long long *__restrict__ offs,
                                                                    const uint32_t *__restrict__ adler32, int nb,
                                                                    PngFixed fixed, uint8_t *__restrict__ d_out,
                                                                    size_t slot_bytes, const int64_t *__restrict__ d_bytes)
{
    __shared__ uint32_t table[256];
    __shared__ uint32_t x2n[32];
    __shared__ uint32_t crc_all;
    const int tid = (int)threadIdx.x;
    const int band = (int)blockIdx.x;
    const size_t f = blockIdx.y;
    if (d_bytes[f] < 0) return;
    if (tid < 256) table[tid] = png_crc_byte((uint32_t)tid, 0);
    if (tid < 32) x2n[tid] = d_png_x2n.t[tid];
    if (tid == 0) crc_all = 0u;
    __syncthreads();
    uint8_t *o = d_out + f * slot_bytes;
    if (band == 0)
        for (int j = tid; j < 33; j += kPngThreads) o[j] = fixed.b[j];
    const uint32_t len = lens[f * (size_t)nb + band];
    const bool last = band == nb - 1;
    const size_t at = 33 + (size_t)offs[f * (size_t)nb + band];
    const uint8_t *src = stage + (f * (size_t)nb + (size_t)band) * stage_cap;
    const uint32_t dlen = len + (last ? 4u : 0u);
    if (tid == 0) {
        o[at + 0] = (uint8_t)(dlen >> 24), o[at + 1] = (uint8_t)(dlen >> 16), o[at + 2] = (uint8_t)(dlen >> 8);
        o[at + 3] = (uint8_t)dlen;
        o[at + 4] = 'I', o[at + 5] = 'D', o[at + 6] = 'A', o[at + 7] = 'T';
    }
    for (uint32_t j = (uint32_t)tid; j < len; j += kPngThreads) o[at + 8 + j] = src[j];
    // a lane's run: seg bytes, a multiple of 4 (the staging area is 256-byte aligned)
    const uint32_t seg = ((len + kPngThreads - 1) / kPngThreads + 3u) & ~3u;
    const uint32_t b0 = (uint32_t)tid * seg < len ? (uint32_t)tid * seg : len;
    const uint32_t b1 = b0 + seg < len ? b0 + seg : len;
    uint32_t part = 0u;
    if (b1 > b0) {
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t j = b0; j < b1; j += 4) {
            const uint32_t wd = *(const uint32_t *)(src + j);
            const int nby = b1 - j < 4u ? (int)(b1 - j) : 4;
            for (int k = 0; k < nby; ++k) c = table[(c ^ (wd >> (8 * k))) & 255u] ^ (c >> 8);
        }
        part = png_crc_shift(c ^ 0xFFFFFFFFu, len - b1, x2n);
    }
    if (tid == 0) part ^= png_crc_shift(kCrcIdat, len, x2n);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) part ^= __shfl_xor(part, k, 64);
    if ((tid & 63) == 0 && part) atomicXor(&crc_all, part);
    __syncthreads();
    if (tid == 0) {
        uint32_t c = crc_all;
        size_t p = at + 8 + len;
        if (last) {
            const uint32_t ad = adler32[f];
            c ^= 0xFFFFFFFFu;
            for (int k = 3; k >= 0; --k) {
                const uint32_t by = (ad >> (8 * k)) & 255u;
                o[p++] = (uint8_t)by;
                c = table[(c ^ by) & 255u] ^ (c >> 8);
            }
            c ^= 0xFFFFFFFFu;
        }
        o[p + 0] = (uint8_t)(c >> 24), o[p + 1] = (uint8_t)(c >> 16), o[p + 2] = (uint8_t)(c >> 8), o[p + 3] = (uint8_t)c;
        if (last)
            for (int k = 0; k < 12; ++k) o[p + 4 + k] = kIend[k];
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

using namespace cg;

// ---- host-only (no device, no context) ------------------------------------------------------
extern "C" long long cg_image_png_bound(int width, int height, int colour)
{
    const cg_png_params p{colour, CG_PNG_FILTER_ADAPTIVE};
    if (!params_ok(width, height, &p)) return CG_E_INVALID;
    return (long long)file_bound(png_shape(width, height, colour));
}

extern "C" int cg_image_png_enc_limits(int *threads, int *window_bytes)
{
    if (threads) *threads = kPngThreads;
    if (window_bytes) *window_bytes = kPngWinBytes;
    return CG_OK;
}

extern "C" int cg_image_png_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *lengths)
{
    if (!freq || !lengths || n < 1 || n > kPngLitLen || limit < 1 || limit > 15) return CG_E_INVALID;
    PngHuffWork w;
    const int m = png_sort_symbols(freq, n, w.order);
    unsigned long long sum = 0;
    for (int s = 0; s < n; ++s) sum += freq[s];
    if (m > (1 << limit) || sum >> 32) return CG_E_INVALID;
    png_lengths_from_order(freq, n, m, limit, lengths, w);
    return CG_OK;
}

extern "C" int cg_image_encode_png_host(const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                                        const cg_png_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!params_ok(width, height, params) || !argb || !n || (!out && cap)) return CG_E_INVALID;
    const size_t stride = row_stride_pixels ? row_stride_pixels : (size_t)width;
    if (stride < (size_t)width) return CG_E_INVALID;
    const PngShape s = png_shape(width, height, params->colour);
    HostSink sink{out, cap};
    uint8_t fixed[33];
    write_fixed(s, fixed);
    for (int i = 0; i < 33; ++i) sink.byte(fixed[i]);
    const int nbytes = s.w * s.bpp;
    std::vector<uint8_t> band((size_t)kPngBandRows * s.rb), data;
    std::vector<uint32_t> freq(kPngLitLen);
    PngPlan plan;
    PngHuffWork work;
    uint32_t ad_a = 1u, ad_b = 0u;
    for (int b = 0; b < s.nb; ++b) {
        const uint32_t nbnd = png_band_bytes(s, b);
        const bool last = b == s.nb - 1;
        for (int y = b * kPngBandRows; y < std::min(s.h, (b + 1) * kPngBandRows); ++y) {
            const uint32_t *cur = argb + (size_t)y * stride, *up = y ? cur - stride : nullptr;
            int type = params->filter;
            if (type == CG_PNG_FILTER_ADAPTIVE) {
                uint32_t sum[5] = {0, 0, 0, 0, 0};
                for (int x = 0; x < nbytes; ++x) {
                    int fv[5];
                    png_filter_all(cur, up, x, s.bpp, fv);
                    for (int t = 0; t < 5; ++t) sum[t] += png_abs8(fv[t]);
                }
                type = 0;
                for (int t = 1; t < 5; ++t)
                    if (sum[t] < sum[type]) type = t;
            }
            uint8_t *row = band.data() + (size_t)(y - b * kPngBandRows) * s.rb;
            row[0] = (uint8_t)type;
            for (int x = 0; x < nbytes; ++x) row[1 + x] = (uint8_t)png_filter_byte(type, cur, up, x, s.bpp);
        }
        for (uint32_t i = 0; i < nbnd; ++i) {
            ad_a = (ad_a + band[i]) % kAdlerMod;
            ad_b = (ad_b + ad_a) % kAdlerMod;
        }
        std::fill(freq.begin(), freq.end(), 0u);
        freq[256] = 1;
        host_tokens(band.data(), nbnd, [&](int kind, int byte, int len) {
            int eb, ev;
            ++freq[kind == 1 ? byte : png_len_symbol(len, &eb, &ev)];
        });
        const int m = png_sort_symbols(freq.data(), kPngLitLen, work.order);
        png_make_plan(freq.data(), m, plan, work);
        data.clear();
        if (b == 0) data.push_back(0x78), data.push_back(0x01);
        if (plan.dyn_bits >= png_stored_bits(nbnd)) {
            const uint32_t nblk = png_stored_blocks(nbnd);
            for (uint32_t k = 0; k < nblk; ++k) {
                const uint32_t l = std::min<uint32_t>(kPngMaxStored, nbnd - k * kPngMaxStored);
                data.push_back((uint8_t)(last && k == nblk - 1 ? 1 : 0));
                data.push_back((uint8_t)(l & 255u)), data.push_back((uint8_t)(l >> 8));
                data.push_back((uint8_t)(~l & 255u)), data.push_back((uint8_t)((~l >> 8) & 255u));
                data.insert(data.end(), band.begin() + (size_t)k * kPngMaxStored, band.begin() + (size_t)k * kPngMaxStored + l);
            }
        } else {
            HostBits w{data};
            png_put_header(plan, last ? 1 : 0, [&](uint32_t bits, int l) { w.put(bits, l); });
            host_tokens(band.data(), nbnd, [&](int kind, int byte, int len) {
                int nb2;
                const uint32_t bits = kind == 1 ? png_literal_bits(plan, byte, &nb2) : png_match_bits(plan, len, &nb2);
                w.put(bits, nb2);
            });
            w.put(plan.ll_code[256], plan.ll_len[256]);
            if (!last) w.put(0u, 3);
            w.align();
        }
        if (!last) {
            if (plan.dyn_bits >= png_stored_bits(nbnd)) data.push_back(0);   // the empty block's 000 and pad
            data.push_back(0), data.push_back(0), data.push_back(0xFF), data.push_back(0xFF);
        } else {
            const uint32_t ad = (ad_b << 16) | ad_a;
            for (int k = 3; k >= 0; --k) data.push_back((uint8_t)(ad >> (8 * k)));
        }
        sink.be32((uint32_t)data.size());
        uint32_t c = 0xFFFFFFFFu;
        for (char ch : {'I', 'D', 'A', 'T'}) sink.byte(ch), c = png_crc_byte(c, (uint8_t)ch);
        for (uint8_t v : data) sink.byte(v), c = png_crc_byte(c, v);
        sink.be32(c ^ 0xFFFFFFFFu);
    }
    for (int i = 0; i < 12; ++i) sink.byte(kIend[i]);
    *n = sink.n;
    return sink.n > cap ? CG_E_CAPACITY : CG_OK;
}

// ---- device ---------------------------------------------------------------------------------
extern "C" int cg_image_encode_png_device(cg_ctx *c, const uint32_t *d_argb, int width, int height, int n_frames,
                                          size_t frame_stride, const cg_png_params *params, uint8_t *d_out,
                                          size_t slot_bytes, int64_t *d_bytes, void *stream)
{
    if (!c || n_frames < 0 || !params_ok(width, height, params)) return CG_E_INVALID;
    if (n_frames == 0) return CG_OK;
    const size_t px = (size_t)width * height;
    if (!frame_stride) frame_stride = px;
    if (!d_argb || ((uintptr_t)d_argb & 3) || !d_out || !d_bytes || ((uintptr_t)d_bytes & 7) || frame_stride < px)
        return CG_E_INVALID;
    const PngShape s = png_shape(width, height, params->colour);
    PngFixed fixed{};
    write_fixed(s, fixed.b);
    // a band longer than the slot belongs to a frame that does not fit: its staging area need not
    // hold more than the slot (the band kernel stops storing at stage_cap and counts on)
    const size_t stage_cap = align256(std::max<size_t>(std::min(band_bound(png_band_bytes(s, 0)) + 2, slot_bytes), 1));
    const int chunk = std::min(n_frames, kPngChunkFrames);
    const size_t frame_bytes = (size_t)s.h * s.rb;
    const size_t nbands = (size_t)chunk * s.nb;
    const size_t filt_b = align256((size_t)chunk * frame_bytes + 4), lens_b = align256(nbands * 4),
                 adl_b = align256(nbands * 8), offs_b = align256(nbands * 8), a32_b = align256((size_t)chunk * 4),
                 stage_b = nbands * stage_cap;
    CG_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipError_t e = hipSuccess;
    uint8_t *scratch = static_cast<uint8_t *>(ctx_png_buf(c, 0, filt_b + lens_b + adl_b + offs_b + a32_b + stage_b, &e));
    if (!scratch) return ctx_fail(c, e, "alloc png encoder scratch");
    uint8_t *filt = scratch;
    uint32_t *lens = (uint32_t *)(scratch + filt_b);
    uint32_t *adl = (uint32_t *)(scratch + filt_b + lens_b);
    unsigned long long *offs = (unsigned long long *)(scratch + filt_b + lens_b + adl_b);
    uint32_t *a32 = (uint32_t *)(scratch + filt_b + lens_b + adl_b + offs_b);
    uint8_t *stage = scratch + filt_b + lens_b + adl_b + offs_b + a32_b;
    hipStream_t st = stream ? (hipStream_t)stream : ctx_stream(c);
    for (int f0 = 0; f0 < n_frames; f0 += kPngChunkFrames) {
        const unsigned nf = (unsigned)std::min(kPngChunkFrames, n_frames - f0);
        kt_launch(KT_PNG_FILTER, png_enc_filter_kernel, dim3((unsigned)s.h, nf), dim3(kPngFilterThreads), 0, st,
                           d_argb + (size_t)f0 * frame_stride, frame_stride, s, params->filter, filt, frame_bytes);
        kt_launch(KT_PNG_BAND, png_enc_band_kernel, dim3((unsigned)s.nb, nf), dim3(kPngThreads), 0, st, (const uint8_t *)filt,
                           frame_bytes, s, stage, stage_cap, lens, adl);
        kt_launch(KT_PNG_SCAN, png_enc_scan_kernel, dim3(nf), dim3(kPngThreads), 0, st, (const uint32_t *)lens,
                           (const uint32_t *)adl, s, slot_bytes, offs, a32, d_bytes + f0);
        kt_launch(KT_PNG_GATHER, png_enc_gather_kernel, dim3((unsigned)s.nb, nf), dim3(kPngThreads), 0, st,
                           (const uint8_t *)stage, stage_cap, (const uint32_t *)lens, (const unsigned long long *)offs,
                           (const uint32_t *)a32, s.nb, fixed, d_out + (size_t)f0 * slot_bytes, slot_bytes,
                           (const int64_t *)(d_bytes + f0));
    }
    CG_TRY(c, hipGetLastError(), "png encoder launch");
    return CG_OK;
}

extern "C" int cg_image_encode_png(cg_ctx *c, const uint32_t *argb, int width, int height, size_t row_stride_pixels,
                                   const cg_png_params *params, uint8_t *out, size_t cap, size_t *n)
{
    if (!c || !params_ok(width, height, params) || !argb || !n || (!out && cap)) return CG_E_INVALID;
    const size_t stride = row_stride_pixels ? row_stride_pixels : (size_t)width;
    if (stride < (size_t)width) return CG_E_INVALID;
    const size_t px_b = align256((size_t)width * height * 4);
    const size_t bound = file_bound(png_shape(width, height, params->colour));
    CG_TRY(c, hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipError_t e = hipSuccess;
    uint8_t *io = static_cast<uint8_t *>(ctx_png_buf(c, 1, px_b + 256 + bound, &e));
    if (!io) return ctx_fail(c, e, "alloc png encoder frame");
    hipStream_t st = ctx_stream(c);
    CG_TRY(c, hipMemcpy2DAsync(io, (size_t)width * 4, argb, stride * 4, (size_t)width * 4, (size_t)height,
                               hipMemcpyHostToDevice, st),
           "png frame upload");
    int64_t *d_bytes = (int64_t *)(io + px_b);
    uint8_t *d_file = io + px_b + 256;
    if (int rc = cg_image_encode_png_device(c, (const uint32_t *)io, width, height, 1, 0, params, d_file, bound, d_bytes, st))
        return rc;
    int64_t len = 0;
    CG_TRY(c, hipMemcpyAsync(&len, d_bytes, 8, hipMemcpyDeviceToHost, st), "png length download");
    CG_TRY(c, hipStreamSynchronize(st), "png encode");
    if (len < 0) return ctx_invalid(c, "png encoder: a file longer than its bound");
    *n = (size_t)len;
    if ((size_t)len > cap) return CG_E_CAPACITY;
    CG_TRY(c, hipMemcpy(out, d_file, (size_t)len, hipMemcpyDeviceToHost), "png file download");
    return CG_OK;
}
