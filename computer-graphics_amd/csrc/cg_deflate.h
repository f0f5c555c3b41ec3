// cg_deflate.h -- deflating one band of bytes with cg_png_enc.h's rules, shared by the PNG encoder
// (cg_png_enc.hip) and the EXR encoder (cg_exr_enc.hip).  Host: the tokens in order, a bit writer
// and a byte sink that counts past its capacity.  Device: a workgroup of 1024 lanes walks the
// band in pieces of one byte a lane, finds each byte's token from ballots, scans the tokens' bit
// counts and deposits their bits into a window of the band's bit string in LDS.
#pragma once

#include <vector>

#include "cg_png_enc.h"

namespace cg {

constexpr uint32_t kAdlerMod = 65521u;

// bits lowest first into bytes
struct HostBits {
    std::vector<uint8_t> &v;
    uint32_t acc = 0;
    int fill = 0;
    void put(uint32_t bits, int len)
    {
        for (int i = 0; i < len; ++i) {
            acc |= ((bits >> i) & 1u) << fill;
            if (++fill == 8) v.push_back((uint8_t)acc), acc = 0, fill = 0;
        }
    }
    void align()
    {
        if (fill) v.push_back((uint8_t)acc), acc = 0, fill = 0;
    }
};

// the tokens of a band in order, as the contract words them: fn(kind, byte, len)
template <class Fn>
void host_tokens(const uint8_t *b, uint32_t n, Fn fn)
{
    for (uint32_t i = 0; i < n;) {
        uint32_t r = 1;
        while (i + r < n && b[i + r] == b[i]) ++r;
        if (r < 4) {
            for (uint32_t k = 0; k < r; ++k) fn(1, b[i], 0);
        } else {
            fn(1, b[i], 0);
            uint32_t rem = r - 1;
            for (; rem >= (uint32_t)kPngMaxMatch; rem -= kPngMaxMatch) fn(2, b[i], kPngMaxMatch);
            if (rem >= 3) fn(2, b[i], (int)rem);
            else
                for (uint32_t k = 0; k < rem; ++k) fn(1, b[i], 0);
        }
        i += r;
    }
}

// a byte sink that counts past its capacity without writing there
struct HostSink {
    uint8_t *out;
    size_t cap, n = 0;
    void byte(int b)
    {
        if (n < cap) out[n] = (uint8_t)b;
        ++n;
    }
    void be32(uint32_t v)
    {
        for (int k = 3; k >= 0; --k) byte((int)(v >> (8 * k)) & 255);
    }
};

constexpr int kPngThreads = 1024;                 // a band workgroup: a piece is one byte a lane
constexpr int kPngWaves = kPngThreads / 64;
constexpr int kPngFilterThreads = 256;
constexpr int kPngWinBytes = 16384;               // a band workgroup's window of its bit string
constexpr int kPngWinWords = kPngWinBytes / 4;
constexpr int kPngWinBits = kPngWinBytes * 8;
constexpr int kPngChunkFrames = 8;                // frames the context's scratch holds
constexpr uint32_t kNone = 0xFFFFFFFFu;

// Exclusive sum of v over the workgroup (kPngThreads lanes, wave 64), *total the whole sum.
// Ends with a barrier: wsum may be reused at once.
__device__ __forceinline__ uint32_t png_scan(uint32_t v, uint32_t *total, uint32_t *wsum, int tid)
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
    for (int i = 0; i < kPngWaves; ++i) {
        const uint32_t w = wsum[i];
        base += i < wv ? w : 0u;
        tot += w;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

struct PngBandShared {
    uint32_t wfirst[kPngWaves], wlast[kPngWaves];   // a wave's first and last run start of the piece
    uint32_t look;                                  // the first run start at or after the piece's end
    uint32_t carry;                                 // where the run that enters the piece began
};

// The token of byte pos0 + tid of a band of n bytes (png_token's kinds; 0 beyond the band).  Three
// barriers; every lane of the workgroup calls it.
__device__ __forceinline__ int png_piece_token(const uint8_t *__restrict__ src, uint32_t n, uint32_t pos0, int tid,
                                               PngBandShared &sh, int *byte, int *len)
{
    const int lane = tid & 63, wv = tid >> 6;
    const uint32_t i = pos0 + (uint32_t)tid;
    const bool valid = i < n;
    const int v = valid ? (int)src[i] : 0;
    const bool start = !valid || i == 0u || v != (int)src[i - 1u];
    const unsigned long long mask = __ballot(start);
    const uint32_t wbase = pos0 + (uint32_t)(wv * 64);
    if (lane == 0) {
        sh.wfirst[wv] = mask ? wbase + (uint32_t)(__ffsll((long long)mask) - 1) : kNone;
        sh.wlast[wv] = mask ? wbase + (uint32_t)(63 - __clzll((long long)mask)) : kNone;
    }
    const uint32_t end = pos0 + (uint32_t)kPngThreads;
    if (tid == 0) sh.look = end + (uint32_t)kPngMaxMatch;
    __syncthreads();
    if (tid < kPngMaxMatch) {
        const uint32_t p = end + (uint32_t)tid;
        if (p >= n || src[p] != src[p - 1u]) atomicMin(&sh.look, p);
    }
    __syncthreads();
    uint32_t rs = kNone, nx = kNone;
    const unsigned long long below = lane == 63 ? mask : mask & ((2ull << lane) - 1ull);
    if (below) rs = wbase + (uint32_t)(63 - __clzll((long long)below));
    else {
        for (int w = wv - 1; w >= 0 && rs == kNone; --w) rs = sh.wlast[w];
        if (rs == kNone) rs = sh.carry;
    }
    const unsigned long long above = lane == 63 ? 0ull : mask >> (lane + 1);
    if (above) nx = i + (uint32_t)__ffsll((long long)above);
    else {
        for (int w = wv + 1; w < kPngWaves && nx == kNone; ++w) nx = sh.wfirst[w];
        if (nx == kNone) nx = sh.look;
    }
    __syncthreads();
    if (tid == kPngThreads - 1) sh.carry = rs;
    *byte = v;
    *len = 0;
    return valid ? png_token(i - rs, nx - i, len) : 0;
}

// `bits` (len of them, len <= 32, lowest first) at bit p of the band's string, into the window
// that starts at bit win0: the parts that fall outside the window are another round's
__device__ __forceinline__ void png_deposit(uint32_t *win, int win0, int p, uint32_t bits, int len)
{
    (void)len;
    const int rp = p - win0;
    const int wi = rp >> 5, sh = rp & 31;
    const unsigned long long v = (unsigned long long)bits << sh;
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (lo && wi >= 0 && wi < kPngWinWords) atomicOr(&win[wi], lo);
    if (hi && wi + 1 >= 0 && wi + 1 < kPngWinWords) atomicOr(&win[wi + 1], hi);
}

// the first nbytes of the window to out[at ..]; nothing at or past cap is written
__device__ __forceinline__ void png_flush(const uint32_t *win, int nbytes, uint8_t *__restrict__ out, size_t cap, size_t at,
                                          int tid)
{
    for (int w = tid; 4 * w < nbytes; w += kPngThreads) {
        const uint32_t wd = win[w];
        const size_t o = at + 4 * (size_t)w;
        if (4 * w + 4 <= nbytes && o + 4 <= cap) *(uint32_t *)(out + o) = wd;
        else
            for (int k = 0; k < 4; ++k)
                if (4 * w + k < nbytes && o + k < cap) out[o + k] = (uint8_t)(wd >> (8 * k));
    }
}

}  // namespace cg
