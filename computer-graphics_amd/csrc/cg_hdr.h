// cg_hdr.h -- the arithmetic of the exposure chain (cg_hdr.hip's kernels and the host-only
// cg_hdr_* entry points share it): luminance, histogram bin, bin edge, a frame's target scale,
// the adaptation step and the tone curves.  Every function is integer arithmetic or single IEEE
// float32 operations in the order written; no FMA may be formed (-ffp-contract=off, as cg_math.h).
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/cg_render.h"
#include "cg_math.h"

namespace cg {

constexpr int kHdrBins = CG_HDR_BINS;
constexpr int kHdrBinBase = 888;   // (bits of 2^-16) >> 20: bin 0 starts at 2^-16, eight bins an octave

CG_HD uint32_t hdr_bits(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
#endif
}
CG_HD float hdr_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float v;
    memcpy(&v, &u, 4);
    return v;
#endif
}

// five float32 operations: (0.2126 x + 0.7152 y) + 0.0722 z
CG_HD float hdr_luminance(float x, float y, float z)
{
    const float a = 0.2126f * x, b = 0.7152f * y, c = 0.0722f * z;
    return (a + b) + c;
}

// counted: L > 0 (true for +inf; false for NaN, +-0 and negatives)
CG_HD bool hdr_counted(float L) { return L > 0.0f; }

// bin of a counted L: clamp((bits >> 20) - 888, 0, 255)
CG_HD int hdr_bin_of_bits(uint32_t bits)
{
    const int b = (int)(bits >> 20) - kHdrBinBase;
    return b < 0 ? 0 : (b > kHdrBins - 1 ? kHdrBins - 1 : b);
}
CG_HD int hdr_bin(float L) { return hdr_counted(L) ? hdr_bin_of_bits(hdr_bits(L)) : -1; }

// upper edge of bin b (0 .. 255): the float with bits (888 + b + 1) << 20; bin 255: 2^16
CG_HD float hdr_bin_edge(int b) { return hdr_float((uint32_t)(kHdrBinBase + b + 1) << 20); }

// k of a frame: max(1, (total * permille + 999) / 1000), 64-bit
CG_HD uint64_t hdr_rank(uint64_t total, int permille)
{
    const uint64_t k = (total * (uint64_t)permille + 999u) / 1000u;
    return k < 1u ? 1u : k;
}

// t_f from the bin the running sum reaches k in (total 0: 1.0f), clamped
CG_HD float hdr_target_scale(uint64_t total, int bin, const cg_hdr_exposure_params &p)
{
    const float t = total == 0 ? 1.0f : p.target / hdr_bin_edge(bin);
    return fminf(fmaxf(t, p.scale_min), p.scale_max);
}

// s_f = s_{f-1} + (t_f - s_{f-1}) * rate: a subtract, a multiply, an add
CG_HD float hdr_adapt(float s_prev, float t, float rate)
{
    const float d = t - s_prev;
    const float m = d * rate;
    return s_prev + m;
}

CG_HD float hdr_tone(int op, float v, float white2)
{
    if (op == CG_TONE_REINHARD) return v / (1.0f + v);
    if (op == CG_TONE_REINHARD_WHITE) {
        const float q = v / white2;
        const float n = v * (1.0f + q);
        return n / (1.0f + v);
    }
    return v;   // CG_TONE_LINEAR
}

// put_pixel(tone(c * s)) per channel
CG_HD unsigned hdr_pack(float x, float y, float z, float s, int op, float white2)
{
    return put_pixel(v3(hdr_tone(op, x * s, white2), hdr_tone(op, y * s, white2), hdr_tone(op, z * s, white2)));
}

// The rasteriser's pack (cg_rast_tonemap_pack_device, cg_rast_pack_pixel).  Border rule: a pixel
// with !(w > 0) is one the reference never gave PutPixelSDL, so its word is 0.  Clamp rule: each
// channel is c > 0 ? c : 0 before the scale (a NaN gives 0), since the reference shows a negative
// channel as black and Reinhard's v / (1 + v) has a pole at -1.
CG_HD float hdr_clamp0(float c) { return c > 0.0f ? c : 0.0f; }
CG_HD unsigned hdr_rast_pack(float x, float y, float z, float w, float s, int op, float white2)
{
    const unsigned px = hdr_pack(hdr_clamp0(x), hdr_clamp0(y), hdr_clamp0(z), s, op, white2);
    return w > 0.0f ? px : 0u;   // a select after the pack: no lane leaves the kernel's straight line
}

inline bool hdr_params_ok(const cg_hdr_exposure_params *p)
{
    return p && p->permille >= 0 && p->permille <= 1000 && p->rate >= 0.0f && p->rate <= 1.0f &&
           p->scale_min <= p->scale_max;   // a NaN fails its comparison
}
inline bool hdr_tone_ok(int op, float white2)
{
    if (op == CG_TONE_LINEAR || op == CG_TONE_REINHARD) return true;
    return op == CG_TONE_REINHARD_WHITE && white2 > 0.0f;
}

}  // namespace cg
