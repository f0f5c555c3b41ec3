// cg_bloom.h -- the arithmetic of the bloom pyramid (cg_bloom.hip's kernels and the host-only
// cg_hdr_bloom* entry points share it): bright pass, level sizes, 2 x 2 box, the five-tap blur,
// the bilinear up-sample and the composite before the tone curve.  Every function is integer
// arithmetic, a select or single IEEE float32 operations in the order written (include/cg_render.h
// states the contract); no FMA may be formed (-ffp-contract=off, as cg_math.h).  Selects are
// ternaries, never fminf / fmaxf: a NaN takes the branch the comparison's `false` names.
#pragma once

#include <stddef.h>

#include "cg_hdr.h"

namespace cg {

constexpr int kBloomMaxLevels = CG_BLOOM_MAX_LEVELS;

// three channels of a pyramid pixel (the fourth is +0.0f wherever one is stored)
struct Bloom3 {
    float x, y, z;
};

// b of one channel: clamp0, scale, threshold, clamp to [0, cap].  Finite whatever c and s hold.
CG_HD float bloom_bright(float c, float s, float threshold, float cap)
{
    const float c0 = c > 0.0f ? c : 0.0f;
    const float v = c0 * s;
    const float e = v - threshold;
    const float b = e > 0.0f ? e : 0.0f;
    return b < cap ? b : cap;
}
// of a CG_PIX_RGBA_F32 pixel: an uncovered one, !(w > 0), is dark
CG_HD Bloom3 bloom_bright_pixel(float x, float y, float z, float w, float s, float threshold, float cap)
{
    const bool cov = w > 0.0f;
    Bloom3 b;
    b.x = cov ? bloom_bright(x, s, threshold, cap) : 0.0f;
    b.y = cov ? bloom_bright(y, s, threshold, cap) : 0.0f;
    b.z = cov ? bloom_bright(z, s, threshold, cap) : 0.0f;
    return b;
}

// 0.25f * ((p00 + p10) + (p01 + p11)): p00 p10 the upper row
CG_HD float bloom_box(float p00, float p10, float p01, float p11)
{
    const float a = p00 + p10;
    const float b = p01 + p11;
    return 0.25f * (a + b);
}

// (a * 0.0625f + q * 0.25f) + t(0) * 0.375f with a = t(-2) + t(2), q = t(-1) + t(1)
CG_HD float bloom_blur(float tm2, float tm1, float t0, float tp1, float tp2)
{
    const float a = tm2 + tp2;
    const float q = tm1 + tp1;
    const float pa = a * 0.0625f;
    const float pq = q * 0.25f;
    const float pc = t0 * 0.375f;
    return (pa + pq) + pc;
}

// (0.5625f * u(cx, cy) + 0.1875f * u(nx, cy)) + (0.1875f * u(cx, ny) + 0.0625f * u(nx, ny))
CG_HD float bloom_up(float ucc, float unc, float ucn, float unn)
{
    const float a = 0.5625f * ucc;
    const float b = 0.1875f * unc;
    const float c = 0.1875f * ucn;
    const float d = 0.0625f * unn;
    return (a + b) + (c + d);
}
// the near and the far tap of fine coordinate X in a coarse plane n wide
CG_HD int bloom_up_near(int X) { return X >> 1; }
CG_HD int bloom_up_far(int X, int n)
{
    const int c = X >> 1;
    return (X & 1) ? (c + 1 < n - 1 ? c + 1 : n - 1) : (c - 1 > 0 ? c - 1 : 0);
}

// tone(op, base * s + intensity * g) of one channel
CG_HD float bloom_composite(float base, float s, float intensity, float g, int op, float white2)
{
    const float v = base * s;
    const float m = intensity * g;
    const float v2 = v + m;
    return hdr_tone(op, v2, white2);
}
// a pixel's word: rule RT packs every pixel from its channels as they are, rule RAST clamps each
// channel at 0 first and gives an uncovered pixel 0u
CG_HD unsigned bloom_pack(float x, float y, float z, float w, Bloom3 g, float s, float intensity, int rule, int op,
                          float white2)
{
    const bool rast = rule == CG_BLOOM_RULE_RAST;
    const float bx = rast ? hdr_clamp0(x) : x, by = rast ? hdr_clamp0(y) : y, bz = rast ? hdr_clamp0(z) : z;
    const unsigned px = put_pixel(v3(bloom_composite(bx, s, intensity, g.x, op, white2),
                                     bloom_composite(by, s, intensity, g.y, op, white2),
                                     bloom_composite(bz, s, intensity, g.z, op, white2)));
    return rast && !(w > 0.0f) ? 0u : px;
}

// Level sizes and offsets: w[0] x h[0] the frame, w[k] = (w[k - 1] + 1) / 2; level k of a pyramid
// starts off[k] pixels in (off[1] = 0), and `total` pixels hold all of it.
struct BloomLayout {
    int levels;
    int w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
    size_t off[kBloomMaxLevels + 1];
    size_t total;
};
inline bool bloom_layout(int width, int height, int levels, BloomLayout *L)
{
    if (width <= 0 || height <= 0 || levels < 1 || levels > kBloomMaxLevels) return false;
    L->levels = levels;
    L->w[0] = width, L->h[0] = height, L->off[0] = 0;
    size_t run = 0;
    for (int k = 1; k <= levels; ++k) {
        L->w[k] = (L->w[k - 1] + 1) / 2;
        L->h[k] = (L->h[k - 1] + 1) / 2;
        L->off[k] = run;
        run += (size_t)L->w[k] * L->h[k];
    }
    L->total = run;
    return true;
}

inline bool bloom_params_ok(const cg_hdr_bloom_params *b)
{
    return b && b->levels >= 1 && b->levels <= kBloomMaxLevels && b->threshold >= 0.0f && b->cap > 0.0f &&
           b->cap <= 0x1p+64f && b->intensity >= 0.0f && b->intensity <= 0x1p+32f;   // a NaN fails its comparison
}
inline bool bloom_rule_ok(int rule) { return rule == CG_BLOOM_RULE_RT || rule == CG_BLOOM_RULE_RAST; }

}  // namespace cg
