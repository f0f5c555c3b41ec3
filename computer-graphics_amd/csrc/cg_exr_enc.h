// cg_exr_enc.h -- the arithmetic of the OpenEXR encoder (cg_exr_enc.hip's kernels and the
// host-only cg_image_encode_exr_host share it): the float -> half rule, the header, the shape of
// a file's chunks, a chunk's raw bytes from the source floats and the reordered, predicted bytes
// that ZIP deflates.  The deflate rules are cg_png_enc.h's.  Everything is integer arithmetic in
// the order written, except the one float32 product of an alpha scale other than 1
// (include/cg_render.h states the contract).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/cg_render.h"
#include "cg_math.h"

namespace cg {

constexpr int kExrZipLines = 16;          // scanlines of a ZIP chunk
constexpr int kExrMaxHeader = 331;        // the RGBA header; RGB's is 313
constexpr uint32_t kExrOne = 0x3F800000u; // an alpha scale with these bits keeps w's bits

// rule 1: float32 bits -> half bits, round to nearest even
CG_HD uint32_t exr_half_bits(uint32_t f)
{
    const uint32_t sign = (f >> 16) & 0x8000u, a = f & 0x7FFFFFFFu;
    if (a > 0x7F800000u) {   // NaN: the top of the payload, bit 0 when that is empty
        const uint32_t m = (a >> 13) & 0x3FFu;
        return sign | 0x7C00u | m | (m ? 0u : 1u);
    }
    if (a >= 0x47800000u) return sign | 0x7C00u;   // 65536 and above, inf
    if (a >= 0x38800000u) {                        // 2^-14 and above: a normal half unless it rounds up to inf
        const uint32_t r = a - 0x38000000u;        // the exponent re-biased, 127 -> 15
        uint32_t h = r >> 13;
        const uint32_t rem = r & 0x1FFFu;
        if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
        return sign | h;
    }
    if (a < 0x33000000u) return sign;              // below 2^-25: zero
    // a subnormal half: the significand in units of 2^-24
    const uint32_t e = a >> 23, m = (a & 0x7FFFFFu) | 0x800000u;
    const uint32_t shift = 126u - e;               // 14 .. 24
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u))) ++h;
    return sign | h;
}

CG_HD uint32_t exr_float_bits(float v)
{
    union {
        float f;
        uint32_t u;
    } x;
    x.f = v;
    return x.u;
}

// the shape of a file
struct ExrShape {
    int w, h, nch, bps, type, zip;   // bps: bytes a sample (2 or 4)
    int lines, nc;                   // scanlines a chunk (1 or 16), chunks
    int hdr;                         // bytes of the header
    uint32_t plane;                  // bytes of one channel of one scanline
    uint32_t rowb;                   // bytes of a scanline
    uint32_t alpha;                  // the alpha scale's bits
};
CG_HD ExrShape exr_shape(int w, int h, const cg_exr_params &p)
{
    ExrShape s;
    s.w = w, s.h = h, s.type = p.type, s.zip = p.compression == CG_EXR_ZIP ? 1 : 0;
    s.nch = p.channels == CG_EXR_RGBA ? 4 : 3;
    s.bps = p.type == CG_EXR_HALF ? 2 : 4;
    s.lines = s.zip ? kExrZipLines : 1;
    s.nc = (h + s.lines - 1) / s.lines;
    s.hdr = s.nch == 4 ? kExrMaxHeader : kExrMaxHeader - 18;
    s.plane = (uint32_t)w * (uint32_t)s.bps;
    s.rowb = s.plane * (uint32_t)s.nch;
    s.alpha = exr_float_bits(p.alpha_scale);
    return s;
}
CG_HD int exr_chunk_rows(const ExrShape &s, int k) { return s.h - k * s.lines < s.lines ? s.h - k * s.lines : s.lines; }
CG_HD uint32_t exr_chunk_bytes(const ExrShape &s, int k) { return (uint32_t)exr_chunk_rows(s, k) * s.rowb; }

// rule 1's sample: channel c (file order A B G R or B G R) of a pixel, as the file stores it
CG_HD uint32_t exr_sample(const float *px, const ExrShape &s, int c)
{
    const int comp = s.nch - 1 - c;
    float v = px[comp];
    if (comp == 3 && s.alpha != kExrOne) {
        union {
            uint32_t u;
            float f;
        } sc;
        sc.u = s.alpha;
        v = v * sc.f;
    }
    const uint32_t u = exr_float_bits(v);
    return s.type == CG_EXR_HALF ? exr_half_bits(u) : u;
}

// Where a raw byte of a chunk (rule 4) comes from.  seek() takes any position; step2() goes on
// two bytes, which never leaves a sample except at its end (a sample has 2 or 4 bytes).
struct ExrCursor {
    uint32_t line, ch, off;   // scanline of the chunk, channel, byte of the channel's plane
    CG_HD void seek(const ExrShape &s, uint32_t p)
    {
        line = p / s.rowb;
        const uint32_t q = p - line * s.rowb;
        ch = q / s.plane;
        off = q - ch * s.plane;
    }
    CG_HD void step2(const ExrShape &s)
    {
        off += 2u;
        if (off >= s.plane) {
            off -= s.plane;
            if (++ch == (uint32_t)s.nch) ch = 0u, ++line;
        }
    }
    // `rows`: the chunk's first scanline in the frame, `stride` pixels a scanline
    CG_HD uint32_t byte(const ExrShape &s, const float *rows, size_t stride) const
    {
        const uint32_t x = s.bps == 2 ? off >> 1 : off >> 2, b = off & (uint32_t)(s.bps - 1);
        return (exr_sample(rows + ((size_t)line * stride + x) * 4, s, (int)ch) >> (8u * b)) & 255u;
    }
};

// rule 5: position i of t (the even bytes, then the odd ones) in a chunk of n raw bytes
CG_HD uint32_t exr_t_pos(uint32_t n, uint32_t i) { return i < n / 2u ? 2u * i : 2u * (i - n / 2u) + 1u; }

// rule 5's d[i0 .. i0 + cnt) of a chunk of n raw bytes, cnt <= 4, from the source floats alone
CG_HD void exr_predicted(const ExrShape &s, const float *rows, size_t stride, uint32_t n, uint32_t i0, int cnt, uint8_t *d)
{
    ExrCursor c;
    uint32_t prev = 0u;
    if (i0) {
        c.seek(s, exr_t_pos(n, i0 - 1u));
        prev = c.byte(s, rows, stride);
    }
    for (int j = 0; j < cnt; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        if (j == 0 || i == n / 2u) c.seek(s, exr_t_pos(n, i));
        else c.step2(s);
        const uint32_t t = c.byte(s, rows, stride);
        d[j] = (uint8_t)(i ? (t - prev + 128u) & 255u : t);
        prev = t;
    }
}

// rule 2: the header into out[0 .. s.hdr) (host: the kernels get it as an argument)
inline int exr_put_header(const ExrShape &s, uint8_t *out)
{
    int n = 0;
    auto str = [&](const char *t) {
        for (; *t; ++t) out[n++] = (uint8_t)*t;
        out[n++] = 0;
    };
    auto i32 = [&](uint32_t v) {
        for (int k = 0; k < 4; ++k) out[n++] = (uint8_t)(v >> (8 * k));
    };
    auto attr = [&](const char *name, const char *type, uint32_t size) { str(name), str(type), i32(size); };
    out[n++] = 0x76, out[n++] = 0x2F, out[n++] = 0x31, out[n++] = 0x01;
    i32(2u);
    attr("channels", "chlist", 18u * (uint32_t)s.nch + 1u);
    const char *names[4] = {"A", "B", "G", "R"};
    for (int c = 4 - s.nch; c < 4; ++c) {
        str(names[c]);
        i32((uint32_t)s.type);
        i32(0u);   // pLinear and three reserved bytes
        i32(1u), i32(1u);
    }
    out[n++] = 0;
    attr("compression", "compression", 1u);
    out[n++] = (uint8_t)(s.zip ? CG_EXR_ZIP : CG_EXR_NONE);
    for (const char *name : {"dataWindow", "displayWindow"}) {
        attr(name, "box2i", 16u);
        i32(0u), i32(0u), i32((uint32_t)(s.w - 1)), i32((uint32_t)(s.h - 1));
    }
    attr("lineOrder", "lineOrder", 1u);
    out[n++] = 0;
    attr("pixelAspectRatio", "float", 4u);
    i32(kExrOne);
    attr("screenWindowCenter", "v2f", 8u);
    i32(0u), i32(0u);
    attr("screenWindowWidth", "float", 4u);
    i32(kExrOne);
    out[n++] = 0;
    return n;
}

}  // namespace cg
