// cg_jpeg_enc.h -- the arithmetic of the baseline JPEG encoder (cg_jpeg_enc.hip's kernels and the
// host-only cg_image_encode_jpeg_host share it): colour conversion, the 2 x 2 chroma mean, the
// forward DCT, quantisation, the Annex K tables and the code of one block.  Every function is
// int32 arithmetic in the order written, `>>` arithmetic (include/cg_render.h states the
// contract); there is no floating point anywhere in the encoder.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/cg_render.h"
#include "cg_math.h"

namespace cg {

constexpr int kJpegHeaderBytes = 629;       // SOI .. SOS, the same for every size and quality
constexpr int kJpegMaxBlockBits = 1660;     // cg_image_jpeg_bound's derivation (cg_jpeg_enc.hip)

// ---- Annex K.1, row-major; K.3 as the DHT segments carry them ----
constexpr uint8_t kJpegBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37, 56,  68,  109, 103, 77, 24, 35, 55,  64,
     81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// kJpegZigzag[k]: the row-major index of the k-th coefficient in zig-zag order
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                        {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The four code tables as the encoder looks them up: (code << 5) | length per symbol, built at
// compile time from the bits / values above (Annex C: codes of a length count up, a longer
// length continues at twice the next code).
struct JpegHuff {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};
constexpr JpegHuff jpeg_make_huff()
{
    JpegHuff h{};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kJpegDcBits[t][len - 1]; ++i) h.dc[t][k++] = (code++ << 5) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kJpegAcBits[t][len - 1]; ++i) h.ac[t][kJpegAcVals[t][k++]] = (code++ << 5) | (uint32_t)len;
            code <<= 1;
        }
    }
    return h;
}

// the geometry of a frame's scan
struct JpegShape {
    int w, h, sub;           // sub: CG_JPEG_444 or CG_JPEG_420
    int mx, my;              // MCUs across and down
    int bpm;                 // blocks of an MCU: 3 or 6
    int bw, bh;              // real Y block columns and rows: ceil(w / 8), ceil(h / 8)
};
CG_HD JpegShape jpeg_shape(int w, int h, int sub)
{
    JpegShape s;
    const int mcu = sub == CG_JPEG_420 ? 16 : 8;
    s.w = w, s.h = h, s.sub = sub;
    s.mx = (w + mcu - 1) / mcu, s.my = (h + mcu - 1) / mcu;
    s.bpm = sub == CG_JPEG_420 ? 6 : 3;
    s.bw = (w + 7) / 8, s.bh = (h + 7) / 8;
    return s;
}

// q of one table entry at a quality
CG_HD int jpeg_quant(int base, int quality)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

// sample `comp` (0 Y, 1 Cb, 2 Cr) of an ARGB8888 pixel
CG_HD int jpeg_ycc(uint32_t argb, int comp)
{
    const int r = (int)((argb >> 16) & 255u), g = (int)((argb >> 8) & 255u), b = (int)(argb & 255u);
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Sample (x, y) of component `comp`'s padded plane: x and y are in the component's own
// resolution and may lie anywhere in the padded MCU grid.  Full-resolution planes replicate the
// last column and row.  A 4:2:0 chroma sample is the biased mean of its four pixels, the
// columns replicated before the mean and the last down-sampled row after it.
CG_HD int jpeg_sample(const uint32_t *px, size_t stride, const JpegShape &s, int comp, int x, int y)
{
    if (comp == 0 || s.sub == CG_JPEG_444) {
        const int xx = x < s.w ? x : s.w - 1, yy = y < s.h ? y : s.h - 1;
        return jpeg_ycc(px[(size_t)yy * stride + xx], comp);
    }
    const int ch = (s.h + 1) / 2;
    const int cy = y < ch ? y : ch - 1;
    const int y0 = 2 * cy, y1 = 2 * cy + 1 < s.h ? 2 * cy + 1 : s.h - 1;
    const int x0 = 2 * x < s.w ? 2 * x : s.w - 1, x1 = 2 * x + 1 < s.w ? 2 * x + 1 : s.w - 1;
    const int sum = jpeg_ycc(px[(size_t)y0 * stride + x0], comp) + jpeg_ycc(px[(size_t)y0 * stride + x1], comp) +
                    jpeg_ycc(px[(size_t)y1 * stride + x0], comp) + jpeg_ycc(px[(size_t)y1 * stride + x1], comp);
    return (sum + ((x & 1) ? 2 : 1)) >> 2;
}

// Where block k of an MCU takes its samples: the component, and the block's column and row in
// that component's block grid.  A dummy Y block (4:2:0, beyond the real block columns or rows)
// reports the block whose quantised DC it copies -- the previous one in MCU order, followed back
// to a real block -- and *dummy = true.
CG_HD void jpeg_block_source(const JpegShape &s, int mcu_x, int mcu_y, int k, int *comp, int *bx, int *by, bool *dummy)
{
    *dummy = false;
    if (s.sub == CG_JPEG_444) {
        *comp = k, *bx = mcu_x, *by = mcu_y;
        return;
    }
    if (k >= 4) {
        *comp = k - 3, *bx = mcu_x, *by = mcu_y;
        return;
    }
    int kk = k;
    while (kk > 0 && (2 * mcu_x + (kk & 1) >= s.bw || 2 * mcu_y + (kk >> 1) >= s.bh)) --kk;
    *dummy = kk != k;
    *comp = 0, *bx = 2 * mcu_x + (kk & 1), *by = 2 * mcu_y + (kk >> 1);
}

CG_HD int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's butterfly over d[0 .. 7] in place: the row pass (kRow) scales up by 4, the column
// pass descales by 4; n = 11 / 15
template <bool kRow>
CG_HD void jpeg_fdct8(int &d0, int &d1, int &d2, int &d3, int &d4, int &d5, int &d6, int &d7)
{
    constexpr int n = kRow ? 11 : 15;
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
    const int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    // the row pass's << 2 as a product: the sums may be negative, and |t10 +- t11| <= 8 * 255
    d0 = kRow ? (t10 + t11) * 4 : jpeg_descale(t10 + t11, 2);
    d4 = kRow ? (t10 - t11) * 4 : jpeg_descale(t10 - t11, 2);
    const int z1e = (t12 + t13) * 4433;
    d2 = jpeg_descale(z1e + t13 * 6270, n);
    d6 = jpeg_descale(z1e - t12 * 15137, n);
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
    z3 += z5, z4 += z5;
    d7 = jpeg_descale(m4 + z1 + z3, n);
    d5 = jpeg_descale(m5 + z2 + z4, n);
    d3 = jpeg_descale(m6 + z2 + z3, n);
    d1 = jpeg_descale(m7 + z1 + z4, n);
}

// sign(c) * ((|c| + (q8 >> 1)) / q8) with q8 = 8 q
CG_HD int jpeg_quantise(int c, int q8)
{
    const unsigned a = (unsigned)(c < 0 ? -c : c);
    const int v = (int)((a + ((unsigned)q8 >> 1)) / (unsigned)q8);
    return c < 0 ? -v : v;
}

// bits of |v|: the category of a DC difference or an AC coefficient
CG_HD int jpeg_nbits(int v)
{
    const unsigned a = (unsigned)(v < 0 ? -v : v);
#if defined(__HIP_DEVICE_COMPILE__)
    return 32 - __clz((int)a);
#else
    return a ? 32 - __builtin_clz(a) : 0;
#endif
}

// The code of one block, coefficient by coefficient: zz(k) gives the k-th zig-zag coefficient,
// emit(bits, len) takes each code with its value bits appended, len <= 26.  `t` is the table
// pair (0 Y, 1 chroma), `pred` the previous block's DC of the component.
template <class Coef, class Emit>
CG_HD void jpeg_code_block(const JpegHuff &hf, int t, int pred, Coef zz, Emit emit)
{
    const int diff = zz(0) - pred;
    const int cat = jpeg_nbits(diff);
    {
        const uint32_t e = hf.dc[t][cat];
        const uint32_t v = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u);
        emit(((e >> 5) << cat) | v, (int)(e & 31u) + cat);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = zz(k);
        if (c == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) emit(hf.ac[t][0xF0] >> 5, (int)(hf.ac[t][0xF0] & 31u));
        const int size = jpeg_nbits(c);
        const uint32_t e = hf.ac[t][(run << 4) | size];
        const uint32_t v = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1u);
        emit(((e >> 5) << size) | v, (int)(e & 31u) + size);
        run = 0;
    }
    if (run) emit(hf.ac[t][0] >> 5, (int)(hf.ac[t][0] & 31u));
}

// the block before block `b` (index in its restart interval) of the same component, or -1 for
// the first MCU of the interval, whose predictors are 0
CG_HD int jpeg_pred_block(const JpegShape &s, int b)
{
    const int k = b % s.bpm;
    if (s.sub == CG_JPEG_420 && k > 0 && k < 4) return b - 1;
    const int back = s.sub == CG_JPEG_420 ? (k == 0 ? 3 : 6) : 3;
    return b < s.bpm ? -1 : b - back;
}

}  // namespace cg
