// cg_png_enc.h -- the arithmetic of the lossless PNG encoder (cg_png_enc.hip's kernels and the
// host-only cg_image_encode_png_host share it): the five row filters, the token rule, the
// length symbols, the code-length rule with its limiter, the canonical codes, the run-length
// coding of the code lengths and the header of a dynamic block.  Everything is integer
// arithmetic in the order written (include/cg_render.h states the contract).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/cg_render.h"
#include "cg_math.h"

namespace cg {

constexpr int kPngBandRows = 16;        // rows of a band: one deflate block run, one IDAT chunk
constexpr int kPngLitLen = 286;         // literal / length alphabet
constexpr int kPngClSyms = 19;          // code-length alphabet
constexpr int kPngMaxStored = 65535;    // bytes of one stored block
constexpr int kPngMaxMatch = 258;
constexpr int kPngClMax = kPngLitLen + 2;   // entries of a block's code-length sequence at most
// the order in which a dynamic block's header carries the code-length code's lengths
constexpr uint8_t kPngClOrder[kPngClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

CG_HD int png_bpp(int colour) { return colour == CG_PNG_RGBA ? 4 : 3; }

// byte x of a row of pixels as the file carries it (R G B [A]); 0 left of the row and above the image
CG_HD int png_raw(const uint32_t *row, int x, int bpp)
{
    if (!row || x < 0) return 0;
    const int px = bpp == 4 ? x >> 2 : x / 3;
    const int c = x - px * bpp;
    return (int)((row[px] >> (c == 3 ? 24 : 16 - 8 * c)) & 255u);
}

CG_HD int png_paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// the five filtered values of byte x of a row (`up`: the row above, NULL for the first)
CG_HD void png_filter_all(const uint32_t *cur, const uint32_t *up, int x, int bpp, int out[5])
{
    const int v = png_raw(cur, x, bpp), a = png_raw(cur, x - bpp, bpp), b = png_raw(up, x, bpp),
              c = png_raw(up, x - bpp, bpp);
    out[0] = v;
    out[1] = (v - a) & 255;
    out[2] = (v - b) & 255;
    out[3] = (v - ((a + b) >> 1)) & 255;
    out[4] = (v - png_paeth(a, b, c)) & 255;
}
CG_HD int png_filter_byte(int type, const uint32_t *cur, const uint32_t *up, int x, int bpp)
{
    int f[5];
    png_filter_all(cur, up, x, bpp, f);
    return f[type];
}
// a filtered byte read as int8, its absolute value
CG_HD uint32_t png_abs8(int b) { return (uint32_t)(b < 128 ? b : 256 - b); }

// The token of one byte of a band from where it stands in its run of equal bytes: j bytes of
// the run precede it, fwd bytes (itself included) remain.  fwd may be cut at any value of 258
// or more.  0: the byte is inside a match and sends nothing; 1: a literal; 2: a match of *len
// (distance 1) starts here.
CG_HD int png_token(uint32_t j, uint32_t fwd, int *len)
{
    if (j == 0 || j + fwd < 4u) return 1;
    const uint32_t r = (j - 1u) % (uint32_t)kPngMaxMatch;
    const uint32_t l = r + fwd < (uint32_t)kPngMaxMatch ? r + fwd : (uint32_t)kPngMaxMatch;
    if (l < 3u) return 1;
    if (r) return 0;
    *len = (int)l;
    return 2;
}

// length 3 .. 258 -> its symbol 257 .. 285, the count of extra bits and their value
CG_HD int png_len_symbol(int len, int *ebits, int *eval)
{
    *ebits = 0, *eval = 0;
    if (len <= 10) return 254 + len;
    if (len == kPngMaxMatch) return 285;
    const int l = len - 3;
    int e = 1;
    while ((l >> (e + 2)) > 1) ++e;
    *ebits = e;
    *eval = l & ((1 << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}
// bits a token of symbol s costs beyond its code: a length's extra bits and its 1-bit distance
CG_HD int png_sym_extra(int s) { return s <= 256 ? 0 : 1 + (s < 265 || s == 285 ? 0 : (s - 261) >> 2); }

CG_HD uint32_t png_bitrev(uint32_t c, int len)
{
    uint32_t r = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
    r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
    r = ((r & 0x0F0Fu) << 4) | ((r >> 4) & 0x0F0Fu);
    r = ((r & 0x00FFu) << 8) | (r >> 8);
    return r >> (16 - len);
}

CG_HD uint32_t png_crc_byte(uint32_t c, int b)
{
    c ^= (uint32_t)b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

// ---- the code-length rule ----
struct PngHuffWork {
    uint16_t order[kPngLitLen];       // the used symbols by (frequency, symbol)
    uint32_t wt[kPngLitLen];          // weights of the internal nodes, in the order made
    uint16_t parent[2 * kPngLitLen];  // leaves 0 .. m - 1 (sorted position), internal nodes m ..
    uint16_t depth[kPngLitLen];       // of the internal nodes
    uint16_t count[16];               // codes per length
    uint32_t clf[kPngClSyms];         // frequencies of the code-length symbols
};

// order[0 .. m) = the symbols of freq[0 .. n) that occur, by (frequency, symbol); returns m
CG_HD int png_sort_symbols(const uint32_t *freq, int n, uint16_t *order)
{
    int m = 0;
    for (int s = 0; s < n; ++s) {
        if (!freq[s]) continue;
        int k = m++;
        while (k > 0 && freq[order[k - 1]] > freq[s]) {
            order[k] = order[k - 1];
            --k;
        }
        order[k] = (uint16_t)s;
    }
    return m;
}

// lengths[0 .. n) from the sorted symbols: a two-queue Huffman merge (a leaf before an internal
// node of equal weight), depths clamped at `limit`, the Kraft sum repaired, the lengths handed
// out in sorted order.  Needs 2 <= m <= 2^limit and a sum of frequencies below 2^32; m == 1
// gives that symbol length 1, m == 0 nothing.
CG_HD void png_lengths_from_order(const uint32_t *freq, int n, int m, int limit, uint8_t *lengths, PngHuffWork &w)
{
    for (int s = 0; s < n; ++s) lengths[s] = 0;
    if (m <= 0) return;
    if (m == 1) {
        lengths[w.order[0]] = 1;
        return;
    }
    int li = 0, ii = 0;
    for (int k = 0; k < m - 1; ++k) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
            const bool leaf = li < m && (ii >= k || freq[w.order[li]] <= w.wt[ii]);
            const int idx = leaf ? li++ : m + ii++;
            sum += leaf ? freq[w.order[idx]] : w.wt[idx - m];
            w.parent[idx] = (uint16_t)(m + k);
        }
        w.wt[k] = sum;
    }
    w.depth[m - 2] = 0;
    for (int k = m - 3; k >= 0; --k) w.depth[k] = (uint16_t)(w.depth[w.parent[m + k] - m] + 1);
    for (int l = 0; l <= limit; ++l) w.count[l] = 0;
    for (int i = 0; i < m; ++i) {
        int d = w.depth[w.parent[i] - m] + 1;
        if (d > limit) d = limit;
        ++w.count[d];
    }
    uint32_t kraft = 0;   // in units of 2^-limit
    for (int l = 1; l <= limit; ++l) kraft += (uint32_t)w.count[l] << (limit - l);
    while (kraft > (1u << limit)) {
        int bits = limit - 1;
        while (bits > 0 && !w.count[bits]) --bits;
        if (!bits) break;
        --w.count[bits];
        w.count[bits + 1] = (uint16_t)(w.count[bits + 1] + 2);
        --w.count[limit];
        --kraft;
    }
    int i = 0;
    for (int l = limit; l >= 1; --l)
        for (int c = 0; c < (int)w.count[l]; ++c) lengths[w.order[i++]] = (uint8_t)l;
}

// canonical codes of lengths[0 .. n), each stored with its first bit lowest (deflate sends a
// code from its top bit, everything from a byte's lowest)
CG_HD void png_assign_codes(const uint8_t *lengths, int n, int limit, uint16_t *codes, uint16_t *next /* [16] */)
{
    for (int l = 0; l <= limit; ++l) next[l] = 0;
    for (int s = 0; s < n; ++s) ++next[lengths[s]];
    uint32_t code = 0, prev = 0;
    for (int l = 1; l <= limit; ++l) {
        code = (code + prev) << 1;
        prev = next[l];
        next[l] = (uint16_t)code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = lengths[s];
        codes[s] = l ? (uint16_t)png_bitrev(next[l]++, l) : (uint16_t)0;
    }
}

// ---- one band's dynamic block ----
struct PngPlan {
    uint8_t ll_len[kPngLitLen];
    uint16_t ll_code[kPngLitLen];
    uint8_t cl_len[kPngClSyms];
    uint16_t cl_code[kPngClSyms];
    uint16_t cl_seq[kPngClMax];   // the code-length sequence: symbol | extra value << 8
    int n_cl, hlit, hclen;
    uint32_t header_bits;         // BFINAL .. the last code length
    uint32_t dyn_bits;            // the whole block, end-of-block included
};

// The plan from a band's frequencies (freq[256] = 1 included) and their sorted order.
CG_HD void png_make_plan(const uint32_t *freq, int m, PngPlan &p, PngHuffWork &w)
{
    png_lengths_from_order(freq, kPngLitLen, m, 15, p.ll_len, w);
    png_assign_codes(p.ll_len, kPngLitLen, 15, p.ll_code, w.count);
    int hlit = kPngLitLen;
    while (hlit > 257 && !p.ll_len[hlit - 1]) --hlit;
    p.hlit = hlit;
    // the hlit lengths and the two distance lengths (1, 1) as one sequence, run-length coded greedily
    const int total = hlit + 2;
    uint32_t *clf = w.clf;
    for (int s = 0; s < kPngClSyms; ++s) clf[s] = 0;
    int n = 0;
    for (int i = 0; i < total;) {
        const int v = i < hlit ? p.ll_len[i] : 1;
        int r = 1;
        while (i + r < total && (i + r < hlit ? p.ll_len[i + r] : 1) == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) {
                const int t = r < 138 ? r : 138;
                p.cl_seq[n++] = (uint16_t)(18 | ((t - 11) << 8)), ++clf[18], r -= t;
            }
            if (r >= 3) p.cl_seq[n++] = (uint16_t)(17 | ((r - 3) << 8)), ++clf[17], r = 0;
        } else {
            p.cl_seq[n++] = (uint16_t)v, ++clf[v], --r;
            while (r >= 3) {
                const int t = r < 6 ? r : 6;
                p.cl_seq[n++] = (uint16_t)(16 | ((t - 3) << 8)), ++clf[16], r -= t;
            }
        }
        for (; r > 0; --r) p.cl_seq[n++] = (uint16_t)v, ++clf[v];
    }
    p.n_cl = n;
    const int mc = png_sort_symbols(clf, kPngClSyms, w.order);
    png_lengths_from_order(clf, kPngClSyms, mc, 7, p.cl_len, w);
    png_assign_codes(p.cl_len, kPngClSyms, 7, p.cl_code, w.count);
    int hclen = kPngClSyms;
    while (hclen > 4 && !p.cl_len[kPngClOrder[hclen - 1]]) --hclen;
    p.hclen = hclen;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int s = 0; s < kPngClSyms; ++s) bits += clf[s] * (uint32_t)(p.cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
    p.header_bits = bits;
    for (int s = 0; s < kPngLitLen; ++s) bits += freq[s] * (uint32_t)(p.ll_len[s] + png_sym_extra(s));
    p.dyn_bits = bits;
}

// the block's header through put(value, bits), values lowest bit first
template <class Put>
CG_HD void png_put_header(const PngPlan &p, int bfinal, Put put)
{
    put((uint32_t)bfinal, 1);
    put(2u, 2);
    put((uint32_t)(p.hlit - 257), 5);
    put(1u, 5);
    put((uint32_t)(p.hclen - 4), 4);
    for (int k = 0; k < p.hclen; ++k) put((uint32_t)p.cl_len[kPngClOrder[k]], 3);
    for (int i = 0; i < p.n_cl; ++i) {
        const int s = p.cl_seq[i] & 255, ev = p.cl_seq[i] >> 8;
        put((uint32_t)p.cl_code[s], p.cl_len[s]);
        if (s >= 16) put((uint32_t)ev, s == 16 ? 2 : s == 17 ? 3 : 7);
    }
}
// a token's bits and their count: a literal's code; a length's code, extra bits and the 1-bit
// distance code 0
CG_HD uint32_t png_literal_bits(const PngPlan &p, int byte, int *n)
{
    *n = p.ll_len[byte];
    return p.ll_code[byte];
}
CG_HD uint32_t png_match_bits(const PngPlan &p, int len, int *n)
{
    int eb, ev;
    const int s = png_len_symbol(len, &eb, &ev);
    const int l = p.ll_len[s];
    *n = l + eb + 1;
    return (uint32_t)p.ll_code[s] | ((uint32_t)ev << l);
}

// a band of n bytes as stored blocks: their count and the bits they take from a byte boundary
CG_HD uint32_t png_stored_blocks(uint32_t n) { return (n + (uint32_t)kPngMaxStored - 1u) / (uint32_t)kPngMaxStored; }
CG_HD uint32_t png_stored_bits(uint32_t n) { return 8u * n + 40u * png_stored_blocks(n); }

// the shape of a file
struct PngShape {
    int w, h, bpp, colour, nb;   // nb: bands
    uint32_t rb;                 // bytes of a filtered row
};
CG_HD PngShape png_shape(int w, int h, int colour)
{
    PngShape s;
    s.w = w, s.h = h, s.colour = colour, s.bpp = png_bpp(colour);
    s.nb = (h + kPngBandRows - 1) / kPngBandRows;
    s.rb = 1u + (uint32_t)w * (uint32_t)s.bpp;
    return s;
}
CG_HD uint32_t png_band_bytes(const PngShape &s, int band)
{
    const int rows = s.h - band * kPngBandRows < kPngBandRows ? s.h - band * kPngBandRows : kPngBandRows;
    return (uint32_t)rows * s.rb;
}

}  // namespace cg
