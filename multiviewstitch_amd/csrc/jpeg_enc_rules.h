// jpeg_enc_rules.h — rules E1-E9 of include/mvs.h (the baseline JPEG encoder): the per-sample and per-symbol rules as one
// __host__ __device__ body — the colour of E2, the sample of E3, the two passes of E4, the quantiser of E5, the dummy blocks and the DC
// predecessor of E6, one block of E7 into a bit sink — and the host parts: the tables of E5 / E7, the header of E8, the bound of E9.
// The scan order of E6 (jpeg_scan_block), the plane order and jpeg_enc_layout are in jpeg_rules.h, stated once for both directions.  The
// kernels of jpeg_enc.hip run this body; tests/jpeg_enc_rules.cpp runs it as a host program of its own, tests/ref_jpeg_enc.py restates it
// operation for operation.  All arithmetic is int32_t; a right shift of a signed value is the arithmetic one.
#ifndef MVS_JPEG_ENC_RULES_H_
#define MVS_JPEG_ENC_RULES_H_
#include "jpeg_rules.h"

constexpr int JPEG_ENC_RESTART_ROW = 65536;                         // MVS_JPEG_RESTART_ROW
constexpr int JPEG_ENC_BLOCK_BITS = 12 + 11 + 63 * (16 + 10);       // E9: a DC code and its bits, 63 AC codes and theirs

// code and length of every symbol of one table
struct JpegEncHuff {
    uint16_t code[256];
    uint8_t size[256];                 // 0: not a symbol of the table
};
struct JpegEncTables {
    JpegEncHuff dc[2], ac[2];          // [0]: luma (T.81 K.3, K.5), [1]: chroma (K.4, K.6)
    uint16_t quant[2][64];             // E5, natural order
};

// ---------------------------------------------------------------- E2 ----
// component c (0: Y, 1: Cb, 2: Cr) of one pixel
__host__ __device__ inline int32_t jpeg_enc_ycc(int32_t r, int32_t g, int32_t b, int c) {
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// the pixels of one image as the encoder reads them: chan = 1 (grey) or 3; rgb != 0: R G B in memory, else B G R
struct JpegEncPixels {
    const uint8_t* px;
    int32_t w, h, chan, rgb;
    __host__ __device__ int32_t operator()(int c, int x, int y) const {   // x, y inside the image
        const uint8_t* p = px + ((int64_t)y * w + x) * chan;
        if (chan == 1) return p[0];
        return jpeg_enc_ycc(rgb ? p[0] : p[2], p[1], rgb ? p[2] : p[0], c);
    }
};

// ---------------------------------------------------------------- E3 ----
// sample (x, y) of component c's plane, which is whole MCUs wide and high
__host__ __device__ inline int32_t jpeg_enc_sample(const JpegLayout& L, const JpegEncPixels& P, int c, int x, int y) {
    const int hr = L.hmax / L.hs[c], vr = L.vmax / L.vs[c];
    const int rows = (L.h + L.vmax - 1) / L.vmax * L.vmax / vr;      // downsampled rows that exist before the last one is repeated
    if (y > rows - 1) y = rows - 1;
    const int W1 = L.w - 1, H1 = L.h - 1;
    if (hr == 1 && vr == 1) return P(c, x < W1 ? x : W1, y < H1 ? y : H1);
    const int x0 = 2 * x < W1 ? 2 * x : W1, x1 = 2 * x + 1 < W1 ? 2 * x + 1 : W1;
    if (vr == 1) {
        const int yy = y < H1 ? y : H1;
        return (P(c, x0, yy) + P(c, x1, yy) + (x & 1)) >> 1;
    }
    const int y0 = 2 * y < H1 ? 2 * y : H1, y1 = 2 * y + 1 < H1 ? 2 * y + 1 : H1;
    return (P(c, x0, y0) + P(c, x1, y0) + P(c, x0, y1) + P(c, x1, y1) + 1 + (x & 1)) >> 2;
}

// ---------------------------------------------------------------- E4 ----
__host__ __device__ inline int32_t jpeg_enc_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's butterfly on eight values; first: the row pass
__host__ __device__ inline void jpeg_fdct8(const int32_t d[8], bool first, int32_t out[8]) {
    int32_t tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int32_t tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int n = first ? 11 : 15;
    out[0] = first ? (tmp10 + tmp11) * 4 : jpeg_enc_descale(tmp10 + tmp11, 2);
    out[4] = first ? (tmp10 - tmp11) * 4 : jpeg_enc_descale(tmp10 - tmp11, 2);
    int32_t z1 = (tmp12 + tmp13) * 4433;
    out[2] = jpeg_enc_descale(z1 + tmp13 * 6270, n);
    out[6] = jpeg_enc_descale(z1 - tmp12 * 15137, n);
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * 9633;
    tmp4 *= 2446; tmp5 *= 16819; tmp6 *= 25172; tmp7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    out[7] = jpeg_enc_descale(tmp4 + z1 + z3, n);
    out[5] = jpeg_enc_descale(tmp5 + z2 + z4, n);
    out[3] = jpeg_enc_descale(tmp6 + z2 + z3, n);
    out[1] = jpeg_enc_descale(tmp7 + z1 + z4, n);
}

// ---------------------------------------------------------------- E5 ----
__host__ __device__ inline int16_t jpeg_enc_quantise(int32_t c, int32_t e) {
    const int32_t a = ((c < 0 ? -c : c) + 4 * e) / (8 * e);
    return (int16_t)(c < 0 ? -a : a);
}

// E3-E5 for block (bx, by) of component c: 64 quantised coefficients in natural order
__host__ __device__ inline void jpeg_enc_block(const JpegLayout& L, const JpegEncPixels& P, int c, int bx, int by, const uint16_t* quant,
                                               int16_t out[64]) {
    int32_t ws[64];
    for (int y = 0; y < 8; ++y) {
        int32_t d[8];
        for (int x = 0; x < 8; ++x) d[x] = jpeg_enc_sample(L, P, c, bx * 8 + x, by * 8 + y) - 128;
        jpeg_fdct8(d, true, ws + 8 * y);
    }
    for (int x = 0; x < 8; ++x) {
        int32_t d[8], r[8];
        for (int y = 0; y < 8; ++y) d[y] = ws[8 * y + x];
        jpeg_fdct8(d, false, r);
        for (int y = 0; y < 8; ++y) out[8 * y + x] = jpeg_enc_quantise(r[y], quant[8 * y + x]);
    }
}

// ---------------------------------------------------------------- E6 ----
__host__ __device__ inline bool jpeg_enc_dummy(const JpegLayout& L, int c, int bx, int by) {
    return bx >= (L.cw[c] + 7) / 8 || by >= (L.ch[c] + 7) / 8;
}
// the DC predictor of scan block j (component c): the DC of the last real block of c in front of it inside its restart interval of
// `per` MCUs, 0 without one.  coef: the image's blocks as JpegLayout places them
__host__ __device__ inline int32_t jpeg_enc_pred(const JpegLayout& L, const int16_t* coef, int j, int c, int per) {
    const int bpm = jpeg_blocks_per_mcu(L), first = j / bpm / per * per * bpm;   // the interval's first block
    for (int q = j - 1; q >= first; --q) {
        int cc, bx, by, m;
        jpeg_scan_block(L, q, &cc, &bx, &by, &m);
        if (cc == c && !jpeg_enc_dummy(L, c, bx, by)) return coef[jpeg_block_at(L, c, bx, by)];
    }
    return 0;
}

// ---------------------------------------------------------------- E7 ----
__host__ __device__ inline int jpeg_enc_size(int32_t v) {
    uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int s = 0;
    while (a) { ++s; a >>= 1; }
    return s;
}
// one block (blk == NULL: a dummy block) into sink.put(bits, count), count in 1 .. 16
template <class Sink>
__host__ __device__ inline void jpeg_enc_block_bits(const int16_t* blk, int32_t pred, const JpegEncHuff& dc, const JpegEncHuff& ac, Sink& sink) {
    if (!blk) {
        sink.put(dc.code[0], dc.size[0]);
        sink.put(ac.code[0], ac.size[0]);
        return;
    }
    const int32_t d = (int32_t)blk[0] - pred;
    int s = jpeg_enc_size(d);
    sink.put(dc.code[s], dc.size[s]);
    if (s) sink.put((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int32_t v = blk[jpeg_zigzag(k)];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) sink.put(ac.code[0xF0], ac.size[0xF0]);
        s = jpeg_enc_size(v);
        sink.put(ac.code[(run << 4) | s], ac.size[(run << 4) | s]);
        sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s);
        run = 0;
    }
    if (run) sink.put(ac.code[0], ac.size[0]);
}
struct JpegEncCount {                  // the sink that measures
    uint32_t bits = 0;
    __host__ __device__ void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// ---------------------------------------------------------------- tables, E8, E9 (host) ----
namespace jpeg_enc_tables {
constexpr uint8_t K1[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t K2[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                            99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t AC_VALS[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
     114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86,
     87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138,
     146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
     194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233,
     234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
     209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
     86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136,
     137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
     185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
     233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};
}  // namespace jpeg_enc_tables

inline void jpeg_enc_build_huff(const uint8_t bits[16], const uint8_t* vals, JpegEncHuff* t) {
    memset(t, 0, sizeof *t);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int k = 0; k < bits[l - 1]; ++k, ++code, ++p) { t->code[vals[p]] = (uint16_t)code; t->size[vals[p]] = (uint8_t)l; }
        code <<= 1;
    }
}
// E5: the table of `base` at `quality` (1 .. 100), natural order
inline void jpeg_enc_quant_table(const uint8_t base[64], int quality, uint16_t out[64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        const int e = (base[k] * scale + 50) / 100;
        out[k] = (uint16_t)(e < 1 ? 1 : e > 255 ? 255 : e);
    }
}
inline void jpeg_enc_make_tables(int quality, JpegEncTables* T) {
    using namespace jpeg_enc_tables;
    for (int t = 0; t < 2; ++t) {
        jpeg_enc_build_huff(DC_BITS[t], DC_VALS, &T->dc[t]);
        jpeg_enc_build_huff(AC_BITS[t], AC_VALS[t], &T->ac[t]);
    }
    jpeg_enc_quant_table(K1, quality, T->quant[0]);
    jpeg_enc_quant_table(K2, quality, T->quant[1]);
}

// E8: everything in front of the scan; restart: the interval in MCUs as DRI states it (0: no DRI)
inline std::vector<uint8_t> jpeg_enc_header(int w, int h, int ncomp, int hmax, int vmax, const JpegEncTables& T, int restart) {
    using namespace jpeg_enc_tables;
    std::vector<uint8_t> o = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
    auto u16 = [&](int v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)(v & 255)); };
    const int ntab = ncomp == 1 ? 1 : 2;
    for (int t = 0; t < ntab; ++t) {
        o.push_back(0xFF); o.push_back(0xDB); u16(67); o.push_back((uint8_t)t);
        for (int k = 0; k < 64; ++k) o.push_back((uint8_t)T.quant[t][jpeg_zigzag(k)]);
    }
    o.push_back(0xFF); o.push_back(0xC0); u16(8 + 3 * ncomp); o.push_back(8); u16(h); u16(w); o.push_back((uint8_t)ncomp);
    for (int c = 0; c < ncomp; ++c) {
        o.push_back((uint8_t)(c + 1)); o.push_back((uint8_t)(c == 0 && ncomp == 3 ? (hmax << 4) | vmax : 0x11)); o.push_back((uint8_t)(c ? 1 : 0));
    }
    for (int t = 0; t < ntab; ++t)
        for (int cls = 0; cls < 2; ++cls) {
            const uint8_t* bits = cls ? AC_BITS[t] : DC_BITS[t];
            const uint8_t* vals = cls ? AC_VALS[t] : DC_VALS;
            const int nv = cls ? 162 : 12;
            o.push_back(0xFF); o.push_back(0xC4); u16(19 + nv); o.push_back((uint8_t)((cls << 4) | t));
            o.insert(o.end(), bits, bits + 16);
            o.insert(o.end(), vals, vals + nv);
        }
    if (restart) { o.push_back(0xFF); o.push_back(0xDD); u16(4); u16(restart); }
    o.push_back(0xFF); o.push_back(0xDA); u16(6 + 2 * ncomp); o.push_back((uint8_t)ncomp);
    for (int c = 0; c < ncomp; ++c) { o.push_back((uint8_t)(c + 1)); o.push_back((uint8_t)(c ? 0x11 : 0x00)); }
    o.push_back(0x00); o.push_back(0x3F); o.push_back(0x00);
    return o;
}

// what a call's parameters come to (E1), validated by the caller
struct JpegEncShape {
    int32_t w, h, ncomp, hmax, vmax, quality;
    int32_t restart;                   // MCUs per interval as DRI states it, 0: none
    int32_t per, nint;                 // MCUs per interval (the whole scan without restarts) and intervals per image
    int64_t nmcu, nblk;                // MCUs and scan blocks per image
};
// E1: NULL, or what is wrong
inline const char* jpeg_enc_shape(int w, int h, bool grey, int quality, int sampling, int restart_interval, JpegEncShape* S) {
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return "w and h must be in 1 .. 65535";
    if (quality < 1 || quality > 100) return "quality must be in 1 .. 100";
    if (sampling != 444 && sampling != 422 && sampling != 420) return "sampling must be 444, 422 or 420";
    if (restart_interval < 0 || (restart_interval > 65535 && restart_interval != JPEG_ENC_RESTART_ROW))
        return "restart_interval must be in 0 .. 65535 or MVS_JPEG_RESTART_ROW";
    S->w = w; S->h = h; S->ncomp = grey ? 1 : 3; S->quality = quality;
    S->hmax = grey || sampling == 444 ? 1 : 2;
    S->vmax = !grey && sampling == 420 ? 2 : 1;
    const int mcux = (w + 8 * S->hmax - 1) / (8 * S->hmax), mcuy = (h + 8 * S->vmax - 1) / (8 * S->vmax);
    S->nmcu = (int64_t)mcux * mcuy;
    S->restart = restart_interval == JPEG_ENC_RESTART_ROW ? mcux : restart_interval;
    const int64_t per = S->restart ? S->restart : S->nmcu;
    if (S->nmcu > 0x7fffffffLL) return "too many MCUs";
    S->per = (int32_t)per;
    S->nint = (int32_t)((S->nmcu + per - 1) / per);
    S->nblk = S->nmcu * (grey ? 1 : S->hmax * S->vmax + 2);
    return nullptr;
}
// E9: an upper bound of one stream: the header (at most 623 bytes + DRI), then every scan block at its longest (JPEG_ENC_BLOCK_BITS),
// every interval's last byte padded, every byte of the scan an FF that takes a second byte, a marker behind every interval (EOI behind
// the last)
inline int64_t jpeg_enc_bound(const JpegEncShape& S) {
    const int64_t scan = (S.nblk * JPEG_ENC_BLOCK_BITS + 7) / 8 + S.nint;
    return 640 + 2 * scan + 2 * (int64_t)S.nint;
}

#endif
