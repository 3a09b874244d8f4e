// jpeg_rules.h — rules J1-J8 of include/mvs.h (the baseline JPEG decoder): the header walk and the segment table (J1, J2: host code), and
// the per-symbol and per-sample rules as one __host__ __device__ body: the bit reader, the Huffman symbol and one block of J3, the two
// passes of J4, the chroma sample of J5 and the colour of J6, J7, and the two walks over an image's blocks (scan order, plane order),
// which the encoder shares.  The kernels of jpeg.hip run this body; tests/jpeg_rules.cpp runs it as a host program of its own,
// tests/ref_jpeg.py restates it operation for operation.  All arithmetic of J4 is uint32_t (32-bit two's-complement wrapping); a right
// shift of a signed value is the arithmetic one.
#ifndef MVS_JPEG_RULES_H_
#define MVS_JPEG_RULES_H_
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

constexpr int JPEG_E_BITS = 1, JPEG_E_CODE = 2, JPEG_E_RUN = 3, JPEG_E_SIZE = 4;   // the error word of a segment (J3)
inline const char* jpeg_scan_error(int e) {
    return e == JPEG_E_BITS ? "scan: out of bits" : e == JPEG_E_CODE ? "scan: a code that is not in its table"
         : e == JPEG_E_RUN ? "scan: a run past coefficient 63" : "scan: size category above 15";
}

// canonical codes of one table: the look-ahead of 8 bits, and maxcode / valoff for the longer codes (T.81 F.2.2.3)
struct JpegHuff {
    int32_t maxcode[17];               // [l]: the largest code of l bits, -1 without one
    int32_t valoff[17];                // [l]: index of HUFFVAL of the first code of l bits, minus that code
    int32_t nvals;
    uint8_t look_n[256], look_v[256];  // length (0: longer than 8 bits) and symbol of the code that starts the 8 bits
    uint8_t vals[256];
    uint8_t pad[4];
};
static_assert(sizeof(JpegHuff) % 4 == 0, "copied as dwords");

struct JpegSeg {                       // J2: one restart interval (or the whole scan)
    int32_t image, mcu0, nmcu, pad;
    int64_t first, end;                // bytes [first, end) of the call's data
};

// one image as the three launch sets read it: planes and coefficient blocks padded to whole MCUs
struct JpegLayout {
    int32_t w, h, ncomp, mcux, mcuy, hmax, vmax, pad;
    int32_t hs[3], vs[3];              // sampling factors (a single component counts as 1 x 1)
    int32_t bw[3], bh[3];              // blocks per row and column of the padded plane
    int32_t cw[3], ch[3];              // real samples per row and column
    int64_t coef[3];                   // first int16 of the component's blocks [bh * bw][64] in the call's coefficient array
    int64_t plane[3];                  // first byte of the component's plane [bh * 8][bw * 8] in the call's plane array
};

__host__ __device__ inline int jpeg_zigzag(int k) {
    static constexpr uint8_t Z[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return Z[k];
}

// ---------------------------------------------------------------- J3 ----
// The bit reader of one segment.  Bytes: byte(pos) for pos in [first, end) and for nothing else.
template <class Bytes>
struct JpegBits {
    Bytes byte;
    int64_t pos, end;
    uint32_t acc;                      // the low n bits are the bits not yet taken
    int n;
    __host__ __device__ void fill() {
        while (n <= 24 && pos < end) {
            const uint32_t b = byte(pos++);
            if (b == 0xFFu) {
                if (pos < end && byte(pos) == 0) ++pos;            // FF 00 is one FF
                else { pos = end; break; }                          // anything else ends the segment's bits
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    __host__ __device__ uint32_t peek16() {
        fill();
        return (n >= 16 ? acc >> (n - 16) : acc << (16 - n)) & 0xFFFFu;
    }
    __host__ __device__ bool skip(int l) {
        if (l > n) return false;
        n -= l;
        return true;
    }
    __host__ __device__ int32_t get(int s) {                       // s in 1 .. 15; -1: out of bits
        fill();
        if (s > n) return -1;
        n -= s;
        return (int32_t)((acc >> n) & ((1u << s) - 1u));
    }
};

template <class Bytes>
__host__ __device__ inline int jpeg_symbol(JpegBits<Bytes>& b, const JpegHuff& t, int* err) {
    const uint32_t pk = b.peek16();
    int l = t.look_n[pk >> 8], v;
    if (l) v = t.look_v[pk >> 8];
    else {
        l = 9;
        while (l <= 16 && (int32_t)(pk >> (16 - l)) > t.maxcode[l]) ++l;
        if (l > 16) { *err = JPEG_E_CODE; return 0; }
        const int32_t at = (int32_t)(pk >> (16 - l)) + t.valoff[l];
        if (at < 0 || at >= t.nvals) { *err = JPEG_E_CODE; return 0; }
        v = t.vals[at];
    }
    if (!b.skip(l)) { *err = JPEG_E_BITS; return 0; }
    return v;
}

__host__ __device__ inline int32_t jpeg_extend(int32_t v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one block into out[64] (zero on entry, natural order); -> 0 or the error
template <class Bytes>
__host__ __device__ inline int jpeg_decode_block(JpegBits<Bytes>& b, const JpegHuff& dc, const JpegHuff& ac, int32_t* pred, int16_t* out) {
    int err = 0;
    int s = jpeg_symbol(b, dc, &err);
    if (err) return err;
    if (s > 15) return JPEG_E_SIZE;
    if (s) {
        const int32_t v = b.get(s);
        if (v < 0) return JPEG_E_BITS;
        *pred = (int32_t)((uint32_t)*pred + (uint32_t)jpeg_extend(v, s));
    }
    out[0] = (int16_t)(uint16_t)(uint32_t)*pred;
    int k = 1;
    while (k < 64) {
        const int rs = jpeg_symbol(b, ac, &err);
        if (err) return err;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;                                     // EOB
            k += 16;                                                // ZRL
            if (k > 64) return JPEG_E_RUN;
            continue;
        }
        k += r;
        if (k > 63) return JPEG_E_RUN;
        const int32_t v = b.get(s);
        if (v < 0) return JPEG_E_BITS;
        out[jpeg_zigzag(k)] = (int16_t)jpeg_extend(v, s);
        ++k;
    }
    return 0;
}

// ---------------------------------------------------------------- the two walks over an image's blocks ----
// Scan order (J3, E6): MCUs row-major; inside an MCU the luma blocks vs x hs row-major, then Cb, then Cr.  An image has at most
// 3 * 8192 * 8192 blocks (w, h <= 65535), so a block of its scan is an int.
__host__ __device__ inline int jpeg_blocks_per_mcu(const JpegLayout& L) {
    const int b0 = L.hs[0] * L.vs[0];
    return L.ncomp == 1 ? 1 : b0 + 2;
}
// block j of the scan -> its MCU, its component and its place (bx, by) among the component's bw x bh blocks
__host__ __device__ inline void jpeg_scan_block(const JpegLayout& L, int j, int* c, int* bx, int* by, int* mcu) {
    const int bpm = jpeg_blocks_per_mcu(L), b0 = L.hs[0] * L.vs[0];
    const int m = j / bpm, k = j % bpm;
    const int cc = k < b0 ? 0 : k - b0 + 1, kk = k < b0 ? k : 0;
    *c = cc; *mcu = m;
    *bx = m % L.mcux * L.hs[cc] + kk % L.hs[cc];
    *by = m / L.mcux * L.vs[cc] + kk / L.hs[cc];
}
// Plane order (J4, E4): component by component, a component's blocks row-major.  Block b of the padded planes -> its component and
// k = by * bw + bx (false behind the last block); k -> its place.  Two steps: k_jpeg_idct addresses its block through k and takes the
// place, a 64-bit division, behind pass 1, whose loads then do not wait for it
__host__ __device__ inline bool jpeg_plane_find(const JpegLayout& L, int64_t b, int* c, int64_t* k) {
    int cc = 0;
    for (; cc < L.ncomp; ++cc) {
        const int64_t nb = (int64_t)L.bw[cc] * L.bh[cc];
        if (b < nb) break;
        b -= nb;
    }
    *c = cc; *k = b;
    return cc < L.ncomp;
}
__host__ __device__ inline void jpeg_plane_place(const JpegLayout& L, int c, int64_t k, int* bx, int* by) {
    *by = (int)(k / L.bw[c]); *bx = (int)(k % L.bw[c]);
}
__host__ __device__ inline bool jpeg_plane_block(const JpegLayout& L, int64_t b, int* c, int* bx, int* by, int64_t* k) {
    if (!jpeg_plane_find(L, b, c, k)) return false;
    jpeg_plane_place(L, *c, *k, bx, by);
    return true;
}
// first int16 of block (bx, by) of component c in the coefficient array
__host__ __device__ inline int64_t jpeg_block_at(const JpegLayout& L, int c, int bx, int by) {
    return L.coef[c] + 64 * ((int64_t)by * L.bw[c] + bx);
}

// ---------------------------------------------------------------- J4 ----
__host__ __device__ inline uint32_t jpeg_descale(uint32_t x, int n) { return (uint32_t)((int32_t)(x + (1u << (n - 1))) >> n); }

// jidctint's butterfly on eight values; the results descaled by `shift`
__host__ __device__ inline void jpeg_idct8(const uint32_t in[8], int shift, uint32_t out[8]) {
    uint32_t z2 = in[2], z3 = in[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 - z3 * 15137u;
    uint32_t tmp3 = z1 + z2 * 6270u;
    z2 = in[0]; z3 = in[4];
    uint32_t tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 = z3 * (0u - 16069u) + z5; z4 = z4 * (0u - 3196u) + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = jpeg_descale(tmp10 + tmp3, shift); out[7] = jpeg_descale(tmp10 - tmp3, shift);
    out[1] = jpeg_descale(tmp11 + tmp2, shift); out[6] = jpeg_descale(tmp11 - tmp2, shift);
    out[2] = jpeg_descale(tmp12 + tmp1, shift); out[5] = jpeg_descale(tmp12 - tmp1, shift);
    out[3] = jpeg_descale(tmp13 + tmp0, shift); out[4] = jpeg_descale(tmp13 - tmp0, shift);
}
// pass 1: column x of a block (coefficients and quantisers in natural order) -> ws[v * 8 + x], v = 0 .. 7
__host__ __device__ inline void jpeg_idct_column(const int16_t* coef, const uint16_t* quant, int x, uint32_t ws[8]) {
    uint32_t in[8];
    for (int v = 0; v < 8; ++v) in[v] = (uint32_t)(int32_t)coef[v * 8 + x] * (uint32_t)quant[v * 8 + x];
    jpeg_idct8(in, 11, ws);
}
// pass 2: one row of the workspace -> eight samples
__host__ __device__ inline void jpeg_idct_row(const uint32_t ws[8], uint8_t out[8]) {
    uint32_t r[8];
    jpeg_idct8(ws, 18, r);
    for (int x = 0; x < 8; ++x) {
        const int32_t v = (int32_t)(r[x] + 128u);
        out[x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
}

// ---------------------------------------------------------------- J5 - J7 ----
// the sample of component c at pixel (x, y): fancy upsampling on the real cw x ch samples
__host__ __device__ inline int32_t jpeg_sample(const JpegLayout& L, const uint8_t* planes, int c, int x, int y) {
    const uint8_t* p = planes + L.plane[c];
    const int pw = L.bw[c] * 8, cw = L.cw[c], ch = L.ch[c];
    const int hr = L.hmax / L.hs[c], vr = L.vmax / L.vs[c];
    if (hr == 1 && vr == 1) return p[(int64_t)y * pw + x];
    if (cw <= 2) return p[(int64_t)(y / vr) * pw + x / hr];           // a plane this narrow is replicated
    const int i = x >> 1;
    if (vr == 1) {
        const uint8_t* row = p + (int64_t)y * pw;
        const int32_t a = row[i];
        if (x & 1) return i == cw - 1 ? a : (3 * a + row[i + 1] + 2) >> 2;
        return i == 0 ? a : (3 * a + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    int far = (y & 1) ? r + 1 : r - 1;
    far = far < 0 ? 0 : far > ch - 1 ? ch - 1 : far;
    const uint8_t* near_row = p + (int64_t)r * pw;
    const uint8_t* far_row = p + (int64_t)far * pw;
    const int32_t s = 3 * near_row[i] + far_row[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near_row[i + 1] + far_row[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near_row[i - 1] + far_row[i - 1] + 8) >> 4;
}

__host__ __device__ inline uint8_t jpeg_clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// pixel (x, y) -> its three bytes; rgb != 0: R G B, else B G R
__host__ __device__ inline void jpeg_pixel(const JpegLayout& L, const uint8_t* planes, int x, int y, int rgb, uint8_t out[3]) {
    const int32_t yy = jpeg_sample(L, planes, 0, x, y);
    if (L.ncomp == 1) { out[0] = out[1] = out[2] = (uint8_t)yy; return; }
    const int32_t cb = jpeg_sample(L, planes, 1, x, y) - 128, cr = jpeg_sample(L, planes, 2, x, y) - 128;
    const uint8_t r = jpeg_clamp8(yy + ((91881 * cr + 32768) >> 16));
    const uint8_t g = jpeg_clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const uint8_t b = jpeg_clamp8(yy + ((116130 * cb + 32768) >> 16));
    out[0] = rgb ? r : b; out[1] = g; out[2] = rgb ? b : r;
}

// ---------------------------------------------------------------- J1, J2 (host) ----
struct JpegHeader {
    int32_t w = 0, h = 0, ncomp = 0, sof = 0, restart = 0;
    int32_t hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};
    uint16_t quant[3][64];             // per component, natural order
    JpegHuff dc[3], ac[3];             // per component
    int32_t dc_id[3] = {0, 0, 0}, ac_id[3] = {0, 0, 0};   // the table ids of the stream (equal ids: equal tables)
    std::vector<JpegSeg> segs;         // image = 0; first / end relative to the stream
    std::string why;                   // the feature or defect that made the walk fail
};

// BITS / HUFFVAL -> the tables of J3; false: the code lengths overflow
inline bool jpeg_build_huff(const uint8_t bits[16], const uint8_t* vals, int nvals, JpegHuff* t) {
    memset(t, 0, sizeof *t);
    t->nvals = nvals;
    memcpy(t->vals, vals, (size_t)nvals);
    int32_t code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        t->maxcode[l] = -1;
        if (bits[l - 1]) {
            t->valoff[l] = p - code;
            for (int k = 0; k < bits[l - 1]; ++k, ++code, ++p) {
                if (code >= (1 << l)) return false;
                if (l <= 8)
                    for (int f = 0; f < (1 << (8 - l)); ++f) {
                        t->look_n[(code << (8 - l)) + f] = (uint8_t)l;
                        t->look_v[(code << (8 - l)) + f] = vals[p];
                    }
            }
            t->maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    return true;
}

// the layout of an image whose coefficient blocks start at coef0 and whose planes start at plane0; -> through n_coef / n_plane what it takes
inline JpegLayout jpeg_layout(const JpegHeader& H, int64_t coef0, int64_t plane0, int64_t* n_coef, int64_t* n_plane) {
    JpegLayout L;
    memset(&L, 0, sizeof L);
    L.w = H.w; L.h = H.h; L.ncomp = H.ncomp; L.hmax = H.hs[0]; L.vmax = H.vs[0];
    L.mcux = (H.w + 8 * L.hmax - 1) / (8 * L.hmax);
    L.mcuy = (H.h + 8 * L.vmax - 1) / (8 * L.vmax);
    int64_t nc = 0, np = 0;
    for (int c = 0; c < 3; ++c) {
        const int cc = c < H.ncomp ? c : 0;
        L.hs[c] = H.hs[cc]; L.vs[c] = H.vs[cc];
        L.bw[c] = L.mcux * L.hs[c]; L.bh[c] = L.mcuy * L.vs[c];
        L.cw[c] = (H.w * L.hs[c] + L.hmax - 1) / L.hmax; L.ch[c] = (H.h * L.vs[c] + L.vmax - 1) / L.vmax;
        if (c < H.ncomp) {
            L.coef[c] = coef0 + nc; L.plane[c] = plane0 + np;
            nc += (int64_t)L.bw[c] * L.bh[c] * 64; np += (int64_t)L.bw[c] * L.bh[c] * 64;
        } else {
            L.coef[c] = L.coef[0]; L.plane[c] = L.plane[0];
        }
    }
    *n_coef = nc; *n_plane = np;
    return L;
}

// the layout of a W x H image of ncomp components with luma sampling hmax x vmax (what the encoder makes), blocks and planes from 0
inline JpegLayout jpeg_enc_layout(int w, int h, int ncomp, int hmax, int vmax, int64_t* n_coef) {
    JpegHeader H;
    H.w = w; H.h = h; H.ncomp = ncomp;
    if (ncomp == 3) { H.hs[0] = hmax; H.vs[0] = vmax; }
    int64_t np = 0;
    return jpeg_layout(H, 0, 0, n_coef, &np);
}

// J1, J2: reads nothing past len; false with H->why set
inline bool jpeg_parse(const uint8_t* d, int64_t n, JpegHeader* H) {
    auto fail = [&](const std::string& s) { H->why = s; return false; };
    auto u16 = [&](int64_t p) { return (int)((d[p] << 8) | d[p + 1]); };
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail("not a JPEG stream (no SOI)");
    uint16_t quant[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    std::vector<JpegHuff> huff(8);
    int ids[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, fh[3] = {1, 1, 1}, fv[3] = {1, 1, 1}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    int adobe = -1;
    bool frame = false;
    int64_t p = 2;
    for (;;) {
        if (p + 4 > n) return fail("header: truncated");
        if (d[p] != 0xFF) return fail("header: marker expected");
        const int m = d[p + 1];
        if (m == 0xFF) { ++p; continue; }
        p += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) return fail("header: EOI before a scan");
        const int ln = u16(p);
        if (ln < 2 || p + ln > n) return fail("header: truncated");
        int64_t s = p + 2;
        const int64_t e = p + ln;
        if (m == 0xC0 || m == 0xC1) {
            if (frame) return fail("more than one frame");
            if (e - s < 6) return fail("header: truncated");
            const int prec = d[s], nc = d[s + 5];
            H->h = u16(s + 1); H->w = u16(s + 3);
            if (prec != 8) return fail("12-bit samples");
            if (nc != 1 && nc != 3) return fail(std::to_string(nc) + " components");
            if (e - s != 6 + 3 * nc) return fail("header: bad SOF length");
            if (H->w == 0 || H->h == 0) return fail("header: empty frame");
            for (int i = 0; i < nc; ++i) {
                ids[i] = d[s + 6 + 3 * i]; fh[i] = d[s + 7 + 3 * i] >> 4; fv[i] = d[s + 7 + 3 * i] & 15; tq[i] = d[s + 8 + 3 * i];
            }
            H->ncomp = nc; H->sof = m - 0xC0;
            frame = true;
        } else if (m == 0xC2) {
            return fail("progressive");
        } else if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCC || m == 0xCD || m == 0xCE || m == 0xCF) {
            return fail("arithmetic coding");
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            return fail("lossless or hierarchical");
        } else if (m == 0xDB) {
            while (s < e) {
                const int pq = d[s] >> 4, t = d[s] & 15;
                if (pq > 1 || t > 3 || s + 1 + 64 * (pq + 1) > e) return fail("header: bad DQT");
                for (int k = 0; k < 64; ++k) quant[t][jpeg_zigzag(k)] = (uint16_t)(pq ? u16(s + 1 + 2 * k) : d[s + 1 + k]);
                have_q[t] = true;
                s += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xC4) {
            while (s < e) {
                const int tc = d[s] >> 4, th = d[s] & 15;
                if (tc > 1 || th > 3 || s + 17 > e) return fail("header: bad DHT");
                int cnt = 0;
                for (int k = 0; k < 16; ++k) cnt += d[s + 1 + k];
                if (cnt > 256 || s + 17 + cnt > e) return fail("header: bad DHT");
                if (!jpeg_build_huff(d + s + 1, d + s + 17, cnt, &huff[(size_t)(tc * 4 + th)])) return fail("Huffman table: code lengths overflow");
                have_h[tc][th] = true;
                s += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (ln != 4) return fail("header: bad DRI");
            H->restart = u16(s);
        } else if (m == 0xEE) {
            if (ln >= 14 && memcmp(d + s, "Adobe", 5) == 0) adobe = d[s + 11];
        } else if (m == 0xDA) {
            if (!frame) return fail("header: SOS before SOF");
            const int ns = e > s ? d[s] : 0;
            if (ns != H->ncomp) return fail("non-interleaved or multi-scan");
            if (e - s != 4 + 2 * ns) return fail("header: bad SOS length");
            for (int i = 0; i < ns; ++i) {
                if (d[s + 1 + 2 * i] != ids[i]) return fail("non-interleaved or multi-scan");
                td[i] = d[s + 2 + 2 * i] >> 4; ta[i] = d[s + 2 + 2 * i] & 15;
            }
            p = e;
            break;
        }
        p = e;
    }
    const int nc = H->ncomp;
    if (nc == 3 && adobe == 0) return fail("Adobe transform 0");
    if (nc == 3) {
        const bool luma = (fh[0] == 1 && fv[0] == 1) || (fh[0] == 2 && fv[0] == 1) || (fh[0] == 2 && fv[0] == 2);
        if (!luma || fh[1] != 1 || fv[1] != 1 || fh[2] != 1 || fv[2] != 1) return fail("sampling factors");
        for (int i = 0; i < 3; ++i) { H->hs[i] = fh[i]; H->vs[i] = fv[i]; }
    }
    for (int i = 0; i < nc; ++i) {
        if (tq[i] > 3 || !have_q[tq[i]]) return fail("header: missing quantisation table");
        if (td[i] > 3 || ta[i] > 3 || !have_h[0][td[i]] || !have_h[1][ta[i]]) return fail("header: missing Huffman table");
        memcpy(H->quant[i], quant[tq[i]], sizeof quant[0]);
        H->dc[i] = huff[(size_t)td[i]]; H->ac[i] = huff[(size_t)(4 + ta[i])];
        H->dc_id[i] = td[i]; H->ac_id[i] = ta[i];
    }
    const int mcux = (H->w + 8 * H->hs[0] - 1) / (8 * H->hs[0]), mcuy = (H->h + 8 * H->vs[0] - 1) / (8 * H->vs[0]);
    const int64_t total = (int64_t)mcux * mcuy, per = H->restart ? H->restart : total, want = (total + per - 1) / per;
    int64_t first = p;
    int marker;
    for (;;) {
        int64_t q = first;
        marker = 0;                                                 // 0: the data ended inside the scan
        for (; q < n; ++q)
            if (d[q] == 0xFF && q + 1 < n && d[q + 1] != 0 && d[q + 1] != 0xFF) { marker = d[q + 1]; break; }
        const int64_t k = (int64_t)H->segs.size();
        if (k == want) return fail("scan: more restart intervals than the frame has");
        const int64_t left = total - k * per;
        H->segs.push_back(JpegSeg{0, (int32_t)(k * per), (int32_t)(left < per ? left : per), 0, first, q});
        if (!(marker >= 0xD0 && marker <= 0xD7)) break;
        first = q + 2;
    }
    if ((int64_t)H->segs.size() != want)
        return fail("scan: " + std::to_string(H->segs.size()) + " of " + std::to_string(want) + " restart intervals");
    if (marker != 0 && marker != 0xD9) return fail("non-interleaved or multi-scan");
    return true;
}

#endif
