// jpeg_enc_rules.cpp — csrc/jpeg_enc_rules.h as a host program of its own (tests/test_jpeg_enc_host.py builds it with the host compiler,
// once plain and once under the address and undefined-behaviour sanitizers): rules E1-E9 on the images of a pack file.
//
//   jpeg_enc_rules <pack> <out>
//
// pack: int64 n, then per image int32 w, h, chan (1 or 3), rgb, quality, sampling, restart_interval and w * h * chan bytes.  A record with
// chan -1 or -3 is a coefficient record: in place of pixels it holds the n_coef int16 of the image as jpeg_enc_layout places them (1 or 3
// components; rgb is not read), and E6-E9 run on those.  Every image or coefficient array is copied into a heap block of its exact size
// before it is read, so a read past it is a sanitizer report.
// out, per image: int64 stream bytes, the stream, int64 n_coef, n_coef int16 (component by component, [block][64], dummy blocks zero; of a
// coefficient record: as they were read).
#include "jpeg_enc_rules.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

struct ByteSink {                      // E7: bits MSB first, FF followed by 00
    std::vector<uint8_t>* out;
    uint32_t acc = 0;
    int n = 0;
    void byte(uint32_t b) {
        out->push_back((uint8_t)b);
        if (b == 255u) out->push_back(0);
    }
    void put(uint32_t v, int k) {
        if (k < 1 || k > 16 || (v >> k)) { std::fprintf(stderr, "put(%u, %d)\n", v, k); std::abort(); }
        acc = (acc << k) | v;
        n += k;
        while (n >= 8) { n -= 8; byte((acc >> n) & 255u); }
        acc &= (1u << n) - 1u;
    }
    void flush() { if (n) put((1u << (8 - n)) - 1u, 8 - n); }
};

// E6-E9 on the n_coef coefficients at coef
static void entropy(const JpegEncShape& S, const JpegEncTables& T, const JpegLayout& L, const int16_t* coef, std::vector<uint8_t>* out) {
    *out = jpeg_enc_header(S.w, S.h, S.ncomp, S.hmax, S.vmax, T, S.restart);
    const int64_t bpm = jpeg_blocks_per_mcu(L);
    for (int t = 0; t < S.nint; ++t) {
        ByteSink sink{out};
        const int64_t first = (int64_t)t * S.per * bpm, end = first + (int64_t)S.per * bpm < S.nblk ? first + (int64_t)S.per * bpm : S.nblk;
        for (int j = (int)first; j < end; ++j) {
            int c, bx, by, m;
            jpeg_scan_block(L, j, &c, &bx, &by, &m);
            if (c < 0 || c >= L.ncomp || bx < 0 || bx >= L.bw[c] || by < 0 || by >= L.bh[c]) std::abort();
            const bool dummy = jpeg_enc_dummy(L, c, bx, by);
            const int16_t* blk = dummy ? nullptr : coef + jpeg_block_at(L, c, bx, by);
            JpegEncCount cnt;
            const int32_t pred = dummy ? 0 : jpeg_enc_pred(L, coef, j, c, S.per);
            jpeg_enc_block_bits(blk, pred, T.dc[c ? 1 : 0], T.ac[c ? 1 : 0], cnt);
            if (cnt.bits > (uint32_t)JPEG_ENC_BLOCK_BITS) std::abort();
            jpeg_enc_block_bits(blk, pred, T.dc[c ? 1 : 0], T.ac[c ? 1 : 0], sink);
        }
        sink.flush();
        if (t + 1 < S.nint) { out->push_back(0xFF); out->push_back((uint8_t)(0xD0 + (t & 7))); }
    }
    out->push_back(0xFF);
    out->push_back(0xD9);
    if ((int64_t)out->size() > jpeg_enc_bound(S)) std::abort();
}

// px: the pixels, or with chan < 0 the coefficients, in a block of their exact size
static int encode(const void* px, int w, int h, int chan, int rgb, int quality, int sampling, int restart, std::vector<uint8_t>* out,
                  std::vector<int16_t>* coef) {
    JpegEncShape S;
    if (jpeg_enc_shape(w, h, chan == 1 || chan == -1, quality, sampling, restart, &S)) return -1;
    JpegEncTables T;
    jpeg_enc_make_tables(quality, &T);
    int64_t nc = 0;
    const JpegLayout L = jpeg_enc_layout(w, h, S.ncomp, S.hmax, S.vmax, &nc);
    if (chan < 0) {
        entropy(S, T, L, (const int16_t*)px, out);
        coef->assign((const int16_t*)px, (const int16_t*)px + nc);
        return 0;
    }
    const JpegEncPixels P{(const uint8_t*)px, w, h, chan, rgb};
    coef->assign((size_t)nc, 0);
    for (int c = 0; c < L.ncomp; ++c)
        for (int by = 0; by < L.bh[c]; ++by)
            for (int bx = 0; bx < L.bw[c]; ++bx)
                if (!jpeg_enc_dummy(L, c, bx, by)) jpeg_enc_block(L, P, c, bx, by, T.quant[c ? 1 : 0], coef->data() + L.coef[c] + 64 * ((int64_t)by * L.bw[c] + bx));
    entropy(S, T, L, coef->data(), out);
    return 0;
}

// int16 of a coefficient record's image (chan -1 or -3)
static size_t coef_count(int w, int h, int chan, int quality, int sampling, int restart) {
    JpegEncShape S;
    if (jpeg_enc_shape(w, h, chan == -1, quality, sampling, restart, &S)) return 0;
    int64_t nc = 0;
    jpeg_enc_layout(w, h, S.ncomp, S.hmax, S.vmax, &nc);
    return (size_t)nc;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: jpeg_enc_rules <pack> <out>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1 || n < 0 || n > (1 << 20)) return 2;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int64_t i = 0; i < n; ++i) {
        int32_t hd[7];
        if (std::fread(hd, 4, 7, f) != 7) return 2;
        if (hd[2] != 1 && hd[2] != 3 && hd[2] != -1 && hd[2] != -3) return 2;
        const size_t len = hd[2] < 0 ? 2 * coef_count(hd[0], hd[1], hd[2], hd[4], hd[5], hd[6]) : (size_t)hd[0] * (size_t)hd[1] * (size_t)hd[2];
        uint8_t* px = (uint8_t*)std::malloc(len ? len : 1);                 // exact size: the rules read nothing outside the image
        if (std::fread(px, 1, len, f) != len) return 2;
        std::vector<uint8_t> out;
        std::vector<int16_t> coef;
        if (encode(px, hd[0], hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], &out, &coef)) return 3;
        std::free(px);
        const int64_t a = (int64_t)out.size(), b = (int64_t)coef.size();
        std::fwrite(&a, 8, 1, o);
        std::fwrite(out.data(), 1, out.size(), o);
        std::fwrite(&b, 8, 1, o);
        std::fwrite(coef.data(), 2, coef.size(), o);
    }
    std::fclose(o);
    std::fclose(f);
    std::printf("jpeg enc rules ok %lld\n", (long long)n);
    return 0;
}
