// jpeg_rules.cpp — csrc/jpeg_rules.h as a host program of its own (tests/test_jpeg_host.py builds it with the host compiler, once plain
// and once under the address and undefined-behaviour sanitizers): the header walk and rules J3-J7 on the streams of a pack file.
//
//   jpeg_rules <pack> <out>
//
// pack: int64 n, int64 offsets[n + 1] (ascending from 0), then the bytes of the n streams.  Every stream is copied into a heap block of
// its exact length before it is walked, so a read past the stream is a sanitizer report.
// out, per stream: int32 status (0 = MVS_OK, -10 = MVS_E_IO), int32 w, h, int64 n_coef, n_plane, then (status 0 only) w * h * 3 bytes R G B,
// n_coef int16 (component by component, [block][64]) and n_plane bytes (component by component, padded planes).
#include "jpeg_rules.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

struct HostBytes {
    const uint8_t* d;
    int64_t first, end;
    uint32_t operator()(int64_t pos) const {
        if (pos < first || pos >= end) { std::fprintf(stderr, "a read outside the segment at %lld\n", (long long)pos); std::abort(); }
        return d[pos];
    }
};

static int decode(const uint8_t* d, int64_t n, JpegHeader* H, std::vector<uint8_t>* px, std::vector<int16_t>* coef, std::vector<uint8_t>* planes) {
    if (!jpeg_parse(d, n, H)) return -10;
    int64_t nc = 0, np = 0;
    const JpegLayout L = jpeg_layout(*H, 0, 0, &nc, &np);
    coef->assign((size_t)nc, 0);
    planes->assign((size_t)np, 0);
    int error = 0;
    const int b0 = L.hs[0] * L.vs[0], bpm = L.ncomp == 1 ? 1 : b0 + 2;
    for (const JpegSeg& sg : H->segs) {
        JpegBits<HostBytes> bits{HostBytes{d, sg.first, sg.end}, sg.first, sg.end, 0u, 0};
        int32_t pred[3] = {0, 0, 0};
        int err = 0;
        for (int blk = 0; blk < sg.nmcu * bpm && !err; ++blk) {
            const int m = sg.mcu0 + blk / bpm, k = blk % bpm;
            const int c = k < b0 ? 0 : k - b0 + 1, kk = k < b0 ? k : 0;
            int16_t* out = coef->data() + L.coef[c] + 64 * jpeg_block_of(L, c, m, kk % L.hs[c], kk / L.hs[c]);
            if (out < coef->data() || out + 64 > coef->data() + nc) std::abort();
            err = jpeg_decode_block(bits, H->dc[c], H->ac[c], &pred[c], out);
            if (err) for (int i = 0; i < 64; ++i) out[i] = 0;
        }
        if (err && !error) error = err;
    }
    if (error) { H->why = jpeg_scan_error(error); return -10; }
    for (int c = 0; c < L.ncomp; ++c)
        for (int64_t b = 0; b < (int64_t)L.bw[c] * L.bh[c]; ++b) {
            uint32_t ws[8][8];
            for (int x = 0; x < 8; ++x) {
                uint32_t col[8];
                jpeg_idct_column(coef->data() + L.coef[c] + 64 * b, H->quant[c], x, col);
                for (int v = 0; v < 8; ++v) ws[v][x] = col[v];
            }
            const int by = (int)(b / L.bw[c]), bx = (int)(b % L.bw[c]);
            for (int y = 0; y < 8; ++y) jpeg_idct_row(ws[y], planes->data() + L.plane[c] + ((int64_t)(by * 8 + y) * L.bw[c] + bx) * 8);
        }
    px->assign((size_t)L.w * L.h * 3, 0);
    for (int y = 0; y < L.h; ++y)
        for (int x = 0; x < L.w; ++x) jpeg_pixel(L, planes->data(), x, y, 1, px->data() + 3 * ((size_t)y * L.w + x));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: jpeg_rules <pack> <out>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1 || n < 0 || n > (1 << 20)) return 2;
    std::vector<int64_t> off((size_t)n + 1);
    if (std::fread(off.data(), 8, off.size(), f) != off.size()) return 2;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = off[(size_t)i + 1] - off[(size_t)i];
        if (len < 0) return 2;
        uint8_t* d = (uint8_t*)std::malloc(len ? (size_t)len : 1);       // exact size: the walk reads nothing past len
        if (len && std::fread(d, 1, (size_t)len, f) != (size_t)len) return 2;
        JpegHeader H;
        std::vector<uint8_t> px, planes;
        std::vector<int16_t> coef;
        const int32_t st = decode(d, len, &H, &px, &coef, &planes);
        std::free(d);
        const int32_t head[3] = {st, H.w, H.h};
        const int64_t cnt[2] = {st ? 0 : (int64_t)coef.size(), st ? 0 : (int64_t)planes.size()};
        std::fwrite(head, 4, 3, o);
        std::fwrite(cnt, 8, 2, o);
        if (st == 0) {
            std::fwrite(px.data(), 1, px.size(), o);
            std::fwrite(coef.data(), 2, coef.size(), o);
            std::fwrite(planes.data(), 1, planes.size(), o);
        }
    }
    std::fclose(o);
    std::fclose(f);
    std::printf("jpeg rules ok %lld\n", (long long)n);
    return 0;
}
