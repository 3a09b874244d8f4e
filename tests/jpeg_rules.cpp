// jpeg_rules.cpp — csrc/jpeg_rules.h as a host program of its own (tests/test_jpeg_host.py builds it with the host compiler, once plain
// and once under the address and undefined-behaviour sanitizers): the header walk and rules J3-J7 on the streams of a pack file.
//
//   jpeg_rules <pack> <out>
//
// pack: int64 n, int64 offsets[n + 1] (ascending from 0), then the bytes of the n streams.  Every stream is copied into a heap block of
// its exact length before it is walked, so a read past the stream is a sanitizer report.
// out, per stream: int32 status (0 = MVS_OK, -10 = MVS_E_IO), int32 w, h, int64 n_coef, n_plane, then (status 0 only) w * h * 3 bytes R G B,
// n_coef int16 (component by component, [block][64]) and n_plane bytes (component by component, padded planes).
// Before that, the header walk of all streams runs on the host fan-out (csrc/host_parts.h, as jpeg_plan of jpeg.hip runs it) with 1 part
// and with 4 parts; the two sets of headers must be identical.
#include "jpeg_rules.h"
#include "host_parts.h"
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
    const int bpm = jpeg_blocks_per_mcu(L);
    for (const JpegSeg& sg : H->segs) {
        JpegBits<HostBytes> bits{HostBytes{d, sg.first, sg.end}, sg.first, sg.end, 0u, 0};
        int32_t pred[3] = {0, 0, 0};
        int err = 0;
        for (int blk = 0; blk < sg.nmcu * bpm && !err; ++blk) {
            int c, bx, by, m;
            jpeg_scan_block(L, sg.mcu0 * bpm + blk, &c, &bx, &by, &m);
            int16_t* out = coef->data() + jpeg_block_at(L, c, bx, by);
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

static bool same_header(bool oka, const JpegHeader& a, bool okb, const JpegHeader& b) {
    if (oka != okb || a.why != b.why) return false;
    if (!oka) return true;
    bool same = a.w == b.w && a.h == b.h && a.ncomp == b.ncomp && a.sof == b.sof && a.restart == b.restart && a.segs.size() == b.segs.size();
    for (int c = 0; same && c < a.ncomp; ++c)
        same = a.hs[c] == b.hs[c] && a.vs[c] == b.vs[c] && a.dc_id[c] == b.dc_id[c] && a.ac_id[c] == b.ac_id[c] &&
               !memcmp(a.quant[c], b.quant[c], sizeof a.quant[c]) && !memcmp(&a.dc[c], &b.dc[c], sizeof(JpegHuff)) &&
               !memcmp(&a.ac[c], &b.ac[c], sizeof(JpegHuff));
    for (size_t k = 0; same && k < a.segs.size(); ++k) same = !memcmp(&a.segs[k], &b.segs[k], sizeof(JpegSeg));
    return same;
}

// the header walk of every stream on `parts` threads, strided as jpeg_plan strides it
static void walk_all(int parts, const std::vector<uint8_t*>& d, const std::vector<int64_t>& off, std::vector<JpegHeader>* hd, std::vector<char>* ok) {
    const int n = (int)d.size();
    hd->assign((size_t)n, JpegHeader());
    ok->assign((size_t)n, 0);
    parallel_parts(parts, [&](int t) {
        for (int i = t; i < n; i += parts) (*ok)[(size_t)i] = jpeg_parse(d[(size_t)i], off[(size_t)i + 1] - off[(size_t)i], &(*hd)[(size_t)i]);
    });
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
    std::vector<uint8_t*> blk((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = off[(size_t)i + 1] - off[(size_t)i];
        if (len < 0) return 2;
        blk[(size_t)i] = (uint8_t*)std::malloc(len ? (size_t)len : 1);   // exact size: the walk reads nothing past len
        if (len && std::fread(blk[(size_t)i], 1, (size_t)len, f) != (size_t)len) return 2;
    }
    std::vector<JpegHeader> h1, h4;
    std::vector<char> ok1, ok4;
    walk_all(1, blk, off, &h1, &ok1);
    walk_all(4, blk, off, &h4, &ok4);
    for (int64_t i = 0; i < n; ++i)
        if (!same_header(ok1[(size_t)i], h1[(size_t)i], ok4[(size_t)i], h4[(size_t)i])) {
            std::fprintf(stderr, "stream %lld: the header walk on 4 parts differs from the walk on 1 part\n", (long long)i);
            return 4;
        }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = off[(size_t)i + 1] - off[(size_t)i];
        uint8_t* d = blk[(size_t)i];
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
    std::printf("jpeg rules ok %lld, headers equal on 1 and 4 parts\n", (long long)n);
    return 0;
}
