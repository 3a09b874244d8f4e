// overlay_rules.cpp — csrc/overlay_rules.h as a host program of its own (tests/test_overlay_host.py builds it with the host compiler, once
// plain and once under the address and undefined-behaviour sanitizers): rules O1-O6 on the cases of a pack file, by the kernel's
// formulation — per 16 x 16 tile the list from the highest index down, the tile test, the survivors' records, per pixel the first hit.
//
//   overlay_rules <pack> <out>
//
// pack: int64 n, then per case int32 w, h, np, np primitives of 24 bytes and w * h * 3 bytes of canvas; then int64 nf and nf floats; then
// uint64 state, int64 nc; then int32 h, swap, int64 nm, nm x 4 int32 matches, uint64 state.  Every array is copied into a heap block of
// its exact size before it is read, so a read past it is a sanitizer report.
// out: per case the painted canvas, int64 survivors (summed over the tiles) and int64 tiles; nf int32 (ovl_round_i32); nc x 3 bytes
// (ovl_rng_colour) and the uint64 state behind them; 3 nm primitives (ovl_match_prims with the colours of the generator) and the state.
// The program aborts when the tile test drops a primitive that covers a pixel of the tile, and returns 3 for a primitive O2 / O5 refuse.
#include "overlay_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class T> static T* exact(FILE* f, size_t n) {
    T* p = (T*)std::malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (std::fread(p, sizeof(T), n, f) != n) std::exit(2);
    return p;
}

static void draw(int32_t w, int32_t h, int32_t np, const OvlPrim* prims, const uint8_t* in, uint8_t* out, int64_t* survivors, int64_t* tiles) {
    std::vector<OvlRec> rec;
    std::vector<int32_t> dropped;
    for (int32_t ty0 = 0; ty0 < h; ty0 += OVL_TILE)
        for (int32_t tx0 = 0; tx0 < w; tx0 += OVL_TILE, ++*tiles) {
            rec.clear();
            dropped.clear();
            for (int32_t k = np - 1; k >= 0; --k) {
                if (ovl_tile_may(prims[k], tx0, ty0)) rec.push_back(ovl_record(prims[k]));
                else dropped.push_back(k);
            }
            *survivors += (int64_t)rec.size();
            for (int32_t y = ty0; y < ty0 + OVL_TILE && y < h; ++y)
                for (int32_t x = tx0; x < tx0 + OVL_TILE && x < w; ++x) {
                    for (int32_t k : dropped)
                        if (ovl_hit(ovl_record(prims[k]), x, y)) { std::fprintf(stderr, "tile test dropped primitive %d at (%d, %d)\n", k, x, y); std::abort(); }
                    const uint8_t* c = in + ((int64_t)y * w + x) * 3;
                    for (const OvlRec& r : rec)
                        if (ovl_hit(r, x, y)) { c = r.c; break; }
                    std::memcpy(out + ((int64_t)y * w + x) * 3, c, 3);
                }
        }
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: overlay_rules <pack> <out>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    FILE* o = f ? std::fopen(argv[2], "wb") : nullptr;
    if (!f || !o) return 2;
    int64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1 || n < 0 || n > (1 << 20)) return 2;
    for (int64_t i = 0; i < n; ++i) {
        int32_t hd[3];
        if (std::fread(hd, 4, 3, f) != 3 || hd[0] < 1 || hd[1] < 1 || hd[0] > OVL_MAX_DIM || hd[1] > OVL_MAX_DIM || hd[2] < 0) return 2;
        const size_t px = (size_t)hd[0] * (size_t)hd[1] * 3;
        OvlPrim* prims = exact<OvlPrim>(f, (size_t)hd[2]);
        uint8_t* in = exact<uint8_t>(f, px);
        for (int32_t k = 0; k < hd[2]; ++k)
            if (const char* why = ovl_prim_error(prims[k], hd[0], hd[1])) { std::fprintf(stderr, "case %lld, primitive %d: %s\n", (long long)i, k, why); return 3; }
        uint8_t* out = (uint8_t*)std::malloc(px);
        int64_t stat[2] = {0, 0};
        draw(hd[0], hd[1], hd[2], prims, in, out, &stat[0], &stat[1]);
        std::fwrite(out, 1, px, o);
        std::fwrite(stat, 8, 2, o);
        std::free(out); std::free(in); std::free(prims);
    }
    int64_t nf = 0;
    if (std::fread(&nf, 8, 1, f) != 1 || nf < 0) return 2;
    float* fl = exact<float>(f, (size_t)nf);
    for (int64_t i = 0; i < nf; ++i) {
        const int32_t r = ovl_round_i32(fl[i]);
        std::fwrite(&r, 4, 1, o);
    }
    std::free(fl);
    uint64_t state = 0;
    int64_t nc = 0;
    if (std::fread(&state, 8, 1, f) != 1 || std::fread(&nc, 8, 1, f) != 1 || nc < 0) return 2;
    for (int64_t i = 0; i < nc; ++i) {
        uint8_t bgr[3];
        ovl_rng_colour(&state, bgr);
        std::fwrite(bgr, 1, 3, o);
    }
    std::fwrite(&state, 8, 1, o);
    int32_t mh[2];
    int64_t nm = 0;
    if (std::fread(mh, 4, 2, f) != 2 || std::fread(&nm, 8, 1, f) != 1 || nm < 0) return 2;
    int32_t* m = exact<int32_t>(f, (size_t)nm * 4);
    if (std::fread(&state, 8, 1, f) != 1) return 2;
    for (int64_t i = 0; i < nm; ++i) {
        uint8_t line[3];
        OvlPrim q[3];
        ovl_rng_colour(&state, line);
        ovl_match_prims(m + 4 * i, mh[0], line, mh[1] != 0, q);
        std::fwrite(q, sizeof(OvlPrim), 3, o);
    }
    std::fwrite(&state, 8, 1, o);
    std::free(m);
    std::fclose(o);
    std::fclose(f);
    std::printf("overlay rules ok %lld\n", (long long)n);
    return 0;
}
