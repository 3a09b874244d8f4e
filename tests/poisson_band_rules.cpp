// Stand-alone host program for the rules of the band levels of the Poisson stage (csrc/poisson_band_rules.h, rules 26, 27, 30 and 31),
// the body the band kernels are to run.  tests/test_poisson_band_host.py builds and runs it.  Without arguments it checks
// bd_segment on block sets of its own: the places it gives are the order (iz, iy, ix) of the rows of the stored blocks.  With two
// arguments it reads `in` — double {o[3], side}, int32 {level, band, n, 0}, n points of 3 doubles, then (G / 2 + 1)^3 doubles: a
// field on the level below — and writes `out`, for the level of G = 2^level cells: the active blocks, (G / 4)^3 bytes; the node
// classes, (G + 1)^3 bytes; for each edge type 0..6 the bytes `exists` and `open` of every node, (G + 1)^3 each (0 where the edge
// leaves the grid); the start values of rule 27 at every node, (G + 1)^3 doubles — what the test compares with
// tests/ref_poisson_band.py.
#include "poisson_band_rules.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int segments() {
    unsigned seed = 12345u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int T : {2, 3, 5, 9}) {
        for (int fill : {1, 2, 5}) {
            std::vector<int> tab((size_t)T * T * T, -1), bx, by, bz;
            for (int t = 0; t < T * T * T; ++t)
                if (rnd() % 6 < (unsigned)fill) { tab[t] = (int)bx.size(); bx.push_back(t % T); by.push_back(t / T % T); bz.push_back(t / (T * T)); }
            const int ns = (int)bx.size();
            std::vector<int> rfirst(T * T, 0), rcnt(T * T, 0), sfirst(T, 0), scnt(T, 0);
            for (int s = ns - 1; s >= 0; --s) { rfirst[bz[s] * T + by[s]] = s; sfirst[bz[s]] = s; }
            for (int s = 0; s < ns; ++s) { ++rcnt[bz[s] * T + by[s]]; ++scnt[bz[s]]; }
            std::vector<std::tuple<int, int, int, int64_t>> rows;               // (iz, iy, bx, place)
            for (int s = 0; s < ns; ++s)
                for (int lz = 0; lz < 4; ++lz)
                    for (int ly = 0; ly < 4; ++ly) {
                        const int row = bz[s] * T + by[s];
                        rows.emplace_back(4 * bz[s] + lz, 4 * by[s] + ly, bx[s], bd_segment(s, ly, lz, rfirst[row], rcnt[row], sfirst[bz[s]], scnt[bz[s]]));
                    }
            std::sort(rows.begin(), rows.end());
            for (size_t k = 0; k < rows.size(); ++k) CHECK(std::get<3>(rows[k]) == (int64_t)k);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) {
        if (segments()) return 1;
        std::printf("poisson band rules ok\n");
        return 0;
    }
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    double head[4];
    int32_t ih[4];
    if (std::fread(head, 8, 4, fi) != 4 || std::fread(ih, 4, 4, fi) != 4) return 2;
    const int l = ih[0], band = ih[1], n = ih[2], G = 1 << l, Gb = G / BD_BLOCK, T = Gb + 1, n1 = G + 1, m1 = G / 2 + 1;
    std::vector<double> pts((size_t)3 * n), below((size_t)m1 * m1 * m1);
    if (std::fread(pts.data(), 8, pts.size(), fi) != pts.size() || std::fread(below.data(), 8, below.size(), fi) != below.size()) return 2;
    std::fclose(fi);
    const double cs = head[3] / (double)G;
    const size_t tn = (size_t)T * T * T, nn = (size_t)n1 * n1 * n1;
    std::vector<uint8_t> a(tn, 0), b(tn, 0);
    for (int i = 0; i < n; ++i) {
        int blk[3];
        bd_point_block(&pts[3 * (size_t)i], head, cs, G, blk);
        a[((size_t)blk[2] * T + blk[1]) * T + blk[0]] = 1;
    }
    for (int axis = 0; axis < 3; ++axis) {                                      // a -> b -> a -> b
        const std::vector<uint8_t>& in = axis == 1 ? b : a;
        std::vector<uint8_t>& out = axis == 1 ? a : b;
        for (int bz = 0; bz < T; ++bz)
            for (int by = 0; by < T; ++by)
                for (int bx = 0; bx < T; ++bx)
                    out[((size_t)bz * T + by) * T + bx] = bx < Gb && by < Gb && bz < Gb && bd_dilate_at(in.data(), T, Gb, bx, by, bz, axis, band) ? 1 : 0;
    }
    const auto active = [&](int cx, int cy, int cz) { return b[((size_t)(cz / BD_BLOCK) * T + cy / BD_BLOCK) * T + cx / BD_BLOCK] != 0; };
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    for (int bz = 0; bz < Gb; ++bz)
        for (int by = 0; by < Gb; ++by) std::fwrite(&b[((size_t)bz * T + by) * T], 1, (size_t)Gb, fo);
    std::vector<uint8_t> cls(nn), ex(nn), op(nn);
    std::vector<double> start(nn);
    const auto coarse = [&](int jx, int jy, int jz) { return below[((size_t)jz * m1 + jy) * m1 + jx]; };
    for (int iz = 0; iz < n1; ++iz)
        for (int iy = 0; iy < n1; ++iy)
            for (int ix = 0; ix < n1; ++ix) {
                const size_t at = ((size_t)iz * n1 + iy) * n1 + ix;
                cls[at] = (uint8_t)bd_node_class(G, ix, iy, iz, active);
                start[at] = bd_start_value(ix, iy, iz, coarse);
            }
    std::fwrite(cls.data(), 1, nn, fo);
    for (int type = 0; type < 7; ++type) {
        for (int iz = 0; iz < n1; ++iz)
            for (int iy = 0; iy < n1; ++iy)
                for (int ix = 0; ix < n1; ++ix) {
                    const size_t at = ((size_t)iz * n1 + iy) * n1 + ix;
                    bool e = false, o = false;
                    if (pn_edge_in_grid(G, ix, iy, iz, type)) bd_edge_state(G, ix, iy, iz, type, active, &e, &o);
                    ex[at] = e;
                    op[at] = o;
                }
        std::fwrite(ex.data(), 1, nn, fo);
        std::fwrite(op.data(), 1, nn, fo);
    }
    std::fwrite(start.data(), 8, nn, fo);
    return std::fclose(fo) == 0 ? 0 : 2;
}
