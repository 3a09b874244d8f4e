// Stand-alone host program for the per-point and per-tetrahedron rules of mvs_poisson_reconstruct (csrc/poisson_rules.h), the body the
// kernels of poisson.hip run.  tests/test_poisson_host.py builds it with -fsanitize=address,undefined and runs it.  Without arguments it
// checks the small tables and the edges of the rules on cases of its own.  With two arguments it reads `in` — double {o[3], h}, int32
// {G, n}, n rows of 6 doubles (point, normal), then 16 doubles: the value of each cube corner (offset mask 0..7) when it is inside and
// when it is outside, iso = 0 — and writes `out`: per point int32 {i0[3], 0}, double w[8], int64 q[8][3] (rule 5); then, for every
// tetrahedron k and every inside pattern 1..14 of its corners in the cube at the origin of a grid with G = 1, int32 {n, idx[4]}: the
// polygon of rule 12 with every vertex numbered by its edge key node * 7 + type (-1 pads a triangle) — what the test compares with
// tests/ref_poisson.py.
#include "poisson_rules.h"
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int tables() {
    const int masks[7] = {1, 2, 4, 3, 5, 6, 7};
    for (int t = 0; t < 7; ++t) CHECK(pn_type_mask(t) == masks[t] && pn_mask_type(masks[t]) == t);
    const int axes[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int k = 0; k < 6; ++k) {
        int m = 0;
        CHECK(pn_tet_corner(k, 0) == 0);
        for (int i = 0; i < 3; ++i) { m |= 1 << axes[k][i]; CHECK(pn_tet_corner(k, i + 1) == m); }
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                if (i == j) continue;
                int nm, type;
                pn_tet_edge(k, i, j, &nm, &type);
                const int lo = pn_tet_corner(k, i < j ? i : j), hi = pn_tet_corner(k, i < j ? j : i);
                CHECK(nm == lo && pn_type_mask(type) == (hi & ~lo) && (lo & ~hi) == 0);
            }
    }
    CHECK(pn_edge_in_grid(4, 3, 4, 4, 0) && !pn_edge_in_grid(4, 4, 0, 0, 0) && !pn_edge_in_grid(4, 3, 4, 0, 3) && pn_edge_in_grid(4, 3, 3, 3, 6) &&
          !pn_edge_in_grid(4, 3, 3, 4, 6));
    CHECK(pn_node(4, 1, 2, 3) == (3 * 5 + 2) * 5 + 1 && pn_node(512, 512, 512, 512) == 513ll * 513 * 513 - 1);
    return 0;
}

static int points() {
    const double inf = INFINITY;
    const double p[3] = {0.0, 1.0, 2.0}, n[3] = {0.0, 0.0, 1.0}, bad1[3] = {0.0, NAN, 2.0}, bad2[3] = {0.0, 1.0, -inf};
    CHECK(pn_used(p, n) && !pn_used(bad1, n) && !pn_used(p, bad1) && !pn_used(bad2, n) && !pn_used(p, bad2));
    CHECK(pn_cell(-0.1, 0.0, 0.5, 8) == 0 && pn_cell(0.0, 0.0, 0.5, 8) == 0 && pn_cell(0.5, 0.0, 0.5, 8) == 1 && pn_cell(3.99, 0.0, 0.5, 8) == 7 &&
          pn_cell(4.0, 0.0, 0.5, 8) == 7 && pn_cell(1e300, 0.0, 0.5, 8) == 7 && pn_cell(-1e300, 0.0, 0.5, 8) == 0);
    // round to nearest even at the ties of 2^-36
    const double u = 1.0 / 68719476736.0;
    CHECK(pn_quant(0.5 * u) == 0 && pn_quant(1.5 * u) == 2 && pn_quant(2.5 * u) == 2 && pn_quant(-0.5 * u) == 0 && pn_quant(-1.5 * u) == -2 &&
          pn_quant(1.0) == 68719476736ll && pn_dequant(-3) == -3.0 * u);
    // a point on the upper faces of the cube: clamped into the last cell with f = 1; one on the lower faces: the first cell with f = 0
    PnGrid g = {{-1.0, -1.0, -1.0}, 0.25, 8};
    int i0[3];
    double w[8];
    const double top[3] = {1.0, 1.0, 1.0}, bottom[3] = {-1.0, -1.0, -1.0}, mid[3] = {-0.875, 0.0625, 0.9375};
    pn_corners_weights(top, g, i0, w);
    CHECK(i0[0] == 7 && i0[1] == 7 && i0[2] == 7 && w[7] == 1.0 && w[0] == 0.0 && w[3] == 0.0);
    pn_corners_weights(bottom, g, i0, w);
    CHECK(i0[0] == 0 && i0[1] == 0 && i0[2] == 0 && w[0] == 1.0 && w[7] == 0.0);
    pn_corners_weights(mid, g, i0, w);
    CHECK(i0[0] == 0 && i0[1] == 4 && i0[2] == 7 && w[0] == (0.5 * 0.75) * 0.25 && w[7] == (0.5 * 0.25) * 0.75 && w[2] == (0.5 * 0.25) * 0.25);
    double sum = 0.0;
    for (int c = 0; c < 8; ++c) sum += w[c];
    CHECK(sum == 1.0);
    return 0;
}

static int polygons() {
    int ci[4], co[4];
    CHECK(pn_tet_cycle(0, ci, co) == 0 && pn_tet_cycle(15, ci, co) == 0);
    CHECK(pn_tet_cycle(1 << 2, ci, co) == 3 && ci[0] == 2 && ci[2] == 2 && co[0] == 0 && co[1] == 1 && co[2] == 3);
    CHECK(pn_tet_cycle(15 ^ (1 << 1), ci, co) == 3 && co[0] == 1 && co[2] == 1 && ci[0] == 0 && ci[1] == 2 && ci[2] == 3);
    CHECK(pn_tet_cycle(0b1001, ci, co) == 4 && ci[0] == 0 && co[0] == 1 && ci[1] == 0 && co[1] == 2 && ci[2] == 3 && co[2] == 2 && ci[3] == 3 && co[3] == 1);
    // a triangle in the plane z = 0, counter-clockwise seen from +z
    const double pos[3][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}};
    const double up[3] = {0, 0, 1}, down[3] = {0, 0, -1}, flat[3] = {1, 1, 0};
    int32_t a[3] = {7, 3, 5};
    pn_polygon(3, a, pos, up);
    CHECK(a[0] == 3 && a[1] == 5 && a[2] == 7);                               // kept, rotated
    int32_t b[3] = {7, 3, 5};
    pn_polygon(3, b, pos, down);
    CHECK(b[0] == 3 && b[1] == 7 && b[2] == 5);                               // reversed, rotated
    int32_t c[3] = {7, 3, 5};
    pn_polygon(3, c, pos, flat);
    CHECK(c[0] == 3 && c[1] == 5 && c[2] == 7);                               // a zero product keeps the listed cycle
    const double quad[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
    int32_t q[4] = {9, 8, 2, 4};
    pn_polygon(4, q, quad, down);
    CHECK(q[0] == 2 && q[1] == 8 && q[2] == 9 && q[3] == 4);
    double out[3];
    const double pa[3] = {1, 2, 3}, pb[3] = {2, 2, 5};
    pn_vertex(-1.0, 3.0, pa, pb, 0.0, out);
    CHECK(out[0] == 1.25 && out[1] == 2.0 && out[2] == 3.5);
    return 0;
}

static int from_file(const char* in, const char* outp) {
    std::FILE* f = std::fopen(in, "rb");
    CHECK(f);
    PnGrid g;
    int32_t hdr[2];
    CHECK(std::fread(g.o, 8, 3, f) == 3 && std::fread(&g.h, 8, 1, f) == 1 && std::fread(hdr, 4, 2, f) == 2);
    g.G = hdr[0];
    const int n = hdr[1];
    std::unique_ptr<double[]> rows(new double[(size_t)6 * n]);                // exactly n rows: a read outside ends the program
    double val[16];
    CHECK(std::fread(rows.get(), 8, (size_t)6 * n, f) == (size_t)6 * n && std::fread(val, 8, 16, f) == 16);
    std::fclose(f);
    std::FILE* o = std::fopen(outp, "wb");
    CHECK(o);
    for (int i = 0; i < n; ++i) {
        int32_t i0[4] = {0, 0, 0, 0};
        double w[8];
        long long q[24];
        pn_corners_weights(rows.get() + 6 * i, g, i0, w);
        for (int c = 0; c < 8; ++c)
            for (int a = 0; a < 3; ++a) q[3 * c + a] = pn_quant(w[c] * rows[(size_t)6 * i + 3 + a]);
        std::fwrite(i0, 4, 4, o);
        std::fwrite(w, 8, 8, o);
        std::fwrite(q, 8, 24, o);
    }
    const PnGrid unit = {{0.0, 0.0, 0.0}, 1.0, 1};
    for (int k = 0; k < 6; ++k)
        for (int in4 = 1; in4 <= 14; ++in4) {
            int ci[4], co[4];
            const int len = pn_tet_cycle(in4, ci, co);
            CHECK(len == 3 || len == 4);
            int32_t rec[5] = {len, -1, -1, -1, -1};
            double pos[4][3], d[3];
            for (int q = 0; q < len; ++q) {
                int nm, type;
                pn_tet_edge(k, ci[q], co[q], &nm, &type);
                rec[1 + q] = (int32_t)(pn_node(unit.G, nm & 1, nm >> 1 & 1, nm >> 2 & 1) * 7 + type);
                const int mi = pn_tet_corner(k, ci[q]), mo = pn_tet_corner(k, co[q]);
                const double pa[3] = {(double)(mi & 1), (double)(mi >> 1 & 1), (double)(mi >> 2 & 1)};
                const double pb[3] = {(double)(mo & 1), (double)(mo >> 1 & 1), (double)(mo >> 2 & 1)};
                pn_vertex(val[mi], val[8 + mo], pa, pb, 0.0, pos[q]);
            }
            pn_tet_dir(k, in4, d);
            pn_polygon(len, rec + 1, pos, d);
            std::fwrite(rec, 4, 5, o);
        }
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return from_file(argv[1], argv[2]);
    if (tables() || points() || polygons()) return 1;
    std::printf("poisson rules ok\n");
    return 0;
}
