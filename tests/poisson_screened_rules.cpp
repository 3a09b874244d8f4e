// Stand-alone host program for the per-point part of rules 19-20 of mvs_poisson_reconstruct_screened (csrc/poisson_rules.h), the body
// the kernels of poisson.hip run.  tests/test_poisson_screened_host.py builds it with -fsanitize=address,undefined and runs it.  Without
// arguments it checks the edges of the rules on cases of its own.  With two arguments it reads `in` — double {o[3], side, lambda}, int32
// {D, n}, n rows of 3 doubles (points) — splats the stencil of rule 20 on the host with the header's pair body and writes `out`: the dense
// [(G + 1)^3][27] int64 sums, then per node the int64 row sum — what the test compares bit for bit with tests/ref_poisson_screened.py.
// Every block is a heap block of exactly its size.
#include "poisson_rules.h"
#include <cmath>
#include <cstdio>
#include <memory>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int edges() {
    CHECK(pn_screen_lambda(4.0, 100, 200) == 4.0 && pn_screen_lambda(4.0, 200, 200) == 4.0 && pn_screen_lambda(4.0, 400, 200) == 2.0 &&
          pn_screen_lambda(64.0, 3, 2) == 64.0 / 1.5 && pn_screen_lambda(0.0, 5, 1) == 0.0);
    CHECK(pn_screen_offset(-1, -1, -1) == 0 && pn_screen_offset(0, 0, 0) == 13 && pn_screen_offset(1, 1, 1) == 26 && pn_screen_offset(1, 0, 0) == 14 &&
          pn_screen_offset(0, 1, 0) == 16 && pn_screen_offset(0, 0, 1) == 22);
    double w[8];
    for (int c = 0; c < 8; ++c) w[c] = 0.125;
    int seen[27] = {0};
    for (int c1 = 0; c1 < 8; ++c1)
        for (int c2 = c1; c2 < 8; ++c2) {
            int o12, o21;
            const long long q = pn_screen_pair(2.0, w, c1, c2, &o12, &o21);
            CHECK(q == (1ll << 25));                                           // 2 / 64 * 2^30
            CHECK(o12 + o21 == 26 && o12 >= 13 && (o12 == 13) == (c1 == c2));   // opposite offsets; c2 - c1 never points backwards in z, then y, then x order
            ++seen[o12];
            if (c1 != c2) ++seen[o21];
        }
    int total = 0;
    for (int o = 0; o < 27; ++o) { CHECK(seen[o] >= 1); total += seen[o]; }    // a point in a cell reaches all 27 offsets, 64 entries in all
    CHECK(total == 64 && seen[13] == 8 && seen[0] == 1 && seen[26] == 1);
    // ties of the quantisation go to even; a zero weight gives nothing
    const double u = 1.0 / 1073741824.0;
    double t[8] = {0.5 * u, 1.0, 1.5 * u, 2.5 * u, 0.0, 1.0, 1.0, 1.0};
    int a, b;
    CHECK(pn_screen_pair(1.0, t, 0, 1, &a, &b) == 0 && pn_screen_pair(1.0, t, 1, 2, &a, &b) == 2 && pn_screen_pair(1.0, t, 1, 3, &a, &b) == 2 &&
          pn_screen_pair(64.0, t, 4, 5, &a, &b) == 0 && pn_screen_pair(64.0, t, 5, 6, &a, &b) == (1ll << 36));
    CHECK(pn_screen_dequant(1ll << 30) == 1.0 && pn_screen_dequant(3) == 3.0 * u);
    return 0;
}

static int from_file(const char* in, const char* outp) {
    std::FILE* f = std::fopen(in, "rb");
    CHECK(f);
    double hd[5];
    int32_t hi[2];
    CHECK(std::fread(hd, 8, 5, f) == 5 && std::fread(hi, 4, 2, f) == 2);
    const PnGrid g = {{hd[0], hd[1], hd[2]}, hd[3] / (double)(1 << hi[0]), 1 << hi[0]};
    const double lambda = hd[4];
    const int n = hi[1];
    const size_t nodes = (size_t)(g.G + 1) * (g.G + 1) * (g.G + 1);
    std::unique_ptr<double[]> pts(new double[(size_t)3 * n]);
    std::unique_ptr<long long[]> S(new long long[nodes * 27]()), rs(new long long[nodes]());   // exactly the nodes: a write outside ends the program
    CHECK(std::fread(pts.get(), 8, (size_t)3 * n, f) == (size_t)3 * n);
    std::fclose(f);
    for (int i = 0; i < n; ++i) {
        int i0[3];
        double w[8];
        int64_t node[8];
        pn_corners_weights(pts.get() + 3 * i, g, i0, w);
        for (int c = 0; c < 8; ++c) node[c] = pn_node(g.G, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
        for (int c1 = 0; c1 < 8; ++c1)
            for (int c2 = c1; c2 < 8; ++c2) {
                int o12, o21;
                const long long q = pn_screen_pair(lambda, w, c1, c2, &o12, &o21);
                S[node[c1] * 27 + o12] += q;
                if (c1 != c2) S[node[c2] * 27 + o21] += q;
            }
    }
    for (size_t i = 0; i < nodes; ++i)
        for (int o = 0; o < 27; ++o) rs[i] += S[i * 27 + o];
    std::FILE* o = std::fopen(outp, "wb");
    CHECK(o);
    CHECK(std::fwrite(S.get(), 8, nodes * 27, o) == nodes * 27 && std::fwrite(rs.get(), 8, nodes, o) == nodes);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return from_file(argv[1], argv[2]);
    if (edges()) return 1;
    std::printf("poisson screened rules ok\n");
    return 0;
}
