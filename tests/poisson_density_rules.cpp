// Stand-alone host program for the per-point and per-vertex parts of rules 14-18 of mvs_poisson_reconstruct_density
// (csrc/poisson_rules.h), the body the kernels of poisson.hip run.  tests/test_poisson_density_host.py builds it with
// -fsanitize=address,undefined and runs it.  Without arguments it checks the edges of the rules on cases of its own.  With two arguments it
// reads `in` — double {o[3], side, rho_mean, max_gain}, int32 {D, drop, n, m}, n rows of 3 doubles (points), m rows of 3 doubles
// (vertices), then the (Gd + 1)^3 int64 node sums of rule 14 — and writes `out`: int32 {Dd, Gd}, double hd; per point int64 q[8] (the
// quantised weights of rule 14), double rho (15), int64 its quantised form, double s (16); per vertex double d_v (17) — what the test
// compares bit for bit with tests/ref_poisson_density.py.  Every block read from the file is a heap block of exactly its size.
#include "poisson_rules.h"
#include <cmath>
#include <cstdio>
#include <memory>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int edges() {
    const PnGrid g = {{-1.0, -2.0, -3.0}, 0.125, 32};
    int Dd = 0;
    PnGrid d = pn_density_grid(g, 4.0, 5, 1, &Dd);
    CHECK(Dd == 4 && d.G == 16 && d.h == 0.25 && d.o[0] == -1.0 && d.o[1] == -2.0 && d.o[2] == -3.0);
    d = pn_density_grid(g, 4.0, 5, 0, &Dd);
    CHECK(Dd == 5 && d.G == 32 && d.h == 0.125);
    d = pn_density_grid(g, 4.0, 3, 4, &Dd);
    CHECK(Dd == 2 && d.G == 4 && d.h == 1.0);                                 // the floor
    d = pn_density_grid(g, 4.0, 9, 8, &Dd);
    CHECK(Dd == 2 && d.G == 4);
    CHECK(pn_gain(8.0, 4.0, 4.0) == 2.0 && pn_gain(8.0, 2.0, 4.0) == 4.0 && pn_gain(8.0, 1.0, 4.0) == 4.0 && pn_gain(8.0, 0.0, 16.0) == 16.0 &&
          pn_gain(1.0, 8.0, 1.0) == 0.125);
    CHECK(pn_rho_quant(0.5 / 65536.0) == 0 && pn_rho_quant(1.5 / 65536.0) == 2 && pn_rho_quant(2.5 / 65536.0) == 2 && pn_rho_quant(3.0) == 196608);
    CHECK(pn_rho_mean(196608, 3) == 1.0 && pn_rho_mean(1, 1) == 1.0 / 65536.0);
    CHECK(pn_trim_pass(1.0, 1.0) && !pn_trim_pass(0.5, 1.0) && !pn_trim_pass(NAN, -INFINITY) && pn_trim_pass(0.0, -INFINITY) &&
          !pn_trim_pass(1e300, INFINITY) && pn_trim_pass(INFINITY, INFINITY));
    // one point in the middle of a cell of a 4^3 grid: every corner gets an eighth, and the point sees its own splat as 8 * (1/8)^2
    const PnGrid u = {{0.0, 0.0, 0.0}, 1.0, 4};
    std::unique_ptr<long long[]> sums(new long long[125]());
    const double p[3] = {1.5, 2.5, 3.5};
    int i0[3];
    double w[8];
    pn_corners_weights(p, u, i0, w);
    for (int c = 0; c < 8; ++c) sums[pn_node(u.G, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1))] += pn_quant(w[c]);
    CHECK(pn_density_at(p, u, sums.get()) == 0.125);
    const double corner[3] = {2.0, 3.0, 4.0}, outside[3] = {9.0, 9.0, 9.0}, far[3] = {0.0, 0.0, 0.0};
    CHECK(pn_density_at(corner, u, sums.get()) == 0.125 && pn_density_at(far, u, sums.get()) == 0.0);
    CHECK(std::isfinite(pn_density_at(outside, u, sums.get())));               // clamped into the last cell: reads stay inside the 125 nodes
    return 0;
}

static int from_file(const char* in, const char* outp) {
    std::FILE* f = std::fopen(in, "rb");
    CHECK(f);
    double hd[6];
    int32_t hi[4];
    CHECK(std::fread(hd, 8, 6, f) == 6 && std::fread(hi, 4, 4, f) == 4);
    const PnGrid g = {{hd[0], hd[1], hd[2]}, hd[3] / (double)(1 << hi[0]), 1 << hi[0]};
    const double rho_mean = hd[4], max_gain = hd[5];
    const int n = hi[2], m = hi[3];
    int Dd = 0;
    const PnGrid gd = pn_density_grid(g, hd[3], hi[0], hi[1], &Dd);
    const size_t nodes = (size_t)(gd.G + 1) * (gd.G + 1) * (gd.G + 1);
    std::unique_ptr<double[]> pts(new double[(size_t)3 * n]), vts(new double[(size_t)3 * m]);
    std::unique_ptr<long long[]> sums(new long long[nodes]);                   // exactly the nodes: a read outside ends the program
    CHECK(std::fread(pts.get(), 8, (size_t)3 * n, f) == (size_t)3 * n && std::fread(vts.get(), 8, (size_t)3 * m, f) == (size_t)3 * m &&
          std::fread(sums.get(), 8, nodes, f) == nodes);
    std::fclose(f);
    std::FILE* o = std::fopen(outp, "wb");
    CHECK(o);
    const int32_t head[2] = {Dd, gd.G};
    std::fwrite(head, 4, 2, o);
    std::fwrite(&gd.h, 8, 1, o);
    for (int i = 0; i < n; ++i) {
        int i0[3];
        double w[8];
        long long q[8];
        pn_corners_weights(pts.get() + 3 * i, gd, i0, w);
        for (int c = 0; c < 8; ++c) q[c] = pn_quant(w[c]);
        const double rho = pn_density_at(pts.get() + 3 * i, gd, sums.get());
        const long long rq = pn_rho_quant(rho);
        const double s = pn_gain(rho_mean, rho, max_gain);
        std::fwrite(q, 8, 8, o);
        std::fwrite(&rho, 8, 1, o);
        std::fwrite(&rq, 8, 1, o);
        std::fwrite(&s, 8, 1, o);
    }
    for (int v = 0; v < m; ++v) {
        const double d = pn_density_at(vts.get() + 3 * v, gd, sums.get());
        std::fwrite(&d, 8, 1, o);
    }
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return from_file(argv[1], argv[2]);
    if (edges()) return 1;
    std::printf("poisson density rules ok\n");
    return 0;
}
