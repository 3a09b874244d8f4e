// Stand-alone host program for rule 32's read of mvs_poisson_reconstruct_band_density (csrc/poisson_band_rules.h: bd_node_slot,
// bd_density_at over BdBlockSums and BdDenseSums) and the bytes of the density structure (csrc/poisson_band_plan.h), the bodies the
// kernels of poisson_band.hip run.  tests/test_poisson_band_density_host.py builds it with -fsanitize=address,undefined and runs it.
// Without arguments it checks cases of its own.  With two arguments it reads `in` — double {o[3], hd}, int32 {Gd, T, ns, m}, the
// table of T^3 int32 block numbers (-1: not stored), 64 * ns int64 node sums in block storage, m rows of 3 doubles — and writes `out`:
// per row double W (rules 15 and 17 through the table), what the test compares bit for bit with tests/ref_poisson_density.py on the
// dense sums.  Every block read from the file is a heap block of exactly its size: a read through a block that is not stored, or
// past the stored ones, ends the program.
#include "poisson_band_rules.h"
#include "poisson_band_plan.h"
#include <cmath>
#include <cstdio>
#include <memory>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int own_cases() {
    CHECK(bd_density_in_blocks(5, 4) && !bd_density_in_blocks(4, 4) && !bd_density_in_blocks(2, 4) && bd_density_in_blocks(10, 9));
    // a grid of 8 cells, T = 3: only block (1, 0, 0) and its +x neighbour (2, 0, 0: the node plane ix = 8) are stored
    const PnGrid u = {{0.0, 0.0, 0.0}, 1.0, 8};
    const int T = 3;
    std::unique_ptr<int32_t[]> num(new int32_t[27]);
    for (int i = 0; i < 27; ++i) num[i] = -1;
    num[1] = 0;
    num[2] = 1;
    std::unique_ptr<long long[]> sums(new long long[128]());
    CHECK(bd_node_slot(num.get(), T, 4, 0, 0) == 0 && bd_node_slot(num.get(), T, 7, 3, 3) == 63 && bd_node_slot(num.get(), T, 8, 1, 2) == 64 + 4 + 32);
    CHECK(bd_node_slot(num.get(), T, 3, 0, 0) == -1 && bd_node_slot(num.get(), T, 4, 4, 0) == -1 && bd_node_slot(num.get(), T, 8, 8, 8) == -1);
    // one point in the middle of cell (5, 1, 2): an eighth to every corner, all stored
    const double p[3] = {5.5, 1.5, 2.5};
    int i0[3];
    double w[8];
    pn_corners_weights(p, u, i0, w);
    for (int c = 0; c < 8; ++c) sums[bd_node_slot(num.get(), T, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1))] += pn_quant(w[c]);
    const BdBlockSums B = {num.get(), T, sums.get()};
    CHECK(bd_density_at(p, u, B) == 0.125);
    const double corner[3] = {6.0, 2.0, 3.0}, far[3] = {1.0, 6.0, 6.0}, outside[3] = {99.0, 99.0, 99.0};
    CHECK(bd_density_at(corner, u, B) == 0.125 && bd_density_at(far, u, B) == 0.0 && bd_density_at(outside, u, B) == 0.0);
    // a cell half of whose corners are not stored: x = 7.5 reads the nodes ix = 7 (block 1) and ix = 8 (block 2); y = 3.5 reads iy = 4, in a row of blocks that is not stored
    std::unique_ptr<long long[]> one(new long long[128]);
    for (int i = 0; i < 128; ++i) one[i] = 1ll << 36;
    const BdBlockSums O = {num.get(), T, one.get()};
    const double half[3] = {7.5, 3.5, 0.5}, whole[3] = {7.5, 2.5, 0.5}, edge[3] = {3.5, 0.5, 0.5};
    CHECK(bd_density_at(whole, u, O) == 1.0 && bd_density_at(half, u, O) == 0.5 && bd_density_at(edge, u, O) == 0.5);
    // the same numbers from a dense array that holds the zeros
    std::unique_ptr<long long[]> dense(new long long[729]());
    for (int iz = 0; iz < 4; ++iz)
        for (int iy = 0; iy < 4; ++iy)
            for (int ix = 4; ix <= 8; ++ix) dense[pn_node(8, ix, iy, iz)] = 1ll << 36;
    const BdDenseSums D = {8, dense.get()};
    CHECK(bd_density_at(whole, u, D) == 1.0 && bd_density_at(half, u, D) == 0.5 && bd_density_at(edge, u, D) == 0.5 && bd_density_at(far, u, D) == 0.0);
    CHECK(bd_density_at(half, u, D) == pn_density_at(half, u, dense.get()));
    // the bytes: dense at or below the base depth, blocks above it
    CHECK(bd_density_bytes(4, 4, 0, 1000) == 16000 + 24 * 1024 + 8 * 17 * 17 * 17 && bd_density_work_bytes(4, 4) == 0);
    CHECK(bd_density_bytes(5, 4, 364, 8000) == 128000 + 24 * 1024 + 4 * 729 + 364 * 516 && bd_density_work_bytes(5, 4) == 2 * 729 + 4 * (2 * 81 + 1));
    // depth 10 over base 8 with density_drop 1: the table of level 9 and a surface's worth of blocks, far below the 8 * 513^3 of a dense array
    const int64_t surf = 6ll * 128 * 128;
    CHECK(bd_density_bytes(9, 8, surf, 1 << 21) < 8ll * 513 * 513 * 513 / 10 && bd_fits_int32(surf));
    return 0;
}

static int from_file(const char* in, const char* outp) {
    std::FILE* f = std::fopen(in, "rb");
    CHECK(f);
    double hd[4];
    int32_t hi[4];
    CHECK(std::fread(hd, 8, 4, f) == 4 && std::fread(hi, 4, 4, f) == 4);
    const PnGrid gd = {{hd[0], hd[1], hd[2]}, hd[3], hi[0]};
    const int T = hi[1], ns = hi[2], m = hi[3];
    CHECK(T == gd.G / BD_BLOCK + 1 && ns >= 0 && m >= 0);
    const size_t table = (size_t)T * T * T;
    std::unique_ptr<int32_t[]> num(new int32_t[table]);
    std::unique_ptr<long long[]> sums(new long long[(size_t)64 * ns]);
    std::unique_ptr<double[]> rows(new double[(size_t)3 * m]);
    CHECK(std::fread(num.get(), 4, table, f) == table && std::fread(sums.get(), 8, (size_t)64 * ns, f) == (size_t)64 * ns &&
          std::fread(rows.get(), 8, (size_t)3 * m, f) == (size_t)3 * m);
    std::fclose(f);
    for (size_t i = 0; i < table; ++i) CHECK(num[i] >= -1 && num[i] < ns);
    std::FILE* o = std::fopen(outp, "wb");
    CHECK(o);
    const BdBlockSums B = {num.get(), T, sums.get()};
    for (int i = 0; i < m; ++i) {
        const double d = bd_density_at(rows.get() + 3 * i, gd, B);
        std::fwrite(&d, 8, 1, o);
    }
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return from_file(argv[1], argv[2]);
    if (own_cases()) return 1;
    std::printf("poisson band density rules ok\n");
    return 0;
}
