// The byte plan of mvs_poisson_reconstruct_band_screened (csrc/poisson_band_plan.h: bd_screen_block_bytes, bd_screen_row_bytes,
// bd_screen_work_bytes, bd_scan_bytes, bd_occupancy_bytes, bd_used_bytes) against a count made array by array, as a stand-alone program
// that tests/test_poisson_band_screened_host.py builds under the address and undefined-behaviour sanitizers.  argv: stored blocks,
// rows, level, used points; prints the totals the test compares with its own.  Without arguments: its own cases, up to the extents of
// depth 10.
#include "poisson_band_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

// what csrc/poisson_band.hip asks for per level of the screened call, one array after the other
struct Arrays { int64_t nb27, has, ridx, dinv, tab, rnode, flag, scan; };
static Arrays count(int64_t stored, int64_t rows) {
    Arrays a{};
    const int64_t nodes = stored * 64;
    a.nb27 = 27 * stored * (int64_t)sizeof(int32_t);
    a.has = stored;
    a.ridx = nodes * (int64_t)sizeof(int32_t);
    a.dinv = nodes * (int64_t)sizeof(double);
    a.tab = rows * 28 * (int64_t)sizeof(double);
    a.rnode = rows * (int64_t)sizeof(int32_t);
    a.flag = nodes;
    // the scan over ceil(nodes / 256) counts: the counts, the bases (one more), 4097 entries and a total per row of 4096 counts, the row bases (one more)
    std::vector<int64_t> parts;
    const int64_t nb = (nodes + 255) / 256;
    int64_t scan_rows = 0;
    for (int64_t c = 0; c < nb; c += 4096) ++scan_rows;
    parts.push_back(4 * nb);
    parts.push_back(4 * (nb + 1));
    parts.push_back(4 * scan_rows * 4097);
    parts.push_back(4 * scan_rows);
    parts.push_back(4 * (scan_rows + 1));
    for (int64_t p : parts) a.scan += p;
    return a;
}

static int check(int64_t stored, int64_t rows) {
    const Arrays a = count(stored, rows);
    int bad = 0;
    bad += bd_screen_block_bytes(stored) != a.nb27 + a.has + a.ridx + a.dinv;
    bad += bd_screen_row_bytes(rows) != a.tab + a.rnode;
    bad += bd_screen_work_bytes(stored) != a.flag + a.scan;
    bad += bd_scan_bytes(stored * 64) != a.scan;
    if (bad) std::printf("plan differs at stored %lld rows %lld\n", (long long)stored, (long long)rows);
    return bad;
}

int main(int argc, char** argv) {
    if (argc == 5) {
        const int64_t stored = std::atoll(argv[1]), rows = std::atoll(argv[2]), used = std::atoll(argv[4]);
        const int level = std::atoi(argv[3]);
        std::printf("%lld %lld %lld %lld %lld\n", (long long)bd_screen_block_bytes(stored), (long long)bd_screen_row_bytes(rows),
                    (long long)bd_screen_work_bytes(stored), (long long)bd_occupancy_bytes(level), (long long)bd_used_bytes(used));
        return check(stored, rows);
    }
    int bad = 0;
    const int64_t most = (int64_t)INT32_MAX / 64;                            // the most blocks bd_fits_int32 lets through
    const int64_t cases[][2] = {{0, 0}, {1, 1}, {1, 64}, {3, 100}, {4095, 17}, {16384, 1000000}, {16385, 1048577}, {most, most * 64}};
    for (const auto& c : cases) bad += check(c[0], c[1]);
    bad += !bd_fits_int32(most) || bd_fits_int32(most + 1);
    bad += bd_screen_row_bytes(most * 64) != most * 64 * 228;                // 228 bytes per touched node, as the header says
    bad += bd_screen_block_bytes(1) != 109 + 64 * 12;
    for (int l = 4; l <= BP_MAX_DEPTH; ++l) bad += bd_occupancy_bytes(l) * 8 != ((int64_t)1 << (3 * l));
    bad += bd_occupancy_bytes(10) != 134217728 || bd_used_bytes((int64_t)1 << 26) != 536870912;
    if (bad) return 1;
    std::printf("poisson band screened plan ok\n");
    return 0;
}
