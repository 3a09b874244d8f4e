// Stand-alone host program for csrc/poisson_band_plan.h, the sizing and index arithmetic the host does for mvs_poisson_reconstruct_band.
// tests/test_poisson_band_entry_host.py builds it with the address and undefined-behaviour sanitizers and runs it: block sets of its
// own — an empty level, a full one, one stored block, blocks on the upper boundary of the grid, random ones — go through the row counts,
// bd_row_firsts and bd_row_slab as poisson_band.hip takes them, and the places bd_segment (csrc/poisson_band_rules.h) then gives must
// be the order (iz, iy, ix) of the rows of the stored blocks, every array indexed inside its bounds; then the extents, the bytes and
// the int32 test at depth 10, the byte bookkeeping and the capacity test.
#include "poisson_band_rules.h"
#include "poisson_band_plan.h"
#include <algorithm>
#include <cstdio>
#include <tuple>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// one stored set of level l: number it as the device does and hold bd_segment to the sorted order
static int one_set(int l, const std::vector<uint8_t>& stored) {
    const BdExtent e = bd_extent(l);
    CHECK((int64_t)stored.size() == e.table);
    std::vector<int32_t> cnt((size_t)e.rows, 0), first((size_t)e.rows + 1, -7), num((size_t)e.table, -1);
    for (int bz = 0; bz < e.T; ++bz)
        for (int by = 0; by < e.T; ++by)
            for (int bx = 0; bx < e.T; ++bx) cnt[(size_t)bz * e.T + by] += stored[(size_t)bd_table_at(e, bx, by, bz)];
    const int64_t ns = bd_row_firsts(e, cnt.data(), first.data());
    CHECK(ns == std::count(stored.begin(), stored.end(), (uint8_t)1) && first[0] == 0 && first[(size_t)e.rows] == ns && bd_fits_int32(ns));
    std::vector<int32_t> bx_of, by_of, bz_of;
    for (int bz = 0; bz < e.T; ++bz)
        for (int by = 0; by < e.T; ++by) {
            int32_t s = first[(size_t)bz * e.T + by];
            for (int bx = 0; bx < e.T; ++bx)
                if (stored[(size_t)bd_table_at(e, bx, by, bz)]) { num[(size_t)bd_table_at(e, bx, by, bz)] = s++; bx_of.push_back(bx); by_of.push_back(by); bz_of.push_back(bz); }
            CHECK(s == first[(size_t)bz * e.T + by + 1]);
        }
    CHECK((int64_t)bx_of.size() == ns);
    std::vector<std::tuple<int, int, int, int64_t>> rows;                     // (iz, iy, bx, place)
    std::vector<uint8_t> seen((size_t)(16 * ns), 0);
    for (int64_t s = 0; s < ns; ++s) {
        CHECK(num[(size_t)bd_table_at(e, bx_of[s], by_of[s], bz_of[s])] == s);
        const BdRowSlab q = bd_row_slab(first.data(), e.T, by_of[s], bz_of[s]);
        CHECK(q.rcnt >= 1 && q.scnt >= q.rcnt && q.sfirst <= q.rfirst && s >= q.rfirst && s < q.rfirst + q.rcnt);
        for (int lz = 0; lz < 4; ++lz)
            for (int ly = 0; ly < 4; ++ly) {
                const int64_t place = bd_segment((int)s, ly, lz, q.rfirst, q.rcnt, q.sfirst, q.scnt);
                CHECK(place >= 0 && place < 16 * ns && !seen[(size_t)place]);
                seen[(size_t)place] = 1;
                rows.emplace_back(4 * bz_of[s] + lz, 4 * by_of[s] + ly, bx_of[s], place);
            }
    }
    std::sort(rows.begin(), rows.end());
    for (size_t k = 0; k < rows.size(); ++k) CHECK(std::get<3>(rows[k]) == (int64_t)k);
    CHECK(bd_block_bytes(ns) == ns * (64 * 49 + 28) && bd_surface_bytes(ns) >= 128 * ns);
    CHECK(bd_level_bytes(e, ns, true) == bd_level_bytes(e, ns, false) + bd_surface_bytes(ns) && bd_level_bytes(e, 0, false) == bd_table_bytes(e));
    return 0;
}

static int sets() {
    unsigned seed = 2024u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int l : {4, 5}) {
        const BdExtent e = bd_extent(l);
        CHECK(e.G == 1 << l && e.n1 == e.G + 1 && e.Gb * 4 == e.G && e.T == e.Gb + 1 && e.rows == (int64_t)e.T * e.T && e.table == e.rows * e.T);
        std::vector<uint8_t> st((size_t)e.table, 0);
        if (one_set(l, st)) return 1;                                          // an empty level
        std::fill(st.begin(), st.end(), (uint8_t)1);
        if (one_set(l, st)) return 1;                                          // a full one, the entries of index Gb included
        for (int k = 0; k < 3; ++k) {                                          // one stored block: the first entry, a middle one, the last
            std::fill(st.begin(), st.end(), (uint8_t)0);
            st[(size_t)(k == 0 ? 0 : k == 1 ? e.table / 2 : e.table - 1)] = 1;
            if (one_set(l, st)) return 1;
        }
        std::fill(st.begin(), st.end(), (uint8_t)0);                           // the upper boundary of the grid: the planes of index Gb and Gb - 1
        for (int a = 0; a < e.T; ++a)
            for (int b = 0; b < e.T; ++b)
                for (int c = e.Gb - 1; c <= e.Gb; ++c) {
                    st[(size_t)bd_table_at(e, c, a, b)] = 1; st[(size_t)bd_table_at(e, a, c, b)] = 1; st[(size_t)bd_table_at(e, a, b, c)] = 1;
                }
        if (one_set(l, st)) return 1;
        for (unsigned fill : {1u, 3u, 5u}) {
            for (auto& v : st) v = rnd() % 6 < fill ? 1 : 0;
            if (one_set(l, st)) return 1;
        }
    }
    return 0;
}

static int depth10() {
    const BdExtent e = bd_extent(BP_MAX_DEPTH);
    CHECK(e.G == 1024 && e.n1 == 1025 && e.Gb == 256 && e.T == 257 && e.rows == 66049 && e.table == 16974593);
    CHECK(bd_table_at(e, e.T - 1, e.T - 1, e.T - 1) == e.table - 1);
    CHECK(bd_table_bytes(e) == 7 * e.table + 4 * (2 * e.rows + 1));
    // every block of depth 10 stored: 257^3 * 64 nodes still fit an int32; the row firsts of such a level
    CHECK(bd_fits_int32(e.table) && e.table * 64 == 1086373952ll);
    CHECK(bd_fits_int32(33554431) && !bd_fits_int32(33554432) && !bd_fits_int32(-1) && bd_fits_int32(0));
    std::vector<int32_t> cnt((size_t)e.rows, e.T), first((size_t)e.rows + 1, -7);
    CHECK(bd_row_firsts(e, cnt.data(), first.data()) == e.table && first[(size_t)e.rows] == e.table && first[1] == e.T);
    const BdRowSlab q = bd_row_slab(first.data(), e.T, e.T - 1, e.T - 1);
    CHECK(q.rcnt == e.T && q.scnt == e.T * e.T && q.rfirst == e.table - e.T && q.sfirst == e.table - (int64_t)e.T * e.T);
    const int64_t last = bd_segment((int)e.table - 1, 3, 3, q.rfirst, q.rcnt, q.sfirst, q.scnt);
    CHECK(last == 16 * e.table - 1);                                           // the last row of the last block is the last place
    CHECK((last * 4 + 3) * 7 + 6 > (int64_t)INT32_MAX);                        // ... and a (place, type) key there needs int64
    cnt[5] = e.T + 1;
    CHECK(bd_row_firsts(e, cnt.data(), first.data()) == -1);
    cnt[5] = -1;
    CHECK(bd_row_firsts(e, cnt.data(), first.data()) == -1);
    // a million stored blocks: about 3.2 GB of node arrays and 0.25 GB for the surface; every block of depth 10: 57 GB
    CHECK(bd_block_bytes(1000000) == 3164000000ll && bd_surface_bytes(1000000) > 128000000ll && bd_surface_bytes(1000000) < 1000000000ll);
    CHECK(bd_level_bytes(e, e.table, true) > 57000000000ll && bd_level_bytes(e, e.table, true) < 59000000000ll);
    CHECK(bd_surface_bytes(0) >= 0 && bd_block_bytes(0) == 0);
    return 0;
}

static int bookkeeping() {
    BdBytes b;
    b.take(100); b.take(50); b.give(100); b.take(20);
    CHECK(b.now == 70 && b.peak == 150);
    b.take(1ll << 40);
    CHECK(b.peak == 70 + (1ll << 40));
    CHECK(bd_capacity_ok(0, 0, 0, 0) && bd_capacity_ok(5, 7, 5, 7) && !bd_capacity_ok(6, 7, 5, 7) && !bd_capacity_ok(5, 8, 5, 7));
    CHECK(bd_capacity_ok(5, 7, INT64_MAX, INT64_MAX));
    return 0;
}

int main() {
    if (sets() || depth10() || bookkeeping()) return 1;
    std::printf("poisson band plan ok\n");
    return 0;
}
