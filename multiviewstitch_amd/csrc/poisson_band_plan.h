// poisson_band_plan.h — the sizes and index arithmetic the host does for the band levels of the Poisson stage (rules 24-31,
// poisson_band_rules.h): the extents of a level's block table, the bytes a level takes, the test that its stored nodes fit an int32
// index, the row and slab tables bd_segment reads, the bytes of the density structure of rules 32-34 (16 bytes per row for rho_p and
// s_p, and the node sums dense or in blocks), the bytes of the stencil rows and block tables of rules 38-40, and the bookkeeping of
// the bytes a call holds.  Plain C++ without a HIP call:
// poisson_band.hip uses it, and tests/poisson_band_plan.cpp runs it as a program of its own under the address and undefined-behaviour
// sanitizers, on block sets of its own and at the extents of depth 10, before anything runs on a device
// (tests/poisson_band_screened_plan.cpp does the same for the screened call's part).
#ifndef MVS_POISSON_BAND_PLAN_H_
#define MVS_POISSON_BAND_PLAN_H_
#include <stddef.h>
#include <stdint.h>

#define BP_MAX_DEPTH 10                  /* MVS_POISSON_BAND_MAX_DEPTH */
#define BP_BLOCK 4                       /* MVS_POISSON_BAND_BLOCK */
#define BP_BLOCK_NODES 64                /* nodes a stored block holds: the lower corners of its 4^3 cells */
#define BP_NODE_BYTES 49                 /* per stored node: the class byte, three 8-byte planes (the sums of the splat, then r and the two p), b, chi, A p */

// The extents of level l (B + 1 <= l <= BP_MAX_DEPTH, so G >= 16): G cells, n1 = G + 1 nodes and Gb = G / 4 blocks per axis; the
// block table has T = Gb + 1 entries per axis, the node plane ix = G belonging to block index Gb, which holds no cell.
struct BdExtent {
    int32_t l, G, n1, Gb, T;
    int64_t table;                       // T^3 entries
    int64_t rows;                        // T^2 rows (bz, by) of the table
};
inline BdExtent bd_extent(int l) {
    BdExtent e;
    e.l = l;
    e.G = 1 << l;
    e.n1 = e.G + 1;
    e.Gb = e.G / BP_BLOCK;
    e.T = e.Gb + 1;
    e.rows = (int64_t)e.T * e.T;
    e.table = e.rows * e.T;
    return e;
}
inline int64_t bd_table_at(const BdExtent& e, int bx, int by, int bz) { return ((int64_t)bz * e.T + by) * e.T + bx; }

// Do `stored` blocks fit?  Node 64 * s + lane and the row 16 * s + (lz, ly) are int32 on the device.
inline bool bd_fits_int32(int64_t stored) { return stored >= 0 && stored * BP_BLOCK_NODES <= (int64_t)INT32_MAX; }

// What the stored blocks of a level take (poisson_band.hip's BdLevel): the node arrays, the packed coordinates and the six face
// neighbours of every block; and what the level's tables take whatever is stored: two bytes of work (points, dilation, stored) and
// the active byte, the int32 number of every block, the row counts and the row firsts.
inline int64_t bd_block_bytes(int64_t stored) { return stored * ((int64_t)BP_BLOCK_NODES * BP_NODE_BYTES + 4 + 24); }
inline int64_t bd_table_bytes(const BdExtent& e) { return e.table * (3 + 4) + (2 * e.rows + 1) * 4; }
// rules 10-12 over the stored nodes of level D (7 edge items and 12 face items per node, 256 items per workgroup): the sixteen row
// records of every block, the cube masks, the edge bitmap, and the counts, their scan's rows and the bases of the two compactions
inline int64_t bd_surface_bytes(int64_t stored) {
    const int64_t nodes = stored * BP_BLOCK_NODES, nbe = (7 * nodes + 255) / 256, nbf = (12 * nodes + 255) / 256;
    return 64 * stored + nodes + 32 * nbe + 13 * (nbe + nbf + 2);
}
// Can level l with `stored` blocks be held at all by a device of `device_bytes`?  (What the pool has free is not known to the caller;
// a level that exceeds the device is refused before its arrays are asked for, with the level named.)
inline int64_t bd_level_bytes(const BdExtent& e, int64_t stored, bool finest) {
    return bd_table_bytes(e) + bd_block_bytes(stored) + (finest ? bd_surface_bytes(stored) : 0);
}

// Rules 32-34, what the density structure of mvs_poisson_reconstruct_band_density holds from before the base splat until the vertex
// densities are written, for n rows: 16 bytes per row (rho_p and s_p), the partials of the reduction over the points (24 bytes for
// each of 1024 workgroups), and the int64 node sums of the density grid of depth Dd — dense, 8 (2^Dd + 1)^3 bytes, when Dd <= B; else
// in the `stored` blocks of level Dd that a cell of a used point touches: 512 bytes and the packed coordinate per block, and the int32
// number of every block of the table.  While the blocks are numbered the two work bytes per table entry, the row counts and the row
// firsts of bd_table_bytes are held too and given back (bd_density_work_bytes).
inline int64_t bd_density_bytes(int Dd, int B, int64_t stored, int64_t n) {
    const int64_t rows = 16 * n + 24 * 1024;
    if (Dd <= B) { const int64_t n1 = ((int64_t)1 << Dd) + 1; return rows + 8 * n1 * n1 * n1; }
    return rows + 4 * bd_extent(Dd).table + stored * (8 * BP_BLOCK_NODES + 4);
}
inline int64_t bd_density_work_bytes(int Dd, int B) {
    if (Dd <= B) return 0;
    const BdExtent e = bd_extent(Dd);
    return 2 * e.table + (2 * e.rows + 1) * 4;
}

// Rules 38-40, what a level of mvs_poisson_reconstruct_band_screened holds beyond bd_level_bytes while it lives.  Per stored block the
// 27 neighbours of the block (int32, offset order of rule 20) and the byte that says whether a node of it has a row; per stored node
// the int32 number of its row and the double of the preconditioner.  Per row (a node that a used point touches) BP_SC_ROW doubles —
// the 27 entries and the row sum — and the int32 place of its node.
#define BP_SC_ROW 28
inline int64_t bd_screen_block_bytes(int64_t stored) { return stored * (27 * 4 + 1 + (int64_t)BP_BLOCK_NODES * (4 + 8)); }
inline int64_t bd_screen_row_bytes(int64_t rows) { return rows * (8 * BP_SC_ROW + 4); }
// ... and while its rows are numbered: a flag byte per stored node and the counts, the scan's rows and the bases of the compaction
// (256 nodes per workgroup, 4096 workgroups per row of the scan: poisson_base.h's PnScan)
inline int64_t bd_scan_bytes(int64_t items) {
    const int64_t nb = (items + 255) / 256, rows = (nb + 4095) / 4096;
    return 4 * nb + 4 * (nb + 1) + 4 * rows * 4097 + 4 * rows + 4 * (rows + 1);
}
inline int64_t bd_screen_work_bytes(int64_t stored) { return stored * BP_BLOCK_NODES + bd_scan_bytes(stored * BP_BLOCK_NODES); }
// occupied(l) of rule 38: one bit per cell of level l while it is counted
inline int64_t bd_occupancy_bytes(int l) { return ((int64_t)1 << (3 * l)) / 8; }
// the list of the used points, kept over the levels for rules 39 and 41, and its scan while it is made (n rows, N used)
inline int64_t bd_used_bytes(int64_t n_used) { return 8 * n_used; }

// The row firsts of a level from its row counts: first[r] = the stored blocks in the rows before r (rows in (bz, by) order), first[rows]
// = all stored blocks.  -> that total, or -1 when a count is negative or exceeds T (the table cannot be right).
inline int64_t bd_row_firsts(const BdExtent& e, const int32_t* count, int32_t* first) {
    int64_t acc = 0;
    for (int64_t r = 0; r < e.rows; ++r) {
        if (count[r] < 0 || count[r] > e.T) return -1;
        first[r] = (int32_t)(acc > INT32_MAX ? INT32_MAX : acc);
        acc += count[r];
    }
    first[e.rows] = (int32_t)(acc > INT32_MAX ? INT32_MAX : acc);
    return acc;
}
// what bd_segment takes for a block of row (bz, by), read from the row firsts (host and device alike)
struct BdRowSlab { int32_t rfirst, rcnt, sfirst, scnt; };
#ifdef __HIPCC__
__host__ __device__
#endif
inline BdRowSlab bd_row_slab(const int32_t* first, int T, int by, int bz) {
    const int64_t r = (int64_t)bz * T + by, s0 = (int64_t)bz * T, s1 = s0 + T;
    BdRowSlab q;
    q.rfirst = first[r];
    q.rcnt = first[r + 1] - first[r];
    q.sfirst = first[s0];
    q.scnt = first[s1] - first[s0];
    return q;
}

// The bytes a call holds from the pool: take() and give() as blocks come and go, peak is mvs_poisson_band_info.scratch_bytes.
struct BdBytes {
    int64_t now = 0, peak = 0;
    void take(int64_t b) { now += b; if (now > peak) peak = now; }
    void give(int64_t b) { now -= b; }
};

// The capacity test of the outputs, as the plain call makes it: the counts are known, nothing has been written.
inline bool bd_capacity_ok(int64_t n_vertices, int64_t n_faces, int64_t vertex_capacity, int64_t face_capacity) {
    return n_vertices <= vertex_capacity && n_faces <= face_capacity;
}

#endif
