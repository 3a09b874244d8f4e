// poisson_band_rules.h — band-refined levels over the dense grid of the Poisson stage (mvs_poisson_reconstruct_band): the per-point,
// per-block, per-node and per-edge decisions of rules 24-31 as one __host__ __device__ body.  The rules themselves are stated in
// include/mvs.h, behind mvs_poisson_reconstruct_screened, as rules 1-23 are.
//
// This header holds the decisions of rules 26, 27, 30 and 31: the block of a point, the dilation that makes a block active, the class
// of a node, the start value of a node, whether an edge exists and is open, and the place of a row of nodes in rule 30's order.
// poisson_band.hip runs it on the device; tests/poisson_band_rules.cpp runs it as a program of its own against
// tests/ref_poisson_band.py, the numpy / scipy restatement of the whole scheme.  A function that needs to know whether a cell is
// active, or the value of a coarse node, takes that as a callable: storage is not a rule.
// For mvs_poisson_reconstruct_band_density it holds rule 32's read: the trilinear density over a lookup that returns 0 where a node of
// the density grid is not stored (tests/poisson_band_density_rules.cpp against tests/ref_poisson_band_density.py).
#ifndef MVS_POISSON_BAND_RULES_H_
#define MVS_POISSON_BAND_RULES_H_
#include "poisson_rules.h"

#define BD_BLOCK 4                       /* MVS_POISSON_BAND_BLOCK: cells per axis of a block */
enum { BD_NONE = 0, BD_FIXED = 1, BD_FREE = 2 };

// rule 26: the block of a used point on the level of G cells of size cs (= side / G) per axis
__host__ __device__ inline void bd_point_block(const double* p, const double* o, double cs, int G, int b[3]) {
    for (int a = 0; a < 3; ++a) b[a] = pn_cell(p[a], o[a], cs, G) / BD_BLOCK;
}

// rule 26: the Chebyshev ball, one axis at a time.  in: one byte per block of a table of T^3 entries (index (bz * T + by) * T + bx)
// of which the blocks [0, Gb)^3 exist.  -> is some block at distance <= band along `axis` from (bx, by, bz) set?  Three passes,
// axis 0 over the blocks of the points, axis 1 over that result, axis 2 over that, give the active blocks.
__host__ __device__ inline bool bd_dilate_at(const uint8_t* in, int T, int Gb, int bx, int by, int bz, int axis, int band) {
    const int c = axis == 0 ? bx : axis == 1 ? by : bz;
    const int64_t stride = axis == 0 ? 1 : axis == 1 ? T : (int64_t)T * T;
    const int64_t at = ((int64_t)bz * T + by) * T + bx;
    const int lo = c - band < 0 ? 0 : c - band, hi = c + band > Gb - 1 ? Gb - 1 : c + band;
    for (int q = lo; q <= hi; ++q)
        if (in[at + (q - c) * stride]) return true;
    return false;
}

// rule 26: the class of node (ix, iy, iz) of a level of G cells; active(cx, cy, cz) answers for a cell inside the grid
template <class F>
__host__ __device__ inline int bd_node_class(int G, int ix, int iy, int iz, F active) {
    int cnt = 0;
    for (int c = 0; c < 8; ++c) {
        const int cx = ix - (c & 1), cy = iy - (c >> 1 & 1), cz = iz - (c >> 2 & 1);
        if (cx < 0 || cx >= G || cy < 0 || cy >= G || cz < 0 || cz >= G) continue;       // a cell outside the grid is not active
        cnt += active(cx, cy, cz) ? 1 : 0;
    }
    return cnt == 8 ? BD_FREE : cnt > 0 ? BD_FIXED : BD_NONE;
}

// rule 27: the start value of fine node (ix, iy, iz); coarse(jx, jy, jz) is chi of the level below at a node that has a value.
// Along x on the coarse rows, then along y, then along z: a coincident coordinate copies, a midpoint is 0.5 * (a + b).
template <class F>
__host__ __device__ inline double bd_start_value(int ix, int iy, int iz, F coarse) {
    const int x0 = ix >> 1, x1 = (ix + 1) >> 1, y0 = iy >> 1, y1 = (iy + 1) >> 1, z0 = iz >> 1, z1 = (iz + 1) >> 1;
    double yz[2];
    for (int kz = 0; kz < 2; ++kz) {
        const int jz = kz ? z1 : z0;
        double xy[2];
        for (int ky = 0; ky < 2; ++ky) {
            const int jy = ky ? y1 : y0;
            xy[ky] = x0 == x1 ? coarse(x0, jy, jz) : 0.5 * (coarse(x0, jy, jz) + coarse(x1, jy, jz));
            if (y0 == y1) break;
        }
        yz[kz] = y0 == y1 ? xy[0] : 0.5 * (xy[0] + xy[1]);
        if (z0 == z1) break;
    }
    return 0.125 * (z0 == z1 ? yz[0] : 0.5 * (yz[0] + yz[1]));
}

// rules 30-31: the edge (node (ix, iy, iz), type) of a level of G cells.  The cubes that contain it have their origin at the node,
// moved back by 0 or 1 along every axis the edge does not run along: 4 cubes for an axis edge, 2 for a face diagonal, 1 for the cube
// diagonal.  The edge exists when one of them is active.  It is open when one is active and another is not, or lies outside the
// grid: neighbours in that ring share a face that contains the edge, so some such face has an active cell on one side only.
template <class F>
__host__ __device__ inline void bd_edge_state(int G, int ix, int iy, int iz, int type, F active, bool* exists, bool* open) {
    const int m = pn_type_mask(type), z = 7 & ~m;
    bool any = false, all = true;
    for (int e = 0; e < 8; ++e) {
        if (e & ~z) continue;
        const int cx = ix - (e & 1), cy = iy - (e >> 1 & 1), cz = iz - (e >> 2 & 1);
        const bool a = cx >= 0 && cx < G && cy >= 0 && cy < G && cz >= 0 && cz < G && active(cx, cy, cz);
        any = any || a;
        all = all && a;
    }
    *exists = any;
    *open = any && !all;
}

// rule 30's order without a sort: with the stored blocks listed in (bz, by, bx) order, block number s of row (bz, by) — first[row] the
// number of the row's first block, cnt[row] its blocks; sfirst, scnt the same for the slab bz —, the row of four nodes (or cubes) at
// (ly, lz) of that block has this place in the global order (iz, iy, ix) of all stored rows
__host__ __device__ inline int64_t bd_segment(int s, int ly, int lz, int rfirst, int rcnt, int sfirst, int scnt) {
    return (int64_t)16 * sfirst + (int64_t)lz * 4 * scnt + (int64_t)4 * (rfirst - sfirst) + (int64_t)ly * rcnt + (s - rfirst);
}

// ------------------------------------------------------------------ rules 32-34: the sampling density over the band ----
// Node (ix, iy, iz) of a level kept in blocks: num[(bz * T + by) * T + bx] is the stored number of block (bx, by, bz) of a table of T
// entries per axis, -1 for a block that is not stored.  -> the node's place 64 s + lx + 4 ly + 16 lz, or -1
__host__ __device__ inline int64_t bd_node_slot(const int32_t* num, int T, int ix, int iy, int iz) {
    const int s = num[((int64_t)(iz >> 2) * T + (iy >> 2)) * T + (ix >> 2)];
    return s < 0 ? -1 : (int64_t)s * 64 + ((iz & 3) << 4 | (iy & 3) << 2 | (ix & 3));
}

// rule 32: does the density grid of depth Dd live in blocks (no array over all its nodes), or dense like the base grid of depth B?
__host__ __device__ inline bool bd_density_in_blocks(int Dd, int B) { return Dd > B; }

// rule 32: the trilinear W of rules 15 and 17 at p over the density grid gd — pn_density_at's corners, weights and order of addition.
// sum(ix, iy, iz) is the int64 node sum of rule 14, 0 at a node without storage: no used point lies in a cell around such a node, so
// its sum is 0 and the zero read is exact.
template <class F>
__host__ __device__ inline double bd_density_at(const double* p, const PnGrid& gd, F sum) {
    int i0[3];
    double w[8], v = 0.0;
    pn_corners_weights(p, gd, i0, w);
    for (int c = 0; c < 8; ++c) v = v + w[c] * pn_dequant(sum(i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1)));
    return v;
}
// sum() of bd_density_at over block storage: 64 sums per stored block behind the table of bd_node_slot.  slot: where the sum of a node
// lies, -1 for a node without storage; dense: every node has storage, known when the code is compiled
struct BdBlockSums {
    static constexpr bool dense = false;
    const int32_t* num;
    int32_t T;
    const long long* sums;
    __host__ __device__ int64_t slot(int ix, int iy, int iz) const { return bd_node_slot(num, T, ix, iy, iz); }
    __host__ __device__ long long operator()(int ix, int iy, int iz) const {
        const int64_t at = slot(ix, iy, iz);
        return at < 0 ? 0 : sums[at];
    }
};
// ... and over a dense array in node order
struct BdDenseSums {
    static constexpr bool dense = true;
    int32_t G;
    const long long* sums;
    __host__ __device__ int64_t slot(int ix, int iy, int iz) const { return pn_node(G, ix, iy, iz); }
    __host__ __device__ long long operator()(int ix, int iy, int iz) const { return sums[slot(ix, iy, iz)]; }
};

#endif
