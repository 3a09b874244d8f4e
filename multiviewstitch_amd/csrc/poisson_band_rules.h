// poisson_band_rules.h — band-refined levels over the dense grid of the Poisson stage: the definition (rules 24-31, continuing rules
// 1-23 of include/mvs.h) and its per-point, per-block, per-node and per-edge decisions as one __host__ __device__ body.
//
// The surface occupies O(G^2) of the G^3 cells of a level; the dense grid of mvs_poisson_reconstruct pays for the empty volume and
// stops at MVS_POISSON_MAX_DEPTH = 9, while config.txt asks for PsnDptMax 10.  The band scheme solves a dense base level and refines it
// level by level on the blocks of cells near the points only, each level taking its boundary values from the level below: still fp64,
// integer splats that do not depend on their order, a stop criterion on the true residual.  It is unscreened and unweighted.  Like rules
// 1-23 these are this library's definition and are NOT VERIFIED against GeoRec.  base_depth (3 .. 9, by default 8) and band (1 .. 64
// blocks, by default 2) are its two parameters; MVS_POISSON_BAND_MAX_DEPTH is 10, MVS_POISSON_BAND_BLOCK is 4.
//  24. depth       : D = rule 3 with Dmax = min(depth_max, MVS_POISSON_BAND_MAX_DEPTH).  At depth 10 the node index and the cube
//                    index still fit in int32; a (node index, type) key needs int64.  B = min(D, base_depth).  With D <= base_depth
//                    the result is that of mvs_poisson_reconstruct at depth_min = depth_max = D.
//  25. base        : rules 4-8 at depth B give chi_B on the dense grid of that depth.
//  26. blocks      : for every level l = B + 1 .. D: G_l = 2^l, h_l = side / G_l, and the cells form blocks of MVS_POISSON_BAND_BLOCK
//                    cells per axis, G_l / 4 blocks per axis.  The block of a used point is the block of its level-l cell (rule 3's
//                    formula at d = l).  A block is active when some used point's block lies at Chebyshev distance <= band blocks
//                    from it.  A cell is active when its block is; cells outside the grid are not active.  A node is FREE when all
//                    eight cells that touch it are active, FIXED when at least one but not all of them are, and has no value
//                    otherwise.  The active set of level l - 1 covers that of level l (the same points, the same band, blocks twice
//                    as wide).
//  27. start       : every node of level l that has a value starts as 0.125 * the trilinear prolongation of chi_(l-1): a node that
//                    coincides with a coarse node copies its value, an edge midpoint is 0.5 * (a + b), and face and cube centres
//                    follow by the same halving applied axis after axis in the order x, y, z (first along x on the coarse rows,
//                    then along y on those results, then along z).  The factor is a power of two: no rounding.  Fixed nodes keep
//                    this value.  (Between two dense levels the field shrinks by 1/8 per level: the splat carries unit mass, b
//                    carries 0.5 h, the stencil is unscaled.)
//  28. system      : rules 5-6 at level l define b at the free nodes (V is needed one node beyond them; every such node has a
//                    value).  The free nodes satisfy rule 7, the terms of fixed neighbours moved to the right side: A_ff chi_f = b',
//                    b' = b - A_fc chi_c.  The solve runs until the true residual, recomputed on the device, satisfies
//                    |b' - A_ff chi|_2 <= solve_tol * |b'|_2; the norms are sums of per-workgroup partials in a fixed order, as in
//                    rule 8.  max_cycles * 64 iterations without that give MVS_E_SOLVER, with the level and the residual reported.
//                    b' = 0 gives chi_f = 0 at once.  The solver is not part of the definition; the stop criterion and the identity
//                    of two runs are.
//  29. iso value   : rule 9 on level D.  The cube of every used point is active, so its eight corners have values.
//  30. surface     : rules 10-12 over the active cubes of level D only.  An edge (node, type) exists when an active cube contains
//                    it.  Vertices are numbered in ascending (node index, type) and faces ordered by ascending cube index, then
//                    tetrahedron, then as listed, over what exists: the numbers of the dense call when every block is active.
//  31. open edges  : a crossed edge of an active cube that lies on a face shared with an inactive cell, or on the boundary of the
//                    grid, is counted in n_open_edges (once, whatever the number of such faces).  The mesh is returned as it is,
//                    open there.  Where the solve closes a scan far from every sample, level D has no field and the surface ends;
//                    mvs_processor_cull_model removes such closure anyway.
//
// This header holds the decisions of rules 26, 27, 30 and 31: the block of a point, the dilation that makes a block active, the class
// of a node, the start value of a node, whether an edge exists and is open, and the place of a row of nodes in rule 30's order.
// tests/poisson_band_rules.cpp runs it as a program of its own against tests/ref_poisson_band.py, the numpy / scipy restatement of the
// whole scheme.  No entry of the library runs the scheme yet.  A function that needs to know whether a cell is active,
// or the value of a coarse node, takes that as a callable: storage is not a rule.
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

#endif
