// poisson_band.hip — mvs_poisson_reconstruct_band (include/mvs.h, rules 24-31): a dense base level from poisson.hip (poisson_base.h),
// then every level l = B + 1 .. D on the blocks of 4^3 cells near the points only.  poisson_band_rules.h makes every decision — the
// block of a point, the dilation, the class of a node, its start value, the state of an edge, the place of a row in rule 30's order —;
// poisson_band_plan.h does the host's sizing; this file stores and moves.
//
// A level keeps a table of T = G / 4 + 1 entries per axis (the node plane ix = G belongs to block index G / 4) and, for every STORED
// block — an active one, or one that holds a node with a value: a block whose neighbour at offset -1 along any subset of axes is
// active —, 64 nodes (the lower corners of its 4^3 cells) in planar arrays: node 64 s + lx + 4 ly + 16 lz.  One wave owns one block, so a
// wave's loads and stores are one contiguous 512-byte run per array; the in-block neighbours come by wave shuffle, the 16 lanes of
// each face read the face neighbour's run (its number is in the block's six-entry neighbour list).
//
//   k_bd_occupy / k_bd_popcount           rule 24: rule 3's occupied cells, one candidate depth at a time (depth 10 included)
//   k_bd_mark / k_bd_dilate / k_bd_stored rule 26: the blocks of the points (plain byte stores of 1), three bd_dilate_at passes, the stored blocks
//   k_bd_row_count / k_bd_number          the stored blocks numbered in (bz, by, bx) order: a wave per table row counts and ranks by
//                                         ballot, the host scans the T^2 row counts (bd_row_firsts; it needs the total anyway).  No atomic counter
//   k_bd_neighbours / k_bd_rows           the six face neighbours of every block; on level D the block and row behind every place of bd_segment
//   k_bd_class_start<Coarse>              rules 26-27: the class byte and the start value, from the dense chi_B or the level below's blocks
//   k_bd_splat<WEIGHTED> / k_bd_rhs       rules 5-6 into block storage: int64 atomic adds (WEIGHTED: rule 33, the normals times s_p), then b at the free nodes
//   k_bd_bnorm                            |b'|^2, b' = b - A_fc chi_c: the stencil over the vector of the fixed values and zeros
//   k_bd_residual<WRITE>                  the TRUE residual of the free nodes from chi and b (fixed neighbours included: the same number
//                                         as b' - A_ff chi_f); WRITE: it becomes r of the solve
//   k_bd_apply / k_bd_update              rule 28's solve, conjugate gradients on 6 x - S = -b' from the start values: p = r + beta p
//                                         and A p fused with the p . A p partials; x, r updated fused with the r . r partials.  Every
//                                         workgroup folds the (at most BD_NPART) partials of the launch before in a fixed order: the
//                                         step lengths never leave the device, the host reads one number per 64 iterations
//   k_bd_used_count / k_bd_used_scatter / k_bd_iso
//                                         rule 29: the reduction of k_pn_iso through the block table, over the used rows listed in
//                                         their order by an ordered compaction, so rows that are not used move no bit of the iso value
//   BdSurf                                rules 30-31: the view through which the extraction of poisson_surface.h (k_pn_cubemask,
//                                         k_pn_edge_count, k_pn_vertex_scatter, k_pn_face_scatter) sees the stored nodes in the order
//                                         bd_segment gives them, items = (place of the node) * 7 + type resp. * 12 + slot (int64)
// What the dense stage has already, it lends (poisson_base.h): the folds and the vertex numbering (poisson_dev.h), the scan between a
// count and a scatter kernel (PnScan), the sum of partials by one workgroup (poisson_fold), the face count and the tail of a call.
// mvs_poisson_reconstruct_band_density (rules 32-35) carries the sampling density of rules 14-17 over every level.  The int64 sums of
// the density grid of depth Dd lie dense when Dd <= B and else in the blocks of level Dd that a cell of a used point touches
// (k_bd_mark without the dilation, k_bd_stored, k_bd_row_count, k_bd_number: the table of a level, 8 bytes per stored node); a node
// without storage reads as 0 (bd_density_at of poisson_band_rules.h).  The kernels of rules 14-17 are poisson.hip's, instantiated for
// either storage (PnDensitySums, poisson_density_rows, poisson_vertex_density of poisson_base.h).
// mvs_poisson_reconstruct_band_screened (rules 36-41) screens the base (PnBaseField with sparams) and every level: the k_bd_sc_* kernels
// below number the rows over the stored node places, splat rule 38's stencil and solve M_ff chi_f = f' in the place of rule 28's system.
// BdRun runs the stages in the order depth, density, base, levels, iso, mesh, vertex density.
// Nothing but integer atomics (the splats, the bitmap, the count of open edges) is unordered: two runs give the same bytes.
#include "engine.h"
#include "trace.h"
#include "frontend_dev.h"
#include "poisson_dev.h"
#include "poisson_surface.h"
#include "poisson_band_rules.h"
#include "poisson_band_plan.h"
#include "poisson_base.h"
#include "knobs.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

static_assert(BP_MAX_DEPTH == MVS_POISSON_BAND_MAX_DEPTH && BP_BLOCK == MVS_POISSON_BAND_BLOCK && BD_BLOCK == MVS_POISSON_BAND_BLOCK, "one block size, one depth limit");

namespace {

constexpr int BD_RED_NB = 1024;          // workgroups of a reduction over the points
constexpr int BD_NPART = 1024;           // workgroups of a solver launch at most: the partials every workgroup folds
constexpr int BD_MAX_D = MVS_POISSON_BAND_MAX_DEPTH;

// ------------------------------------------------------------------ rule 24 ----
__global__ __launch_bounds__(PN_TPB) void k_bd_occupy(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g,
                                                      unsigned* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    const int m = g.G;
    const int64_t cell = ((int64_t)pn_cell(pts[3 * i + 2], g.o[2], g.h, m) * m + pn_cell(pts[3 * i + 1], g.o[1], g.h, m)) * m + pn_cell(pts[3 * i], g.o[0], g.h, m);
    atomicOr(bits + (cell >> 5), 1u << (cell & 31));
}
__global__ __launch_bounds__(PN_TPB) void k_bd_popcount(int64_t words, const unsigned* __restrict__ bits, unsigned long long* __restrict__ occupied) {
    const int64_t w = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const unsigned v = w < words ? bits[w] : 0u;
    if (v) atomicAdd(occupied, (unsigned long long)__popc(v));
}

// ------------------------------------------------------------------ the level as the kernels see it ----
struct BdView {
    int32_t G, T, Gb;
    const uint8_t* act;                   // T^3: is the block active?
    const int32_t* num;                   // T^3: the stored number of the block, -1: not stored
    const int32_t* first;                 // T^2 + 1: the row firsts (bd_row_firsts)
};
__device__ inline int64_t bd_tab(const BdView& v, int bx, int by, int bz) { return ((int64_t)bz * v.T + by) * v.T + bx; }
struct BdActive {
    BdView v;
    __device__ bool operator()(int cx, int cy, int cz) const { return v.act[bd_tab(v, cx >> 2, cy >> 2, cz >> 2)] != 0; }
};
// node (ix, iy, iz) in [0, G]^3 -> its place 64 s + lane in the node arrays, -1 when its block is not stored
__device__ inline int64_t bd_slot(const BdView& v, int ix, int iy, int iz) { return bd_node_slot(v.num, v.T, ix, iy, iz); }
__host__ __device__ inline void bd_unpack(int32_t c, int* bx, int* by, int* bz) { *bx = c & 1023; *by = c >> 10 & 1023; *bz = c >> 20 & 1023; }

// ------------------------------------------------------------------ rule 26 ----
__global__ __launch_bounds__(PN_TPB) void k_bd_mark(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g, int T,
                                                    uint8_t* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int b[3];
    bd_point_block(pts + 3 * i, g.o, g.h, g.G, b);
    tab[((int64_t)b[2] * T + b[1]) * T + b[0]] = 1;
}

__global__ __launch_bounds__(PN_TPB) void k_bd_dilate(int T, int Gb, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int axis, int band) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= (int64_t)T * T * T) return;
    const int bx = (int)(at % T), by = (int)(at / T % T), bz = (int)(at / ((int64_t)T * T));
    out[at] = bx < Gb && by < Gb && bz < Gb && bd_dilate_at(in, T, Gb, bx, by, bz, axis, band) ? 1 : 0;
}

__global__ __launch_bounds__(PN_TPB) void k_bd_stored(int T, const uint8_t* __restrict__ act, uint8_t* __restrict__ stored) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= (int64_t)T * T * T) return;
    const int bx = (int)(at % T), by = (int)(at / T % T), bz = (int)(at / ((int64_t)T * T));
    bool any = false;
    for (int c = 0; c < 8; ++c) {
        const int qx = bx - (c & 1), qy = by - (c >> 1 & 1), qz = bz - (c >> 2 & 1);
        if (qx < 0 || qy < 0 || qz < 0) continue;
        any = any || act[((int64_t)qz * T + qy) * T + qx];
    }
    stored[at] = any ? 1 : 0;
}

// a wave per row (bz, by) of the table: how many of its T blocks are stored
__global__ __launch_bounds__(PN_TPB) void k_bd_row_count(int T, const uint8_t* __restrict__ stored, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * PN_WAVES + (threadIdx.x >> 6);
    if (row >= (int64_t)T * T) return;                                       // the whole wave
    int acc = 0;
    for (int c0 = 0; c0 < T; c0 += 64) {
        const bool f = c0 + lane < T && stored[row * T + c0 + lane];
        acc += __popcll(__ballot(f));
    }
    if (lane == 0) cnt[row] = acc;
}

// ... and their numbers, ascending along the row from the row's first; coord[s] = bx | by << 10 | bz << 20
__global__ __launch_bounds__(PN_TPB) void k_bd_number(int T, const uint8_t* __restrict__ stored, const int32_t* __restrict__ first,
                                                      int32_t* __restrict__ num, int32_t* __restrict__ coord) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * PN_WAVES + (threadIdx.x >> 6);
    if (row >= (int64_t)T * T) return;
    int acc = first[row];
    for (int c0 = 0; c0 < T; c0 += 64) {
        const int bx = c0 + lane;
        const bool f = bx < T && stored[row * T + bx];
        const unsigned long long bal = __ballot(f);
        const int s = acc + __popcll(bal & ((1ull << lane) - 1ull));
        if (bx < T) num[row * T + bx] = f ? s : -1;
        if (f) coord[s] = bx | (int)(row % T) << 10 | (int)(row / T) << 20;
        acc += __popcll(bal);
    }
}

// nbr[6 s + f]: the stored number of the neighbour of block s across face f = -x, +x, -y, +y, -z, +z; -1: none
__global__ __launch_bounds__(PN_TPB) void k_bd_neighbours(int64_t ns, const int32_t* __restrict__ coord, BdView v, int32_t* __restrict__ nbr) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= 6 * ns) return;
    const int f = (int)(i % 6);
    int b[3];
    bd_unpack(coord[i / 6], &b[0], &b[1], &b[2]);
    b[f >> 1] += f & 1 ? 1 : -1;
    nbr[i] = b[f >> 1] < 0 || b[f >> 1] >= v.T ? -1 : v.num[bd_tab(v, b[0], b[1], b[2])];
}

// rows[place] = 16 s + 4 lz + ly for the row of four nodes at (ly, lz) of block s, place = bd_segment: the stored rows in (iz, iy, ix) order
__global__ __launch_bounds__(PN_TPB) void k_bd_rows(int64_t ns, const int32_t* __restrict__ coord, BdView v, int32_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= 16 * ns) return;
    const int s = (int)(i >> 4), ly = (int)(i & 3), lz = (int)(i >> 2 & 3);
    int bx, by, bz;
    bd_unpack(coord[s], &bx, &by, &bz);
    const BdRowSlab q = bd_row_slab(v.first, v.T, by, bz);
    rows[bd_segment(s, ly, lz, q.rfirst, q.rcnt, q.sfirst, q.scnt)] = (int32_t)i;
}

// ------------------------------------------------------------------ rules 26-27 ----
struct BdDenseCoarse {                   // chi_B on the dense grid of Gc cells
    const double* chi;
    int Gc;
    __device__ double operator()(int jx, int jy, int jz) const { return chi[pn_node(Gc, jx, jy, jz)]; }
};
struct BdBlockCoarse {                   // chi of the level below in its blocks; rule 26's nesting: the node is stored
    BdView v;
    const double* chi;
    __device__ double operator()(int jx, int jy, int jz) const {
        const int64_t at = bd_slot(v, jx, jy, jz);
        return at < 0 ? NAN : chi[at];
    }
};

template <class Coarse>
__global__ __launch_bounds__(PN_TPB) void k_bd_class_start(int64_t ns, const int32_t* __restrict__ coord, BdView v, Coarse coarse,
                                                           uint8_t* __restrict__ cls, double* __restrict__ x) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= 64 * ns) return;
    const int lane = (int)(at & 63);
    int bx, by, bz;
    bd_unpack(coord[at >> 6], &bx, &by, &bz);
    const int ix = 4 * bx + (lane & 3), iy = 4 * by + (lane >> 2 & 3), iz = 4 * bz + (lane >> 4);
    int c = BD_NONE;
    if (ix <= v.G && iy <= v.G && iz <= v.G) c = bd_node_class(v.G, ix, iy, iz, BdActive{v});
    cls[at] = (uint8_t)c;
    x[at] = c == BD_NONE ? 0.0 : bd_start_value(ix, iy, iz, coarse);
}

// ------------------------------------------------------------------ rules 5-6 in block storage ----
// WEIGHTED: rule 33, every normal scaled by the gain s_p of its point (k_pn_splat<true>'s expression)
template <bool WEIGHTED>
__global__ __launch_bounds__(PN_TPB) void k_bd_splat(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g, BdView v,
                                                     int64_t nodes, unsigned long long* __restrict__ sums, const double* __restrict__ gain) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int i0[3];
    double w[8], na[3];
    pn_corners_weights(pts + 3 * i, g, i0, w);
    for (int a = 0; a < 3; ++a) na[a] = WEIGHTED ? nrm[3 * i + a] * gain[i] : nrm[3 * i + a];
    for (int c = 0; c < 8; ++c) {
        const int64_t at = bd_slot(v, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
        if (at < 0) continue;                                                // rule 29: cannot be, the cube of a used point is active
        for (int a = 0; a < 3; ++a) atomicAdd(sums + a * nodes + at, (unsigned long long)pn_quant(w[c] * na[a]));
    }
}

// the places of the six neighbours of node `lane` of block s, in the order of nbr; -1: in a block that is not stored
__device__ inline void bd_nb_slots(const int32_t* __restrict__ nb, int64_t s, int lane, int64_t at[6]) {
    const int l[3] = {lane & 3, lane >> 2 & 3, lane >> 4};
    for (int a = 0; a < 3; ++a) {
        const int st = 1 << (2 * a);
        at[2 * a] = l[a] > 0 ? s * 64 + lane - st : nb[2 * a] >= 0 ? (int64_t)nb[2 * a] * 64 + lane + 3 * st : -1;
        at[2 * a + 1] = l[a] < 3 ? s * 64 + lane + st : nb[2 * a + 1] >= 0 ? (int64_t)nb[2 * a + 1] * 64 + lane - 3 * st : -1;
    }
}

// rule 6 at the free nodes (k_pn_rhs's expression); 0 elsewhere
__global__ __launch_bounds__(PN_TPB) void k_bd_rhs(int64_t ns, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ cls, int64_t nodes,
                                                   const long long* __restrict__ sums, double h, double* __restrict__ b) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= 64 * ns) return;
    double val = 0.0;
    if (cls[at] == BD_FREE) {
        int64_t q[6];
        bd_nb_slots(nbr + 6 * (at >> 6), at >> 6, (int)(at & 63), q);
        const long long *sx = sums, *sy = sums + nodes, *sz = sums + 2 * nodes;
        // every neighbour of a free node has a value, so its block is stored and no q is -1; a table that broke that must not read outside
        const auto V = [](const long long* a, int64_t i) { return i < 0 ? 0.0 : pn_dequant(a[i]); };
        val = (((V(sx, q[1]) - V(sx, q[0])) + (V(sy, q[3]) - V(sy, q[2]))) + (V(sz, q[5]) - V(sz, q[4]))) * (0.5 * h);
    }
    b[at] = val;
}

// ------------------------------------------------------------------ rule 28 ----
// The six-neighbour sum of a planar quantity at node `lane` of the wave's block (every lane of the wave calls it): own the lane's value,
// load(place) the same quantity anywhere; the neighbours inside the block come by shuffle, those across a face from the neighbour's
// run, 0 where that block is not stored (only beside nodes that are not free).  The order of pn_nbr_sum.
template <class F>
__device__ inline double bd_sum6(double own, const int32_t* __restrict__ nb, int lane, F load) {
    const int lx = lane & 3, ly = lane >> 2 & 3, lz = lane >> 4;
    double xm = __shfl(own, (lane + 63) & 63, 64), xp = __shfl(own, (lane + 1) & 63, 64);
    double ym = __shfl(own, (lane + 60) & 63, 64), yp = __shfl(own, (lane + 4) & 63, 64);
    double zm = __shfl(own, (lane + 48) & 63, 64), zp = __shfl(own, (lane + 16) & 63, 64);
    if (lx == 0) xm = nb[0] >= 0 ? load((int64_t)nb[0] * 64 + lane + 3) : 0.0;
    if (lx == 3) xp = nb[1] >= 0 ? load((int64_t)nb[1] * 64 + lane - 3) : 0.0;
    if (ly == 0) ym = nb[2] >= 0 ? load((int64_t)nb[2] * 64 + lane + 12) : 0.0;
    if (ly == 3) yp = nb[3] >= 0 ? load((int64_t)nb[3] * 64 + lane - 12) : 0.0;
    if (lz == 0) zm = nb[4] >= 0 ? load((int64_t)nb[4] * 64 + lane + 48) : 0.0;
    if (lz == 3) zp = nb[5] >= 0 ? load((int64_t)nb[5] * 64 + lane - 48) : 0.0;
    return ((xm + xp) + (ym + yp)) + (zm + zp);
}

// The launches of the solve: wave w of the launch takes the blocks w, w + waves, ...; a workgroup leaves one partial.
#define BD_EACH_BLOCK(s) for (int64_t s = (int64_t)blockIdx.x * PN_WAVES + (threadIdx.x >> 6); s < ns; s += (int64_t)gridDim.x * PN_WAVES)

// |b'|^2 over the free nodes, b' = b - (the stencil over the fixed values and zeros)
__global__ __launch_bounds__(PN_TPB) void k_bd_bnorm(int64_t ns, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ cls,
                                                     const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ part) {
    __shared__ double s_part[PN_WAVES];
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        const int c = cls[at];
        const double fx = c == BD_FIXED ? x[at] : 0.0;
        const double S = bd_sum6(fx, nbr + 6 * s, lane, [&](int64_t q) { return cls[q] == BD_FIXED ? x[q] : 0.0; });
        const double bp = c == BD_FREE ? b[at] - S : 0.0;
        acc += bp * bp;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// the residual of 6 x - S = -b at the free nodes, x with the fixed values in place: (S - 6 x) - b, 0 at the other nodes.  Its squared norm
// per workgroup; WRITE: r, the start of the solve.
template <bool WRITE>
__global__ __launch_bounds__(PN_TPB) void k_bd_residual(int64_t ns, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ cls,
                                                        const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ r,
                                                        double* __restrict__ part) {
    __shared__ double s_part[PN_WAVES];
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        const double xv = x[at];
        const double S = bd_sum6(xv, nbr + 6 * s, lane, [&](int64_t q) { return x[q]; });
        const double rv = cls[at] == BD_FREE ? (S - 6.0 * xv) - b[at] : 0.0;
        if (WRITE) r[at] = rv;
        acc += rv * rv;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// p = r + beta p_old (beta = rr / rr_before, 0 in the first iteration), A p = 6 p - S(p) at the free nodes, and the partials of p . A p.
// r and p are 0 at the nodes that are not free, so the neighbour's new p is r + beta p_old there too.
__global__ __launch_bounds__(PN_TPB) void k_bd_apply(int64_t ns, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ cls, int first, int np,
                                                     const double* __restrict__ rr, const double* __restrict__ rr_before,
                                                     const double* __restrict__ r, const double* __restrict__ p_old, double* __restrict__ p,
                                                     double* __restrict__ ap, double* __restrict__ part) {
    __shared__ double s_a[PN_WAVES], s_b[PN_WAVES], s_part[PN_WAVES], s_o[2];
    double beta = 0.0;
    if (!first) {
        const double n = wg_sum_partials_all(rr, np, s_a, s_o), d = wg_sum_partials_all(rr_before, np, s_b, s_o + 1);
        beta = d > 0.0 ? n / d : 0.0;
    }
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        const double pv = r[at] + beta * p_old[at];
        const double S = bd_sum6(pv, nbr + 6 * s, lane, [&](int64_t q) { return r[q] + beta * p_old[q]; });
        const double av = cls[at] == BD_FREE ? 6.0 * pv - S : 0.0;
        p[at] = pv;
        ap[at] = av;
        acc += pv * av;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// alpha = rr / (p . A p); x += alpha p, r -= alpha A p, and the partials of the new r . r
__global__ __launch_bounds__(PN_TPB) void k_bd_update(int64_t ns, int np, const double* __restrict__ rr, const double* __restrict__ pap,
                                                      const double* __restrict__ p, const double* __restrict__ ap, double* __restrict__ x,
                                                      double* __restrict__ r, double* __restrict__ part) {
    __shared__ double s_a[PN_WAVES], s_b[PN_WAVES], s_part[PN_WAVES], s_o[2];
    const double n = wg_sum_partials_all(rr, np, s_a, s_o), d = wg_sum_partials_all(pap, np, s_b, s_o + 1);
    const double alpha = d > 0.0 ? n / d : 0.0;
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        x[at] = x[at] + alpha * p[at];
        const double rv = r[at] - alpha * ap[at];
        r[at] = rv;
        acc += rv * rv;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(PN_TPB) void k_bd_zero_free(int64_t nodes, const uint8_t* __restrict__ cls, double* __restrict__ x) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at < nodes && cls[at] == BD_FREE) x[at] = 0.0;
}

// how many nodes are free: integers
__global__ __launch_bounds__(PN_TPB) void k_bd_count_free(int64_t nodes, const uint8_t* __restrict__ cls, unsigned long long* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const unsigned long long bal = __ballot(at < nodes && cls[at] == BD_FREE);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(out, (unsigned long long)__popcll(bal));
}
__global__ __launch_bounds__(PN_TPB) void k_bd_count_set(int64_t n, const uint8_t* __restrict__ flag, unsigned long long* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const unsigned long long bal = __ballot(at < n && flag[at]);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(out, (unsigned long long)__popcll(bal));
}

// ------------------------------------------------------------------ rules 38-40 ----
// mvs_poisson_reconstruct_band_screened: the stencil rows of level l over the stored node places, and the solve of M_ff chi_f = f'.
//   k_bd_sc_flag / k_bd_sc_count / k_bd_sc_number   plain byte stores of 1 at the places the points touch (and at their blocks), then an
//                                                   ordered compaction over the places: ridx[place] = the number of its row or -1,
//                                                   rnode[row] = its place.  No atomic counter
//   k_bd_nb27                                       the 27 blocks around every stored block, in the offset order of rule 20
//   k_bd_sc_splat                                   rule 38 through the block table: pn_screen_pair and int64 atomic adds (order-free);
//                                                   poisson_screen_convert makes the sums doubles in place
//   k_bd_sc_rhs / k_bd_sc_dinv                      f = b - T_l rs at the rows; the inverse diagonal 1 / (6 + S_{i,0}) of every place
//   k_bd_sc_residual / k_bd_sc_apply / k_bd_sc_update   k_bd_residual / apply / update with the stencil term and the preconditioner.
//                                                   A wave whose block has a row stages its 64 values and the one-node halo around
//                                                   them, 6^3 doubles, in its own part of LDS, and the lanes with a row read their 27
//                                                   operands there; a wave whose block has none takes the plain path: the branch is
//                                                   uniform over the wave, and most stored blocks lie in the band, not on the surface
// Rule 38: every neighbour of a node with a row is stored, so no operand of a row is missing; a table that broke that reads 0.
constexpr int BD_HALO = 6 * 6 * 6;
struct BdScreen {
    const int32_t* nb27;                  // 27 per stored block, -1: not stored
    const uint8_t* has;                   // per stored block: does a node of it have a row?
    const int32_t* ridx;                  // per place: the number of its row, -1: none
    const double* tab;                    // PN_SC_ROW doubles per row
};

__global__ __launch_bounds__(PN_TPB) void k_bd_sc_flag(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g, BdView v,
                                                       uint8_t* __restrict__ flag, uint8_t* __restrict__ has) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int i0[3];
    double w[8];
    pn_corners_weights(pts + 3 * i, g, i0, w);
    for (int c = 0; c < 8; ++c) {
        const int64_t at = bd_slot(v, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
        if (at < 0) continue;                                                // rule 29: cannot be
        flag[at] = 1;
        has[at >> 6] = 1;
    }
}
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_count(int64_t nodes, const uint8_t* __restrict__ flag, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const WgRank k = wg_rank<PN_WAVES>(at < nodes && flag[at], s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_number(int64_t nodes, const uint8_t* __restrict__ flag, const int32_t* __restrict__ base,
                                                         int32_t* __restrict__ ridx, int32_t* __restrict__ rnode) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const bool f = at < nodes && flag[at];
    const int pos = base[blockIdx.x] + wg_rank<PN_WAVES>(f, s_wsum).rank;
    if (at < nodes) ridx[at] = f ? pos : -1;
    if (f) rnode[pos] = (int32_t)at;
}

// nb27[27 s + o]: the stored number of the block at offset o = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) from block s (o = 13: s); -1: none
__global__ __launch_bounds__(PN_TPB) void k_bd_nb27(int64_t ns, const int32_t* __restrict__ coord, BdView v, int32_t* __restrict__ nb27) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= 27 * ns) return;
    const int o = (int)(i % 27);
    int bx, by, bz;
    bd_unpack(coord[i / 27], &bx, &by, &bz);
    bx += o % 3 - 1; by += o / 3 % 3 - 1; bz += o / 9 - 1;
    nb27[i] = bx < 0 || bx >= v.T || by < 0 || by >= v.T || bz < 0 || bz >= v.T ? -1 : v.num[bd_tab(v, bx, by, bz)];
}

__global__ __launch_bounds__(PN_TPB) void k_bd_sc_splat(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g, BdView v,
                                                        double lambda, const int32_t* __restrict__ ridx, unsigned long long* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int i0[3];
    double w[8];
    int64_t row[8];
    pn_corners_weights(pts + 3 * i, g, i0, w);
    bool ok = true;
    for (int c = 0; c < 8; ++c) {
        const int64_t at = bd_slot(v, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
        const int a = at < 0 ? -1 : ridx[at];
        ok = ok && a >= 0;                                                   // flagged by k_bd_sc_flag: >= 0
        row[c] = (int64_t)PN_SC_ROW * a;
    }
    if (!ok) return;
    for (int c1 = 0; c1 < 8; ++c1)
        for (int c2 = c1; c2 < 8; ++c2) {
            int o12, o21;
            const unsigned long long q = (unsigned long long)pn_screen_pair(lambda, w, c1, c2, &o12, &o21);
            atomicAdd(tab + row[c1] + o12, q);
            if (c1 != c2) atomicAdd(tab + row[c2] + o21, q);
        }
}

// rule 40's f = b - T rs at the rows (all at free nodes: rule 38)
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_rhs(int64_t rows, const int32_t* __restrict__ rnode, const uint8_t* __restrict__ cls,
                                                      const double* __restrict__ tab, double T, double* __restrict__ b) {
    const int64_t a = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (a >= rows) return;
    const int64_t at = rnode[a];
    if (cls[at] == BD_FREE) b[at] = b[at] - T * tab[(int64_t)PN_SC_ROW * a + 27];
}

// the preconditioner: 1 / (6 + S_{i,0}) with a row, 1 / 6 without; JACOBI = false: 1, plain conjugate gradients
template <bool JACOBI>
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_dinv(int64_t nodes, const int32_t* __restrict__ ridx, const double* __restrict__ tab,
                                                       double* __restrict__ dinv) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= nodes) return;
    const int a = ridx[at];
    dinv[at] = !JACOBI ? 1.0 : 1.0 / (6.0 + (a < 0 ? 0.0 : tab[(int64_t)PN_SC_ROW * a + 13]));
}

// sum_o S_{i,o} x_{i+o} at node `lane` of block s, 0 at a lane without a row; every lane of the wave calls it, and only when q.has[s].
// own: the lane's x; load(place): x anywhere; halo: the wave's BD_HALO doubles of LDS.
template <class F>
__device__ inline double bd_sc_term(const BdScreen& q, int64_t s, int lane, double own, double* halo, F load) {
    const int lx = lane & 3, ly = lane >> 2 & 3, lz = lane >> 4;
    const int32_t* nb = q.nb27 + 27 * s;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                   // the reads of the block before are done
    __builtin_amdgcn_wave_barrier();
    halo[(lz + 1) * 36 + (ly + 1) * 6 + (lx + 1)] = own;
    for (int h = lane; h < BD_HALO; h += 64) {
        const int hx = h % 6, hy = h / 6 % 6, hz = h / 36;
        const int ox = hx == 0 ? 0 : hx == 5 ? 2 : 1, oy = hy == 0 ? 0 : hy == 5 ? 2 : 1, oz = hz == 0 ? 0 : hz == 5 ? 2 : 1;
        if (ox == 1 && oy == 1 && oz == 1) continue;                          // inside the block: written above
        const int32_t b = nb[oz * 9 + oy * 3 + ox];
        halo[h] = b >= 0 ? load((int64_t)b * 64 + (((hz - 1) & 3) << 4 | ((hy - 1) & 3) << 2 | ((hx - 1) & 3))) : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int a = q.ridx[s * 64 + lane];
    double acc = 0.0;
    if (a >= 0) {
        const double* __restrict__ row = q.tab + (int64_t)PN_SC_ROW * a;
        const double* c = halo + lz * 36 + ly * 6 + lx;                      // the node at offset (-1, -1, -1)
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = acc + row[k] * c[(k / 9) * 36 + (k / 3 % 3) * 6 + k % 3];
    }
    return acc;
}

// k_bd_residual with the stencil term: (S6 - 6 x) - sum_o S_o x_o - f at the free nodes.  WRITE: r, and the partials of r . (r dinv) too
template <bool WRITE>
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_residual(int64_t ns, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ cls, BdScreen q,
                                                           const double* __restrict__ x, const double* __restrict__ b,
                                                           const double* __restrict__ dinv, double* __restrict__ r, double* __restrict__ part,
                                                           double* __restrict__ part_z) {
    __shared__ double s_part[PN_WAVES], s_z[PN_WAVES], s_halo[PN_WAVES][BD_HALO];
    const int lane = threadIdx.x & 63;
    double acc = 0.0, accz = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        const double xv = x[at];
        const double S = bd_sum6(xv, nbr + 6 * s, lane, [&](int64_t p) { return x[p]; });
        double rv = (S - 6.0 * xv) - b[at];
        if (q.has[s]) rv = rv - bd_sc_term(q, s, lane, xv, s_halo[threadIdx.x >> 6], [&](int64_t p) { return x[p]; });
        if (cls[at] != BD_FREE) rv = 0.0;
        if (WRITE) { r[at] = rv; accz += rv * (rv * dinv[at]); }
        acc += rv * rv;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
    if (WRITE) {
        const double tz = wg_sum<PN_WAVES>(accz, s_z, threadIdx.x);
        if (threadIdx.x == 0) part_z[blockIdx.x] = tz;
    }
}

// k_bd_apply on -M_ff with the preconditioner: p = r dinv + beta p_old (beta = rz / rz_before), A p = (6 p - S6(p)) + sum_o S_o p_o
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_apply(int64_t ns, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ cls, BdScreen q, int first,
                                                        int np, const double* __restrict__ rz, const double* __restrict__ rz_before,
                                                        const double* __restrict__ r, const double* __restrict__ dinv,
                                                        const double* __restrict__ p_old, double* __restrict__ p, double* __restrict__ ap,
                                                        double* __restrict__ part) {
    __shared__ double s_a[PN_WAVES], s_b[PN_WAVES], s_part[PN_WAVES], s_o[2], s_halo[PN_WAVES][BD_HALO];
    double beta = 0.0;
    if (!first) {
        const double n = wg_sum_partials_all(rz, np, s_a, s_o), d = wg_sum_partials_all(rz_before, np, s_b, s_o + 1);
        beta = d > 0.0 ? n / d : 0.0;
    }
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        const auto P = [&](int64_t k) { return r[k] * dinv[k] + beta * p_old[k]; };
        const double pv = P(at);
        const double S = bd_sum6(pv, nbr + 6 * s, lane, P);
        double av = 6.0 * pv - S;
        if (q.has[s]) av = av + bd_sc_term(q, s, lane, pv, s_halo[threadIdx.x >> 6], P);
        if (cls[at] != BD_FREE) av = 0.0;
        p[at] = pv;
        ap[at] = av;
        acc += pv * av;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// k_bd_update with the partials of the new r . (r dinv)
__global__ __launch_bounds__(PN_TPB) void k_bd_sc_update(int64_t ns, int np, const double* __restrict__ rz, const double* __restrict__ pap,
                                                         const double* __restrict__ p, const double* __restrict__ ap,
                                                         const double* __restrict__ dinv, double* __restrict__ x, double* __restrict__ r,
                                                         double* __restrict__ part) {
    __shared__ double s_a[PN_WAVES], s_b[PN_WAVES], s_part[PN_WAVES], s_o[2];
    const double n = wg_sum_partials_all(rz, np, s_a, s_o), d = wg_sum_partials_all(pap, np, s_b, s_o + 1);
    const double alpha = d > 0.0 ? n / d : 0.0;
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    BD_EACH_BLOCK(s) {
        const int64_t at = s * 64 + lane;
        x[at] = x[at] + alpha * p[at];
        const double rv = r[at] - alpha * ap[at];
        r[at] = rv;
        acc += rv * (rv * dinv[at]);
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ------------------------------------------------------------------ rule 29 ----
// The used rows in their order, by ordered compaction: the sum of rule 29 then runs over used[0 .. N), so a row that is not used moves
// no used row to another thread and the iso value, an fp64 sum in a fixed order, does not depend on such rows.
__global__ __launch_bounds__(PN_TPB) void k_bd_used_count(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const WgRank k = wg_rank<PN_WAVES>(i < n && pn_used(pts + 3 * i, nrm + 3 * i), s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}
__global__ __launch_bounds__(PN_TPB) void k_bd_used_scatter(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm,
                                                            const int32_t* __restrict__ base, int64_t* __restrict__ used) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const bool f = i < n && pn_used(pts + 3 * i, nrm + 3 * i);
    const int64_t pos = (int64_t)base[blockIdx.x] + wg_rank<PN_WAVES>(f, s_wsum).rank;
    if (f) used[pos] = i;
}

__global__ __launch_bounds__(PN_TPB) void k_bd_iso(int64_t m, const int64_t* __restrict__ used, const double* __restrict__ pts, PnGrid g, BdView v,
                                                   const double* __restrict__ chi, double* __restrict__ part) {
    __shared__ double s_part[PN_WAVES];
    double acc = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * PN_TPB + threadIdx.x; k < m; k += (int64_t)gridDim.x * PN_TPB) {
        const int64_t i = used[k];
        int i0[3];
        double w[8], val = 0.0;
        pn_corners_weights(pts + 3 * i, g, i0, w);
        for (int c = 0; c < 8; ++c) {
            const int64_t at = bd_slot(v, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
            val = val + w[c] * (at < 0 ? NAN : chi[at]);
        }
        acc += val;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ------------------------------------------------------------------ rules 30-31 ----
// Level D as poisson_surface.h's kernels see it: node and cube items are the places q = 4 * place of the row + lx of the stored nodes,
// in (iz, iy, ix) order
struct BdSurf {
    static constexpr bool counts_open = true;
    BdView v;
    PnGrid g;
    const int32_t *coord, *rows;          // per stored block; per place of bd_segment
    const double* chi;
    double iso;
    int64_t nodes;                        // 64 * stored blocks
    unsigned long long* n_open;           // rule 31's count
    __host__ __device__ int64_t node_items() const { return nodes; }
    __host__ __device__ int64_t cube_items() const { return nodes; }
    __device__ int64_t node(int64_t place, int i[3]) const {
        const int32_t ri = rows[place >> 2];
        const int s = ri >> 4, lx = (int)(place & 3), ly = ri & 3, lz = ri >> 2 & 3;
        int bx, by, bz;
        bd_unpack(coord[s], &bx, &by, &bz);
        i[0] = 4 * bx + lx; i[1] = 4 * by + ly; i[2] = 4 * bz + lz;
        return (int64_t)s * 64 + (lz << 4 | ly << 2 | lx);
    }
    __device__ void cube(int64_t place, int i[3]) const { node(place, i); }
    __device__ bool takes_part(const int i[3]) const { return i[0] < v.G && i[1] < v.G && i[2] < v.G && BdActive{v}(i[0], i[1], i[2]); }
    __device__ int64_t slot(int ix, int iy, int iz) const { return bd_slot(v, ix, iy, iz); }
    __device__ bool has(int64_t at) const { return at >= 0; }
    __device__ int64_t place(int ix, int iy, int iz) const {                // the node's block is stored
        const int by = iy >> 2, bz = iz >> 2;
        const int s = v.num[bd_tab(v, ix >> 2, by, bz)];
        const BdRowSlab q = bd_row_slab(v.first, v.T, by, bz);
        return bd_segment(s, iy & 3, iz & 3, q.rfirst, q.rcnt, q.sfirst, q.scnt) * 4 + (ix & 3);
    }
    __device__ bool edge(const int i[3], int type, bool* open) const {
        bool exists = false;
        *open = false;
        if (i[0] <= v.G && i[1] <= v.G && i[2] <= v.G) bd_edge_state(v.G, i[0], i[1], i[2], type, BdActive{v}, &exists, open);
        return exists;
    }
};

// ------------------------------------------------------------------ host ----
inline unsigned bd_grid(int64_t items) { return (unsigned)((items + PN_TPB - 1) / PN_TPB); }

int check_band(const char* fn, const mvs_poisson_band_params* bp, const void* binfo) {
    if (!bp || !binfo) return bad(fn, "bparams or binfo is NULL");
    if (bp->base_depth < 3 || bp->base_depth > MVS_POISSON_MAX_DEPTH) return bad(fn, "need base_depth in [3, MVS_POISSON_MAX_DEPTH]");
    if (bp->band < 1 || bp->band > 64) return bad(fn, "need band in [1, 64]");
    if (bp->reserved[0] != 0 || bp->reserved[1] != 0) return bad(fn, "bparams.reserved is not 0");
    return MVS_OK;
}

// one level of the band on the device
struct BdLevel {
    BdExtent e{};
    PnGrid g{};
    int64_t ns = 0, nodes = 0, held = 0;  // stored blocks, 64 * ns, bytes taken from the pool
    Scratch act, num, first, coord, nbr, cls, sums, b, x, ap;
    int64_t rows = 0;                     // rules 38-40: the nodes with a stencil row, and what the screened solve needs
    Scratch nb27, has, ridx, rnode, tab, dinv;
    BdScreen screen() const { return BdScreen{nb27.as<int32_t>(), has.as<uint8_t>(), ridx.as<int32_t>(), tab.as<double>()}; }
    BdView view() const { return BdView{e.G, e.T, e.Gb, act.as<uint8_t>(), num.as<int32_t>(), first.as<int32_t>()}; }
};

// what the test hook wants of one level, dense and in node order
struct BdDump {
    int level;
    uint8_t *active, *cls;
    double *b, *chi;
    int64_t node_capacity;
    int64_t* stencil = nullptr;           // mvs_test_poisson_band_screened_level only: [n1^3][27], f and the start values
    double *f = nullptr, *start = nullptr;
};

// One call past its checks, the points on the device.
struct BdRun {
    const char* fn;
    const mvs_poisson_params& p;
    const mvs_poisson_band_params& bp;
    mvs_poisson_info& info;
    mvs_poisson_band_info& binfo;
    int64_t n;
    const double *pts, *nrm;
    hipStream_t s;
    double origin[3] = {0.0, 0.0, 0.0}, side = 0.0, iso = 0.0;
    int D = 0, B = 0;
    BdBytes bytes;
    Scratch red, cnt8;                    // the partials of the reductions and their sum; one integer counter
    // rules 32-34 (mvs_poisson_reconstruct_band_density): absent for the band call
    const mvs_poisson_density_params* dp = nullptr;
    mvs_poisson_density_info* dinfo = nullptr;
    PnGrid gd{};
    int Dd = 0;
    BdExtent de{};                        // the block table of level Dd, when the sums live in blocks
    int64_t dns = 0, dslots = 0;          // stored blocks of the density grid; int64 sums held (64 dns, or every node of a dense grid)
    Scratch dnum, dcoord, dsum, rho, gain, dpart;
    // rules 36-41 (mvs_poisson_reconstruct_band_screened): absent for the other calls, and for alpha = 0
    const mvs_poisson_screen_params* sp = nullptr;
    mvs_poisson_screen_info* sinfo = nullptr;
    mvs_poisson_band_screen_info* bsinfo = nullptr;
    Scratch used;                         // the used rows in their order, kept over the levels
    std::vector<double> kept_b, kept_start;   // the hook's level: rule 28's b and the start values, before rules 39-40 change them
    std::unique_ptr<BdLevel> top;         // level D after levels()
    // the surface
    Scratch rows, mask, words;
    PnScan ve, fa;
    int64_t edge_items = 0, face_items = 0;

    BdRun(const BdCall& c, const double* pd, const double* nd, hipStream_t st)
        : fn(c.fn), p(*c.p), bp(*c.bp), info(*c.info), binfo(*c.binfo), n(c.n), pts(pd), nrm(nd), s(st), dp(c.dp), dinfo(c.dinfo) {
        std::memset(&info, 0, sizeof info);
        std::memset(&binfo, 0, sizeof binfo);
        if (dinfo) std::memset(dinfo, 0, sizeof *dinfo);
        if (c.screen) {
            std::memset(c.sinfo, 0, sizeof *c.sinfo);
            std::memset(c.bsinfo, 0, sizeof *c.bsinfo);
            if (c.sp->alpha > 0.0) { sp = c.sp; sinfo = c.sinfo; bsinfo = c.bsinfo; }
        }
    }
    bool weighted() const { return dp && (dp->flags & MVS_POISSON_WEIGHT_NORMALS); }
    PnDensitySums density_sums() const { return PnDensitySums{gd, bd_density_in_blocks(Dd, B) ? dnum.as<int32_t>() : nullptr, de.T, dsum.as<long long>()}; }

    int take(Scratch& sc, int64_t b, int64_t* held = nullptr) {
        const int rc = sc.alloc((size_t)b, s);
        if (rc) return rc;
        bytes.take(b);
        if (held) *held += b;
        return MVS_OK;
    }
    int fetch(void* dst, const void* src, size_t b) {
        HIPCHK(hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MVS_OK;
    }
    PnGrid grid_of(int l) const {
        PnGrid g{};
        for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
        g.G = 1 << l;
        g.h = side / (double)g.G;
        return g;
    }
    // the number behind the flags of a byte array, or the free nodes of a class array
    int count(const uint8_t* flag, int64_t m, bool free_nodes, int64_t* out) {
        HIPCHK(hipMemsetAsync(cnt8.p, 0, 8, s));
        if (free_nodes) k_bd_count_free<<<dim3(bd_grid(m)), dim3(PN_TPB), 0, s>>>(m, flag, cnt8.as<unsigned long long>());
        else k_bd_count_set<<<dim3(bd_grid(m)), dim3(PN_TPB), 0, s>>>(m, flag, cnt8.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        unsigned long long v = 0;
        const int rc = fetch(&v, cnt8.p, 8);
        *out = (int64_t)v;
        return rc;
    }

    // rules 1-2 and 24: the cube, N, D and B
    int depth() {
        int rc;
        mvs_poisson_info i0;
        const PnCall c{fn, PN_PLAIN, n, pts, nrm, &p, &i0, nullptr, nullptr, nullptr, nullptr};
        if ((rc = poisson_cube(c, pts, nrm, s, origin, &side))) return rc;
        info.n_used = i0.n_used;
        for (int a = 0; a < 3; ++a) info.origin[a] = origin[a];
        if ((rc = take(red, 8 * (1 + 4 * (int64_t)BD_NPART))) || (rc = take(cnt8, 8))) return rc;
        const int dmax = p.depth_max < BD_MAX_D ? p.depth_max : BD_MAX_D;
        D = p.depth_min;
        for (int d = p.depth_min + 1; d <= dmax; ++d) {                       // depth_min is the answer when nothing finer qualifies
            const PnGrid g = grid_of(d);
            const int64_t words = ((int64_t)1 << (3 * d)) / 32;
            Scratch bits;
            if ((rc = take(bits, 4 * words))) return rc;
            HIPCHK(hipMemsetAsync(bits.p, 0, (size_t)(4 * words), s));
            HIPCHK(hipMemsetAsync(cnt8.p, 0, 8, s));
            k_bd_occupy<<<dim3(bd_grid(n)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, bits.as<unsigned>());
            k_bd_popcount<<<dim3(bd_grid(words)), dim3(PN_TPB), 0, s>>>(words, bits.as<unsigned>(), cnt8.as<unsigned long long>());
            HIPCHK(hipGetLastError());
            unsigned long long occ = 0;
            if ((rc = fetch(&occ, cnt8.p, 8))) return rc;                     // synchronises: bits may go
            bytes.give(4 * words);
            if ((double)info.n_used >= p.samples_per_node * (double)occ) D = d;
        }
        B = D < bp.base_depth ? D : bp.base_depth;
        binfo.base_depth = B;
        return MVS_OK;
    }

    // rules 32-33 up to the gains: where the sums of the density grid live, rule 14 into it, rho_p, rho_mean and s_p
    int density() {
        int rc;
        gd = pn_density_grid(grid_of(D), side, D, dp->density_drop, &Dd);
        dinfo->density_depth = Dd;
        if (bd_density_in_blocks(Dd, B)) {                                   // the blocks a cell of a used point touches: rule 26's marks, not dilated
            de = bd_extent(Dd);
            const unsigned tgrid = bd_grid(de.table), rgrid = (unsigned)((de.rows + PN_WAVES - 1) / PN_WAVES);
            Scratch ta, tb, rcnt, first;
            if ((rc = take(ta, de.table)) || (rc = take(tb, de.table)) || (rc = take(rcnt, 4 * de.rows)) || (rc = take(first, 4 * (de.rows + 1))) ||
                (rc = dnum.alloc((size_t)(4 * de.table), s))) return rc;
            HIPCHK(hipMemsetAsync(ta.p, 0, (size_t)de.table, s));
            k_bd_mark<<<dim3(bd_grid(n)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, gd, de.T, ta.as<uint8_t>());
            k_bd_stored<<<dim3(tgrid), dim3(PN_TPB), 0, s>>>(de.T, ta.as<uint8_t>(), tb.as<uint8_t>());
            k_bd_row_count<<<dim3(rgrid), dim3(PN_TPB), 0, s>>>(de.T, tb.as<uint8_t>(), rcnt.as<int32_t>());
            HIPCHK(hipGetLastError());
            std::vector<int32_t> hc((size_t)de.rows), hf((size_t)de.rows + 1);
            if ((rc = fetch(hc.data(), rcnt.p, 4 * (size_t)de.rows))) return rc;
            dns = bd_row_firsts(de, hc.data(), hf.data());
            if (dns < 0) { mvs_set_error("%s: the row counts of the density grid are not counts", fn); return MVS_E_HIP; }
            if (!bd_fits_int32(dns)) {
                mvs_set_error("%s: the density grid of depth %d stores %lld blocks of 64 nodes: more than an int32 index reaches", fn, Dd, (long long)dns);
                return MVS_E_INVALID_ARG;
            }
            if ((rc = dcoord.alloc((size_t)(4 * dns), s))) return rc;
            HIPCHK(hipMemcpy(first.p, hf.data(), 4 * hf.size(), hipMemcpyHostToDevice));     // the stream is idle: fetch synchronised it
            k_bd_number<<<dim3(rgrid), dim3(PN_TPB), 0, s>>>(de.T, tb.as<uint8_t>(), first.as<int32_t>(), dnum.as<int32_t>(), dcoord.as<int32_t>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));                                  // ta, tb, rcnt and first go
            bytes.give(bd_density_work_bytes(Dd, B));
            dslots = dns * 64;
        } else
            dslots = (int64_t)(gd.G + 1) * (gd.G + 1) * (gd.G + 1);
        if ((rc = dsum.alloc((size_t)(8 * dslots), s)) || (rc = rho.alloc(8 * (size_t)n, s)) || (rc = gain.alloc(8 * (size_t)n, s)) ||
            (rc = dpart.alloc(24 * (size_t)BD_RED_NB, s))) return rc;
        bytes.take(bd_density_bytes(Dd, B, dns, n));
        HIPCHK(hipMemsetAsync(dsum.p, 0, (size_t)(8 * dslots), s));
        return poisson_density_rows(n, pts, nrm, density_sums(), info.n_used, dp->max_gain, rho.as<double>(), gain.as<double>(), dpart, dinfo, s);
    }

    // rule 34, after scatter
    int vertex_density(const double* vertices, double* out) {
        return out && info.n_vertices > 0 ? poisson_vertex_density(info.n_vertices, vertices, density_sums(), out, s) : MVS_OK;
    }

    // the hook's part of rules 32-33: the node sums expanded to the dense layout of the density grid, rho_p and s_p per row
    int dump_density(int64_t* node_sums, int64_t capacity, double* rho_out, double* gain_out) {
        const int n1 = gd.G + 1;
        const int64_t nn = (int64_t)n1 * n1 * n1;
        if (nn > capacity) return bad(fn, "density_node_capacity is below (2^density_depth + 1)^3 (dinfo holds the depth)");
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(rho_out, rho.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(gain_out, gain.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
        if (!bd_density_in_blocks(Dd, B)) {
            HIPCHK(hipMemcpy(node_sums, dsum.p, 8 * (size_t)nn, hipMemcpyDeviceToHost));
            return MVS_OK;
        }
        std::vector<long long> hs((size_t)dslots + 1);
        std::vector<int32_t> coord((size_t)dns + 1);
        HIPCHK(hipMemcpy(hs.data(), dsum.p, 8 * (size_t)dslots, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(coord.data(), dcoord.p, 4 * (size_t)dns, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < nn; ++i) node_sums[i] = 0;
        for (int64_t sb = 0; sb < dns; ++sb) {
            int bx, by, bz;
            bd_unpack(coord[(size_t)sb], &bx, &by, &bz);
            for (int lane = 0; lane < 64; ++lane) {
                const int ix = 4 * bx + (lane & 3), iy = 4 * by + (lane >> 2 & 3), iz = 4 * bz + (lane >> 4);
                if (ix <= gd.G && iy <= gd.G && iz <= gd.G) node_sums[((int64_t)iz * n1 + iy) * n1 + ix] = hs[(size_t)(sb * 64 + lane)];
            }
        }
        return MVS_OK;
    }

    // rule 26 and the numbering: the tables and the per-block arrays of level l
    int blocks(BdLevel& L, int l) {
        int rc;
        L.e = bd_extent(l);
        L.g = grid_of(l);
        const BdExtent& e = L.e;
        const unsigned tgrid = bd_grid(e.table), rgrid = (unsigned)((e.rows + PN_WAVES - 1) / PN_WAVES);
        Scratch ta, tb, rcnt;
        if ((rc = take(ta, e.table)) || (rc = take(tb, e.table)) || (rc = take(rcnt, 4 * e.rows)) || (rc = take(L.act, e.table, &L.held)) ||
            (rc = take(L.num, 4 * e.table, &L.held)) || (rc = take(L.first, 4 * (e.rows + 1), &L.held))) return rc;
        HIPCHK(hipMemsetAsync(ta.p, 0, (size_t)e.table, s));
        k_bd_mark<<<dim3(bd_grid(n)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, L.g, e.T, ta.as<uint8_t>());
        k_bd_dilate<<<dim3(tgrid), dim3(PN_TPB), 0, s>>>(e.T, e.Gb, ta.as<uint8_t>(), tb.as<uint8_t>(), 0, bp.band);
        k_bd_dilate<<<dim3(tgrid), dim3(PN_TPB), 0, s>>>(e.T, e.Gb, tb.as<uint8_t>(), ta.as<uint8_t>(), 1, bp.band);
        k_bd_dilate<<<dim3(tgrid), dim3(PN_TPB), 0, s>>>(e.T, e.Gb, ta.as<uint8_t>(), L.act.as<uint8_t>(), 2, bp.band);
        k_bd_stored<<<dim3(tgrid), dim3(PN_TPB), 0, s>>>(e.T, L.act.as<uint8_t>(), tb.as<uint8_t>());
        k_bd_row_count<<<dim3(rgrid), dim3(PN_TPB), 0, s>>>(e.T, tb.as<uint8_t>(), rcnt.as<int32_t>());
        HIPCHK(hipGetLastError());
        std::vector<int32_t> hc((size_t)e.rows), hf((size_t)e.rows + 1);
        if ((rc = fetch(hc.data(), rcnt.p, 4 * (size_t)e.rows))) return rc;
        L.ns = bd_row_firsts(e, hc.data(), hf.data());
        if (L.ns < 0) { mvs_set_error("%s: the row counts of level %d are not counts", fn, l); return MVS_E_HIP; }
        if ((rc = count(L.act.as<uint8_t>(), e.table, false, &binfo.n_active_blocks[l]))) return rc;
        if (!bd_fits_int32(L.ns)) {
            mvs_set_error("%s: level %d stores %lld blocks of 64 nodes: more than an int32 index reaches", fn, l, (long long)L.ns);
            return MVS_E_INVALID_ARG;
        }
        L.nodes = L.ns * 64;
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        const int64_t need = bd_level_bytes(e, L.ns, l == D) + (sp ? bd_screen_block_bytes(L.ns) + bd_screen_work_bytes(L.ns) : 0);
        if (need > (int64_t)total_b) {
            mvs_set_error("%s: level %d stores %lld blocks and needs %lld bytes: more than the device has", fn, l, (long long)L.ns, (long long)need);
            return MVS_E_OOM;
        }
        if ((rc = take(L.coord, 4 * L.ns, &L.held)) || (rc = take(L.nbr, 24 * L.ns, &L.held))) return rc;
        HIPCHK(hipMemcpy(L.first.p, hf.data(), 4 * hf.size(), hipMemcpyHostToDevice));       // the stream is idle: fetch synchronised it
        k_bd_number<<<dim3(rgrid), dim3(PN_TPB), 0, s>>>(e.T, tb.as<uint8_t>(), L.first.as<int32_t>(), L.num.as<int32_t>(), L.coord.as<int32_t>());
        if (L.ns > 0) k_bd_neighbours<<<dim3(bd_grid(6 * L.ns)), dim3(PN_TPB), 0, s>>>(L.ns, L.coord.as<int32_t>(), L.view(), L.nbr.as<int32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                                      // ta, tb and rcnt go
        bytes.give(2 * e.table + 4 * e.rows);
        return MVS_OK;
    }

    // rules 26-28 on level l; coarse: the level below
    template <class Coarse>
    int fill(BdLevel& L, int l, Coarse coarse) {
        int rc;
        if ((rc = take(L.cls, L.nodes, &L.held)) || (rc = take(L.sums, 24 * L.nodes, &L.held)) || (rc = take(L.b, 8 * L.nodes, &L.held)) ||
            (rc = take(L.x, 8 * L.nodes, &L.held)) || (rc = take(L.ap, 8 * L.nodes, &L.held))) return rc;
        if (L.ns == 0) return MVS_OK;
        const BdView v = L.view();
        const unsigned ngrid = bd_grid(L.nodes);
        k_bd_class_start<Coarse><<<dim3(ngrid), dim3(PN_TPB), 0, s>>>(L.ns, L.coord.as<int32_t>(), v, coarse, L.cls.as<uint8_t>(), L.x.as<double>());
        HIPCHK(hipMemsetAsync(L.sums.p, 0, (size_t)(24 * L.nodes), s));
        if (weighted()) k_bd_splat<true><<<dim3(bd_grid(n)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, L.g, v, L.nodes, L.sums.as<unsigned long long>(), gain.as<double>());
        else k_bd_splat<false><<<dim3(bd_grid(n)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, L.g, v, L.nodes, L.sums.as<unsigned long long>(), nullptr);
        k_bd_rhs<<<dim3(ngrid), dim3(PN_TPB), 0, s>>>(L.ns, L.nbr.as<int32_t>(), L.cls.as<uint8_t>(), L.nodes, L.sums.as<long long>(), L.g.h, L.b.as<double>());
        HIPCHK(hipGetLastError());
        return count(L.cls.as<uint8_t>(), L.nodes, true, &binfo.n_free[l]);
    }

    // occupied(l) of rule 38
    int occupied_at(int l, int64_t* out) {
        int rc;
        const PnGrid g = grid_of(l);
        const int64_t words = bd_occupancy_bytes(l) / 4;
        Scratch bits;
        if ((rc = take(bits, bd_occupancy_bytes(l)))) return rc;
        HIPCHK(hipMemsetAsync(bits.p, 0, (size_t)bd_occupancy_bytes(l), s));
        HIPCHK(hipMemsetAsync(cnt8.p, 0, 8, s));
        k_bd_occupy<<<dim3(bd_grid(n)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, bits.as<unsigned>());
        k_bd_popcount<<<dim3(bd_grid(words)), dim3(PN_TPB), 0, s>>>(words, bits.as<unsigned>(), cnt8.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        unsigned long long occ = 0;
        rc = fetch(&occ, cnt8.p, 8);                                          // synchronises: bits may go
        bytes.give(bd_occupancy_bytes(l));
        *out = (int64_t)occ;
        return rc;
    }

    // the used rows in their order (rule 29's list), once per call
    int used_list() {
        int rc;
        const int64_t m = info.n_used, nbu = (n + PN_TPB - 1) / PN_TPB;
        PnScan us;
        if ((rc = us.alloc((size_t)nbu, s)) || (rc = take(used, bd_used_bytes(m)))) return rc;
        if (us.bytes != bd_scan_bytes(n)) { mvs_set_error("%s: the scan over the points holds %lld bytes where the plan says %lld", fn, (long long)us.bytes, (long long)bd_scan_bytes(n)); return MVS_E_HIP; }
        bytes.take(bd_scan_bytes(n));
        k_bd_used_count<<<dim3((unsigned)nbu), dim3(PN_TPB), 0, s>>>(n, pts, nrm, us.cnt.as<int32_t>());
        us.run((int)nbu, s);
        k_bd_used_scatter<<<dim3((unsigned)nbu), dim3(PN_TPB), 0, s>>>(n, pts, nrm, us.base.as<int32_t>(), used.as<int64_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                                      // the scan may go
        bytes.give(bd_scan_bytes(n));
        return MVS_OK;
    }
    // rule 29's mean of x over the used points of the list
    int mean_at_points(const BdLevel& L, const double* x, double* out) {
        const int64_t m = info.n_used;
        const int nb = (int)std::min<int64_t>(BD_RED_NB, (m + PN_TPB - 1) / PN_TPB);
        double* part = red.as<double>() + 1;
        k_bd_iso<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(m, used.as<int64_t>(), pts, L.g, L.view(), x, part);
        double sum = 0.0;
        const int rc = folded(nb, part, &sum);
        *out = sum / (double)info.n_used;
        return rc;
    }

    // rules 38-40 on level l after fill(): occupied(l), lambda_l, the rows and their stencils, T_l on the start values, f in the place
    // of b.  d (may be NULL): the hook's level, which takes the int64 sums, f and the start values here.
    int screen_fill(BdLevel& L, int l, const BdDump* d) {
        int rc;
        if (L.ns == 0) return MVS_OK;
        if ((rc = occupied_at(l, &bsinfo->occupied[l]))) return rc;
        bsinfo->lambda[l] = pn_screen_lambda(sp->alpha, info.n_used, bsinfo->occupied[l]);
        const BdView v = L.view();
        const dim3 pgrid(bd_grid(n)), tb(PN_TPB);
        const int64_t nb = (L.nodes + PN_TPB - 1) / PN_TPB;
        {
            Scratch flag;
            PnScan sn;
            // the arrays one by one, the bytes by the plan (bd_screen_block_bytes, bd_screen_work_bytes): the plan's tests hold for what is asked for here
            if ((rc = L.nb27.alloc((size_t)(27 * 4 * L.ns), s)) || (rc = L.has.alloc((size_t)L.ns, s)) || (rc = L.ridx.alloc((size_t)(4 * L.nodes), s)) ||
                (rc = L.dinv.alloc((size_t)(8 * L.nodes), s)) || (rc = flag.alloc((size_t)L.nodes, s)) || (rc = sn.alloc((size_t)nb, s))) return rc;
            if (27 * 4 * L.ns + L.ns + 4 * L.nodes + 8 * L.nodes != bd_screen_block_bytes(L.ns) || L.nodes + sn.bytes != bd_screen_work_bytes(L.ns)) {
                mvs_set_error("%s: level %d: the arrays of the screened solve are not what the plan counts", fn, l);
                return MVS_E_HIP;
            }
            bytes.take(bd_screen_block_bytes(L.ns) + bd_screen_work_bytes(L.ns));
            L.held += bd_screen_block_bytes(L.ns);
            HIPCHK(hipMemsetAsync(flag.p, 0, (size_t)L.nodes, s));
            HIPCHK(hipMemsetAsync(L.has.p, 0, (size_t)L.ns, s));
            k_bd_nb27<<<dim3(bd_grid(27 * L.ns)), tb, 0, s>>>(L.ns, L.coord.as<int32_t>(), v, L.nb27.as<int32_t>());
            k_bd_sc_flag<<<pgrid, tb, 0, s>>>(n, pts, nrm, L.g, v, flag.as<uint8_t>(), L.has.as<uint8_t>());
            k_bd_sc_count<<<dim3((unsigned)nb), tb, 0, s>>>(L.nodes, flag.as<uint8_t>(), sn.cnt.as<int32_t>());
            sn.run((int)nb, s);
            HIPCHK(hipGetLastError());
            int32_t rows = 0;                                                 // base[nb]: all flagged places
            if ((rc = fetch(&rows, sn.base.as<int32_t>() + nb, 4))) return rc;
            L.rows = bsinfo->active_nodes[l] = rows;
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            if (bd_level_bytes(L.e, L.ns, l == D) + bd_screen_block_bytes(L.ns) + bd_screen_row_bytes(L.rows) > (int64_t)total_b) {
                mvs_set_error("%s: level %d has %lld stencil rows and needs %lld bytes for them: more than the device has", fn, l, (long long)L.rows,
                              (long long)bd_screen_row_bytes(L.rows));
                return MVS_E_OOM;
            }
            static_assert(BP_SC_ROW == PN_SC_ROW, "one row layout");
            if ((rc = L.tab.alloc((size_t)(8 * PN_SC_ROW * L.rows), s)) || (rc = L.rnode.alloc((size_t)(4 * L.rows), s))) return rc;
            bytes.take(bd_screen_row_bytes(L.rows));                          // 8 * BP_SC_ROW + 4 per row: the two arrays above
            L.held += bd_screen_row_bytes(L.rows);
            k_bd_sc_number<<<dim3((unsigned)nb), tb, 0, s>>>(L.nodes, flag.as<uint8_t>(), sn.base.as<int32_t>(), L.ridx.as<int32_t>(), L.rnode.as<int32_t>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));                                  // flag and the scan go
            bytes.give(bd_screen_work_bytes(L.ns));
        }
        HIPCHK(hipMemsetAsync(L.tab.p, 0, (size_t)(8 * PN_SC_ROW * L.rows), s));
        k_bd_sc_splat<<<pgrid, tb, 0, s>>>(n, pts, nrm, L.g, v, bsinfo->lambda[l], L.ridx.as<int32_t>(), L.tab.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        if (d && (rc = dump_stencil(L, *d))) return rc;
        poisson_screen_convert(L.rows, L.tab.as<long long>(), s);
        if (MVS_KNOB("MVS_BD_SC_JACOBI", 1, 0, 1) != 0.0)
            k_bd_sc_dinv<true><<<dim3(bd_grid(L.nodes)), tb, 0, s>>>(L.nodes, L.ridx.as<int32_t>(), L.tab.as<double>(), L.dinv.as<double>());
        else
            k_bd_sc_dinv<false><<<dim3(bd_grid(L.nodes)), tb, 0, s>>>(L.nodes, L.ridx.as<int32_t>(), L.tab.as<double>(), L.dinv.as<double>());
        HIPCHK(hipGetLastError());
        if ((rc = mean_at_points(L, L.x.as<double>(), &bsinfo->target[l]))) return rc;
        if (L.rows > 0) k_bd_sc_rhs<<<dim3(bd_grid(L.rows)), tb, 0, s>>>(L.rows, L.rnode.as<int32_t>(), L.cls.as<uint8_t>(), L.tab.as<double>(), bsinfo->target[l], L.b.as<double>());
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }

    // the hook's int64 sums of level l, dense [n1^3][27], before they become doubles
    int dump_stencil(const BdLevel& L, const BdDump& d) {
        const BdExtent& e = L.e;
        std::vector<long long> tab((size_t)(PN_SC_ROW * L.rows) + 1);
        std::vector<int32_t> rnode((size_t)L.rows + 1), coord((size_t)L.ns + 1);
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(tab.data(), L.tab.p, 8 * (size_t)(PN_SC_ROW * L.rows), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(rnode.data(), L.rnode.p, 4 * (size_t)L.rows, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(coord.data(), L.coord.p, 4 * (size_t)L.ns, hipMemcpyDeviceToHost));
        for (int64_t a = 0; a < L.rows; ++a) {
            const int64_t at = rnode[(size_t)a];
            const int lane = (int)(at & 63);
            int bx, by, bz;
            bd_unpack(coord[(size_t)(at >> 6)], &bx, &by, &bz);
            const int ix = 4 * bx + (lane & 3), iy = 4 * by + (lane >> 2 & 3), iz = 4 * bz + (lane >> 4);
            if (ix > e.G || iy > e.G || iz > e.G) continue;
            const int64_t node = ((int64_t)iz * e.n1 + iy) * e.n1 + ix;
            for (int k = 0; k < 27; ++k) d.stencil[27 * node + k] = tab[(size_t)(PN_SC_ROW * a + k)];
        }
        return MVS_OK;
    }

    int folded(int np, double* part, double* out) {
        poisson_fold(part, np, red.as<double>(), s);
        HIPCHK(hipGetLastError());
        return fetch(out, red.p, 8);
    }

    // rule 28: conjugate gradients from the start values until the true residual meets solve_tol
    int solve(BdLevel& L, int l) {
        int rc;
        if (L.ns == 0) return MVS_OK;
        const int np = (int)std::min<int64_t>((L.ns + PN_WAVES - 1) / PN_WAVES, BD_NPART);
        const dim3 gr((unsigned)np), tb(PN_TPB);
        double* part[4];                                                     // r . r twice (this iteration's and the one before), p . A p, the true residual
        for (int q = 0; q < 4; ++q) part[q] = red.as<double>() + 1 + q * BD_NPART;
        const int32_t* nbr = L.nbr.as<int32_t>();
        const uint8_t* cls = L.cls.as<uint8_t>();
        double *x = L.x.as<double>(), *b = L.b.as<double>(), *ap = L.ap.as<double>();
        double *r = L.sums.as<double>(), *pa = r + L.nodes, *pb = r + 2 * L.nodes;      // the sums are spent
        double b2 = 0.0, r2 = 0.0;
        const bool sc = sp != nullptr;                                        // rule 40: M_ff and f' in the place of A_ff and b'
        const BdScreen q = L.screen();
        const double* dinv = L.dinv.as<double>();
        k_bd_bnorm<<<gr, tb, 0, s>>>(L.ns, nbr, cls, x, b, part[3]);
        if ((rc = folded(np, part[3], &b2))) return rc;
        binfo.bnorm[l] = std::sqrt(b2);
        if (!(b2 > 0.0)) {                                                    // b' = 0 (or not finite): chi_f = 0
            k_bd_zero_free<<<dim3(bd_grid(L.nodes)), tb, 0, s>>>(L.nodes, cls, x);
            HIPCHK(hipGetLastError());
            return MVS_OK;
        }
        HIPCHK(hipMemsetAsync(L.sums.p, 0, (size_t)(24 * L.nodes), s));
        if (sc) k_bd_sc_residual<true><<<gr, tb, 0, s>>>(L.ns, nbr, cls, q, x, b, dinv, r, part[3], part[0]);
        else k_bd_residual<true><<<gr, tb, 0, s>>>(L.ns, nbr, cls, x, b, r, part[0]);
        if ((rc = folded(np, part[sc ? 3 : 0], &r2))) return rc;
        binfo.rel_residual[l] = std::sqrt(r2) / std::sqrt(b2);
        if (std::sqrt(r2) <= p.solve_tol * std::sqrt(b2)) return MVS_OK;
        int cur = 0, it = 0;
        for (int c = 1; c <= p.max_cycles; ++c) {
            for (int k = 0; k < 64; ++k, ++it) {
                if (sc) {
                    k_bd_sc_apply<<<gr, tb, 0, s>>>(L.ns, nbr, cls, q, it == 0 ? 1 : 0, np, part[cur], part[cur ^ 1], r, dinv, pa, pb, ap, part[2]);
                    k_bd_sc_update<<<gr, tb, 0, s>>>(L.ns, np, part[cur], part[2], pb, ap, dinv, x, r, part[cur ^ 1]);
                } else {
                    k_bd_apply<<<gr, tb, 0, s>>>(L.ns, nbr, cls, it == 0 ? 1 : 0, np, part[cur], part[cur ^ 1], r, pa, pb, ap, part[2]);
                    k_bd_update<<<gr, tb, 0, s>>>(L.ns, np, part[cur], part[2], pb, ap, x, r, part[cur ^ 1]);
                }
                cur ^= 1;
                std::swap(pa, pb);
            }
            if (sc) k_bd_sc_residual<false><<<gr, tb, 0, s>>>(L.ns, nbr, cls, q, x, b, nullptr, nullptr, part[3], nullptr);
            else k_bd_residual<false><<<gr, tb, 0, s>>>(L.ns, nbr, cls, x, b, nullptr, part[3]);
            if ((rc = folded(np, part[3], &r2))) return rc;
            binfo.iterations[l] = it;
            binfo.rel_residual[l] = std::sqrt(r2) / std::sqrt(b2);
            if (std::sqrt(r2) <= p.solve_tol * std::sqrt(b2)) return MVS_OK;
        }
        binfo.failed_level = l;
        mvs_set_error("%s: level %d: relative residual %.3e after %d iterations, above solve_tol %.3e", fn, l, binfo.rel_residual[l], it, p.solve_tol);
        return MVS_E_SOLVER;
    }

    // level l of the hook, dense: active [Gb^3], cls, b, chi [n1^3] in node order; NaN where a node has no value, b 0 at fixed nodes
    int dump(const BdLevel& L, const double* b_dev, const BdDump& d) {
        const BdExtent& e = L.e;
        const int64_t nn = (int64_t)e.n1 * e.n1 * e.n1;
        std::vector<uint8_t> act((size_t)e.table), cls((size_t)L.nodes + 1);
        std::vector<double> hb((size_t)L.nodes + 1), hx((size_t)L.nodes + 1);
        std::vector<int32_t> coord((size_t)L.ns + 1);
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(act.data(), L.act.p, (size_t)e.table, hipMemcpyDeviceToHost));
        if (L.ns > 0) {
            HIPCHK(hipMemcpy(cls.data(), L.cls.p, (size_t)L.nodes, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hb.data(), b_dev, 8 * (size_t)L.nodes, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hx.data(), L.x.p, 8 * (size_t)L.nodes, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(coord.data(), L.coord.p, 4 * (size_t)L.ns, hipMemcpyDeviceToHost));
        }
        for (int bz = 0; bz < e.Gb; ++bz)
            for (int by = 0; by < e.Gb; ++by)
                for (int bx = 0; bx < e.Gb; ++bx) d.active[((int64_t)bz * e.Gb + by) * e.Gb + bx] = act[(size_t)bd_table_at(e, bx, by, bz)];
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int64_t i = 0; i < nn; ++i) { d.cls[i] = BD_NONE; d.b[i] = nan; d.chi[i] = nan; }
        if (d.f) for (int64_t i = 0; i < nn; ++i) d.f[i] = d.start[i] = nan;
        for (int64_t sb = 0; sb < L.ns; ++sb) {
            int bx, by, bz;
            bd_unpack(coord[(size_t)sb], &bx, &by, &bz);
            for (int lane = 0; lane < 64; ++lane) {
                const int ix = 4 * bx + (lane & 3), iy = 4 * by + (lane >> 2 & 3), iz = 4 * bz + (lane >> 4);
                const size_t at = (size_t)(sb * 64 + lane);
                if (ix > e.G || iy > e.G || iz > e.G || cls[at] == BD_NONE) continue;
                const int64_t node = ((int64_t)iz * e.n1 + iy) * e.n1 + ix;
                d.cls[node] = cls[at];
                d.b[node] = cls[at] == BD_FREE ? hb[at] : 0.0;
                d.chi[node] = hx[at];
                if (d.f) {                                                   // b_dev holds f; rule 28's b and the start values were kept
                    d.f[node] = d.b[node];
                    d.b[node] = cls[at] == BD_FREE ? kept_b[at] : 0.0;
                    d.start[node] = kept_start[at];
                }
            }
        }
        return MVS_OK;
    }

    // rules 25-28: the base, then the levels B + 1 .. D; level D stays in `top`.  dump (may be NULL): the hook's level.
    int levels(const BdDump* d) {
        int rc;
        mvs_poisson_params pb = p;
        pb.depth_min = pb.depth_max = B;
        pb.max_cycles = (int32_t)std::min<int64_t>((int64_t)p.max_cycles * 64, INT32_MAX);   // rule 25: one budget for every solve of the call
        mvs_poisson_info ib;
        const PnCall cb{fn, PN_PLAIN, n, pts, nrm, &pb, &ib, nullptr, nullptr, sp, sinfo};    // sp: rule 37, the screened chi_B
        std::unique_ptr<PnBaseField> base(new PnBaseField);
        rc = base->solve(cb, pts, nrm, s, weighted() ? gain.as<double>() : nullptr);
        info.cycles = ib.cycles;
        info.rel_residual = ib.rel_residual;
        if (rc == MVS_E_SOLVER) binfo.failed_level = B;
        if (rc) return rc;
        bytes.take(base->bytes);
        if (sp && (rc = used_list())) return rc;
        std::unique_ptr<BdLevel> below;
        for (int l = B + 1; l <= D; ++l) {
            std::unique_ptr<BdLevel> L(new BdLevel);
            if ((rc = blocks(*L, l))) return rc;
            if (d && d->level == l && (int64_t)L->e.n1 * L->e.n1 * L->e.n1 > d->node_capacity)
                return bad(fn, "node_capacity is below (2^level + 1)^3");
            if (below) rc = fill(*L, l, BdBlockCoarse{below->view(), below->x.as<double>()});
            else rc = fill(*L, l, BdDenseCoarse{base->chi, 1 << B});
            if (rc) return rc;
            if (d && d->level == l && d->stencil) std::memset(d->stencil, 0, 27 * 8 * (size_t)L->e.n1 * L->e.n1 * L->e.n1);   // rows are written over it
            if (d && d->level == l && d->f && L->ns > 0) {
                kept_b.resize((size_t)L->nodes);
                kept_start.resize((size_t)L->nodes);
                HIPCHK(hipStreamSynchronize(s));
                HIPCHK(hipMemcpy(kept_b.data(), L->b.p, 8 * (size_t)L->nodes, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(kept_start.data(), L->x.p, 8 * (size_t)L->nodes, hipMemcpyDeviceToHost));
            }
            if (sp && (rc = screen_fill(*L, l, d && d->level == l && d->stencil ? d : nullptr))) return rc;
            HIPCHK(hipStreamSynchronize(s));                                  // the level below has been read: it goes back to the pool
            if (below) { bytes.give(below->held); below.reset(); }
            if (base) { bytes.give(base->bytes); base.reset(); }
            const int src = solve(*L, l);
            if (src && src != MVS_E_SOLVER) return src;
            if (d && d->level == l && (rc = dump(*L, L->b.as<double>(), *d))) return rc;   // the solve leaves b as it is
            if (src) return src;
            below = std::move(L);
        }
        top = std::move(below);
        return MVS_OK;
    }

    // rule 29
    int iso_value() {
        int rc;
        const BdLevel& L = *top;
        if (sp) {                                                             // rule 41: the list of the call
            rc = mean_at_points(L, L.x.as<double>(), &iso);
            info.iso = iso;
            return rc;
        }
        const int64_t m = info.n_used, nbu = (n + PN_TPB - 1) / PN_TPB;
        PnScan us;
        Scratch used;                                                         // of this stage only
        if ((rc = us.alloc((size_t)nbu, s)) || (rc = take(used, 8 * m))) return rc;
        bytes.take(us.bytes);
        k_bd_used_count<<<dim3((unsigned)nbu), dim3(PN_TPB), 0, s>>>(n, pts, nrm, us.cnt.as<int32_t>());
        us.run((int)nbu, s);
        k_bd_used_scatter<<<dim3((unsigned)nbu), dim3(PN_TPB), 0, s>>>(n, pts, nrm, us.base.as<int32_t>(), used.as<int64_t>());
        const int nb = (int)std::min<int64_t>(BD_RED_NB, (m + PN_TPB - 1) / PN_TPB);
        double* part = red.as<double>() + 1;
        k_bd_iso<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(m, used.as<int64_t>(), pts, L.g, L.view(), L.x.as<double>(), part);
        double sum = 0.0;
        rc = folded(nb, part, &sum);                                          // synchronises: used and the scan may go
        bytes.give(us.bytes + 8 * m);
        if (rc) return rc;
        info.iso = iso = sum / (double)info.n_used;
        return MVS_OK;
    }

    BdSurf surf() const {
        const BdLevel& L = *top;
        return BdSurf{L.view(), L.g, L.coord.as<int32_t>(), rows.as<int32_t>(), L.x.as<double>(), iso, L.nodes, cnt8.as<unsigned long long>()};
    }

    // rules 30-31 up to the counts
    int count_mesh() {
        int rc;
        BdLevel& L = *top;
        if (L.ns == 0) return MVS_OK;
        edge_items = 7 * L.nodes;
        face_items = 12 * L.nodes;
        const int64_t nbe = (edge_items + PN_TPB - 1) / PN_TPB, nbf = (face_items + PN_TPB - 1) / PN_TPB;
        if ((rc = take(rows, 64 * L.ns)) || (rc = take(mask, L.nodes)) || (rc = take(words, 8 * PN_WAVES * nbe)) || (rc = ve.alloc((size_t)nbe, s)) ||
            (rc = fa.alloc((size_t)nbf, s))) return rc;
        bytes.take(ve.bytes + fa.bytes);
        k_bd_rows<<<dim3(bd_grid(16 * L.ns)), dim3(PN_TPB), 0, s>>>(L.ns, L.coord.as<int32_t>(), L.view(), rows.as<int32_t>());
        const BdSurf q = surf();
        HIPCHK(hipMemsetAsync(cnt8.p, 0, 8, s));
        k_pn_cubemask<<<dim3(bd_grid(L.nodes)), dim3(PN_TPB), 0, s>>>(q, mask.as<uint8_t>());
        k_pn_edge_count<<<dim3((unsigned)nbe), dim3(PN_TPB), 0, s>>>(q, edge_items, words.as<unsigned long long>(), ve.cnt.as<int32_t>());
        ve.run((int)nbe, s);
        poisson_face_count(mask.as<uint8_t>(), face_items, fa.cnt.as<int32_t>(), s);
        fa.run((int)nbf, s);
        HIPCHK(hipGetLastError());
        int32_t nv = 0, nf = 0;
        unsigned long long nopen = 0;
        HIPCHK(hipMemcpyAsync(&nv, ve.base.as<int32_t>() + nbe, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&nopen, cnt8.p, 8, hipMemcpyDeviceToHost, s));
        if ((rc = fetch(&nf, fa.base.as<int32_t>() + nbf, 4))) return rc;
        info.n_vertices = nv;
        info.n_faces = nf;
        binfo.n_open_edges = (int64_t)nopen;
        return MVS_OK;
    }

    int scatter(double* vertices, int32_t* faces) {
        if (info.n_vertices == 0) return MVS_OK;
        const int64_t nbe = (edge_items + PN_TPB - 1) / PN_TPB, nbf = (face_items + PN_TPB - 1) / PN_TPB;
        const BdSurf q = surf();
        k_pn_vertex_scatter<<<dim3((unsigned)nbe), dim3(PN_TPB), 0, s>>>(q, edge_items, words.as<unsigned long long>(), ve.base.as<int32_t>(), vertices);
        k_pn_face_scatter<<<dim3((unsigned)nbf), dim3(PN_TPB), 0, s>>>(q, mask.as<uint8_t>(), face_items, words.as<unsigned long long>(), ve.base.as<int32_t>(),
                                                                      vertices, fa.base.as<int32_t>(), faces);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        return MVS_OK;
    }

    void finish_info() {
        info.depth = D;
        info.h = side / (double)(1 << D);
        binfo.scratch_bytes = bytes.peak;
    }
};

int check_band_call(const BdCall& c, const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b) {
    const PnCall pc{c.fn, PN_PLAIN, c.n, c.points, c.normals, c.p, c.info, nullptr, nullptr, nullptr, nullptr};
    int rc = poisson_check_plain(pc, BD_MAX_D, out_a, cap_a, out_b, cap_b);
    if (!rc) rc = check_band(c.fn, c.bp, c.binfo);
    if (!rc && c.density) rc = poisson_check_density(c.fn, c.n, c.dp, c.dinfo);
    if (!rc && c.screen) rc = poisson_check_screen(c.fn, c.sp, c.sinfo);
    if (!rc && c.screen && !c.bsinfo) rc = bad(c.fn, "bsinfo is NULL");
    return rc;
}

// the device form of the entry, after its checks
int band_reconstruct(const BdCall& c, const double* pts, const double* nrm, PnOut o, hipStream_t s) {
    int rc;
    BdRun run(c, pts, nrm, s);
    if ((rc = run.depth())) return rc;
    if (run.D <= run.B) {                                                     // rules 24, 32 and 36: the plain, the density or the screened call at depth D, its bytes
        mvs_poisson_params pd = *c.p;
        pd.depth_min = pd.depth_max = run.D;
        if (c.screen) return poisson_dense_dev(PnCall{c.fn, PN_SCREENED, c.n, pts, nrm, &pd, c.info, c.dp, c.dinfo, c.sp, c.sinfo}, pts, nrm, o, s);
        return poisson_dense_dev(PnCall{c.fn, c.density ? PN_DENSITY : PN_PLAIN, c.n, pts, nrm, &pd, c.info, c.dp, c.dinfo, nullptr, nullptr}, pts, nrm, o, s);
    }
    if (c.density && (rc = run.density())) { run.finish_info(); return rc; }
    rc = run.levels(nullptr);
    run.finish_info();
    if (rc || (rc = run.iso_value()) || (rc = run.count_mesh())) { run.finish_info(); return rc; }
    run.finish_info();
    return poisson_finish(c.fn, run, *c.info, o);
}

// the host form of the two entries: the points go up, the device form fills blocks, the blocks come down
int band_reconstruct_host(const BdCall& c, double* vertices, double* density, int64_t vcap, int32_t* faces, int64_t fcap) {
    Scratch dp, dn, dv, dd, df;
    int rc = check_band_call(c, vertices, vcap, faces, fcap);
    if (rc || (rc = need_device()) || (rc = up(dp, c.points, 3 * (size_t)c.n)) || (rc = up(dn, c.normals, 3 * (size_t)c.n)) ||
        (rc = band_reconstruct(c, dp.as<double>(), dn.as<double>(), PnOut{nullptr, nullptr, nullptr, vcap, fcap, &dv, density ? &dd : nullptr, &df}, nullptr)))
        return rc;
    const size_t V = (size_t)c.info->n_vertices, F = (size_t)c.info->n_faces;
    if ((density && (rc = down(density, dd, V))) || (rc = down(vertices, dv, 3 * V))) return rc;
    return down(faces, df, 3 * F);
}

// The two hooks after their checks: the call up to rule 29, level d.level handed out dense; with rules 32-33 (c.density) the density too.
// MVS_E_SOLVER of that level still hands out what it reached.
int band_level(const BdCall& c, const BdDump& d, int64_t* node_sums, int64_t density_node_capacity, double* rho, double* gain) {
    Scratch dp, dn;
    int rc;
    if ((rc = need_device()) || (rc = up(dp, c.points, 3 * (size_t)c.n)) || (rc = up(dn, c.normals, 3 * (size_t)c.n))) return rc;
    BdRun run(c, dp.as<double>(), dn.as<double>(), nullptr);
    if ((rc = run.depth())) return rc;
    run.finish_info();
    if (d.level <= run.B || d.level > run.D) return bad(c.fn, "level is outside base_depth + 1 .. depth (info and binfo hold them)");
    if (c.density) {
        rc = run.density();
        run.finish_info();
        if (rc || (rc = run.dump_density(node_sums, density_node_capacity, rho, gain))) return rc;
    }
    rc = run.levels(&d);
    run.finish_info();
    if (rc) return rc;
    rc = run.iso_value();
    run.finish_info();
    return rc;
}

}  // namespace

// the device form for a caller inside the library that cannot know the counts in advance (mvs_processor_poisson_band and
// mvs_processor_poisson_band_density); c.density: density receives d_v of rule 34 per vertex
int poisson_band_blocks(const BdCall& c, Scratch* vertices, Scratch* density, Scratch* faces) {
    const int rc = check_band_call(c, nullptr, 0, nullptr, 0);
    if (rc) return rc;
    return band_reconstruct(c, c.points, c.normals, PnOut{nullptr, nullptr, nullptr, INT64_MAX, INT64_MAX, vertices, c.density ? density : nullptr, faces}, nullptr);
}

extern "C" {

void mvs_poisson_band_default_params(mvs_poisson_band_params* p) {
    if (!p) return;
    p->base_depth = 8; p->band = 2; p->reserved[0] = p->reserved[1] = 0;
}

int mvs_poisson_reconstruct_band_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                     const mvs_poisson_band_params* bparams, mvs_poisson_info* info, mvs_poisson_band_info* binfo,
                                     double* vertices_dev, int64_t vertex_capacity, int32_t* faces_dev, int64_t face_capacity, void* hip_stream) {
    MVS_TRACE();
    const BdCall c{__func__, n, points_dev, normals_dev, p, bparams, info, binfo};
    int rc = check_band_call(c, vertices_dev, vertex_capacity, faces_dev, face_capacity);
    if (rc || (rc = need_device())) return rc;
    return band_reconstruct(c, points_dev, normals_dev, PnOut{vertices_dev, nullptr, faces_dev, vertex_capacity, face_capacity}, (hipStream_t)hip_stream);
}

int mvs_poisson_reconstruct_band(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                 const mvs_poisson_band_params* bparams, mvs_poisson_info* info, mvs_poisson_band_info* binfo, double* vertices,
                                 int64_t vertex_capacity, int32_t* faces, int64_t face_capacity) {
    MVS_TRACE();
    return band_reconstruct_host(BdCall{__func__, n, points, normals, p, bparams, info, binfo}, vertices, nullptr, vertex_capacity, faces, face_capacity);
}

// The call up to rule 29, level `level` handed out dense (include/mvs_test.h).  MVS_E_SOLVER of that level still hands out what it reached.
int mvs_test_poisson_band_level(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                const mvs_poisson_band_params* bparams, mvs_poisson_info* info, mvs_poisson_band_info* binfo, int32_t level,
                                uint8_t* active, uint8_t* cls, double* b, double* chi, int64_t node_capacity) {
    MVS_TRACE();
    const BdCall c{__func__, n, points, normals, p, bparams, info, binfo};
    const int rc = check_band_call(c, b, node_capacity, chi, node_capacity);
    if (rc) return rc;
    if (!active || !cls || !b || !chi) return bad(__func__, "active, cls, b or chi is NULL");
    return band_level(c, BdDump{level, active, cls, b, chi, node_capacity}, nullptr, 0, nullptr, nullptr);
}

// ------------------------------------------------------------------ rules 32-35 ----
int mvs_poisson_reconstruct_band_density_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                             const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                             mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo,
                                             double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                             int64_t face_capacity, void* hip_stream) {
    MVS_TRACE();
    const BdCall c{__func__, n, points_dev, normals_dev, p, bparams, info, binfo, dparams, dinfo, true};
    int rc = check_band_call(c, vertices_dev, vertex_capacity, faces_dev, face_capacity);
    if (rc || (rc = need_device())) return rc;
    return band_reconstruct(c, points_dev, normals_dev, PnOut{vertices_dev, vertex_density_dev, faces_dev, vertex_capacity, face_capacity}, (hipStream_t)hip_stream);
}

int mvs_poisson_reconstruct_band_density(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                         const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams, mvs_poisson_info* info,
                                         mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo, double* vertices, double* vertex_density,
                                         int64_t vertex_capacity, int32_t* faces, int64_t face_capacity) {
    MVS_TRACE();
    return band_reconstruct_host(BdCall{__func__, n, points, normals, p, bparams, info, binfo, dparams, dinfo, true}, vertices, vertex_density,
                                 vertex_capacity, faces, face_capacity);
}

// The call up to rule 29 with rules 32-33, level `level` and the density handed out dense (include/mvs_test.h)
int mvs_test_poisson_band_density_level(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                        const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams, mvs_poisson_info* info,
                                        mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo, int32_t level, uint8_t* active, uint8_t* cls,
                                        double* b, double* chi, int64_t node_capacity, int64_t* node_sums, int64_t density_node_capacity, double* rho,
                                        double* gain) {
    MVS_TRACE();
    const BdCall c{__func__, n, points, normals, p, bparams, info, binfo, dparams, dinfo, true};
    const int rc = check_band_call(c, b, node_capacity, node_sums, density_node_capacity);
    if (rc) return rc;
    if (!active || !cls || !b || !chi || !node_sums || !rho || !gain) return bad(__func__, "active, cls, b, chi, node_sums, rho or gain is NULL");
    return band_level(c, BdDump{level, active, cls, b, chi, node_capacity}, node_sums, density_node_capacity, rho, gain);
}

// ------------------------------------------------------------------ rules 36-41 ----
int mvs_poisson_reconstruct_band_screened_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                              const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                              mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo,
                                              double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                              int64_t face_capacity, void* hip_stream, const mvs_poisson_screen_params* sparams,
                                              mvs_poisson_screen_info* sinfo, mvs_poisson_band_screen_info* bsinfo) {
    MVS_TRACE();
    const BdCall c{__func__, n, points_dev, normals_dev, p, bparams, info, binfo, dparams, dinfo, true, sparams, sinfo, bsinfo, true};
    int rc = check_band_call(c, vertices_dev, vertex_capacity, faces_dev, face_capacity);
    if (rc || (rc = need_device())) return rc;
    return band_reconstruct(c, points_dev, normals_dev, PnOut{vertices_dev, vertex_density_dev, faces_dev, vertex_capacity, face_capacity}, (hipStream_t)hip_stream);
}

int mvs_poisson_reconstruct_band_screened(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                          const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams, mvs_poisson_info* info,
                                          mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo, double* vertices, double* vertex_density,
                                          int64_t vertex_capacity, int32_t* faces, int64_t face_capacity, const mvs_poisson_screen_params* sparams,
                                          mvs_poisson_screen_info* sinfo, mvs_poisson_band_screen_info* bsinfo) {
    MVS_TRACE();
    return band_reconstruct_host(BdCall{__func__, n, points, normals, p, bparams, info, binfo, dparams, dinfo, true, sparams, sinfo, bsinfo, true}, vertices,
                                 vertex_density, vertex_capacity, faces, face_capacity);
}

// The call up to rule 41's iso value, level `level` with its stencil sums, f and start values handed out dense (include/mvs_test.h)
int mvs_test_poisson_band_screened_level(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                         const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams, mvs_poisson_info* info,
                                         mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo, int32_t level, uint8_t* active, uint8_t* cls,
                                         double* b, double* chi, int64_t node_capacity, int64_t* node_sums, int64_t density_node_capacity, double* rho,
                                         double* gain, const mvs_poisson_screen_params* sparams, mvs_poisson_screen_info* sinfo,
                                         mvs_poisson_band_screen_info* bsinfo, int64_t* stencil, double* f, double* start) {
    MVS_TRACE();
    const BdCall c{__func__, n, points, normals, p, bparams, info, binfo, dparams, dinfo, true, sparams, sinfo, bsinfo, true};
    const int rc = check_band_call(c, b, node_capacity, node_sums, density_node_capacity);
    if (rc) return rc;
    if (!active || !cls || !b || !chi || !node_sums || !rho || !gain || !stencil || !f || !start)
        return bad(__func__, "active, cls, b, chi, node_sums, rho, gain, stencil, f or start is NULL");
    BdDump d{level, active, cls, b, chi, node_capacity};
    d.stencil = stencil; d.f = f; d.start = start;
    return band_level(c, d, node_sums, density_node_capacity, rho, gain);
}

}  // extern "C"
