// poisson.hip — mvs_poisson_reconstruct (include/mvs.h): oriented points to a triangle mesh, the step GeometryRec::RunPoisson takes
// between Result/PSR.npts and Result/Model.obj (R/Processor/Processor.cpp:1042-1058).  GeoRec is a closed binary: the rules are this
// library's definition, stated in include/mvs.h — an unscreened Poisson reconstruction on a dense grid; their per-point and
// per-tetrahedron part is poisson_rules.h, one body for these kernels and for host code.
//
//   k_pn_bbox          used rows, min and max per workgroup (order-free); the host finishes and derives cube, depth and grid (rules 1-4)
//   k_pn_occupy / k_pn_popcount
//                      rule 3 when depth_min < Dmax: one bitmap of cells per candidate depth, atomicOr, then a popcount
//   k_pn_splat         rule 5: a thread per point, 24 int64 atomic adds into the three planar sum arrays
//   k_pn_rhs           rule 6: a thread per node
//   k_mg_smooth<Op> / k_mg_residual<Op> / k_mg_restrict / k_mg_prolong
//                      rule 8, levels above 33^3: V(2,2) cycles, Jacobi damped by 6/7, full weighting (x 4: the stencil is unscaled),
//                      trilinear prolongation.  Smoother and residual march along z with the column's three values in registers.
//                      Op: the operator, MgPlain here (S - 6 x) or MgScreened<diagonal> for the second solve of the screened call
//   k_mg_coarse<Op>    the levels of 33^3 and below, down to the single interior node of level 1 and back, in ONE workgroup
//   k_mg_residual<Op> (out == NULL) / k_pn_fold
//                      the true residual's squared norm: partials per workgroup, folded by one workgroup in a fixed order
//   k_pn_iso           rule 9, the same two-step reduction
//   k_pn_cubemask<S> / k_pn_edge_count<S> / k_pn_vertex_scatter<S> / k_pn_face_scatter<S> (poisson_surface.h), k_pn_face_count
//                      rules 10-12 over a surface view, here PnDenseSurf: the cube masks and two ordered compactions, described there.
//                      k_pn_scan_rows / _totals / _add (PnScan) scan the millions of counts in two levels.
// mvs_poisson_reconstruct_density adds the sampling density (rules 14-17; the trim of rule 18 is mesh_trim.hip):
//   k_pn_density_splat<Sums> rule 14: a thread per point, 8 int64 atomic adds into the node sums of the coarser density grid
//   k_pn_point_density<Sums> rule 15: rho_p per row; min, max and the int64 sum of the quantised densities per workgroup (order-free)
//   k_pn_gain          rule 16: s_p per row and the rows cut at max_gain; k_pn_splat<true> is the splat of the scaled normals
//   k_pn_vertex_density<Sums> rule 17, over the vertex list the scatter wrote
//                      Sums: how the node sums are stored, BdDenseSums here; the band levels (poisson_band.hip) run the same three
//                      kernels over BdBlockSums too, through poisson_density_rows and poisson_vertex_density
// mvs_poisson_reconstruct_screened adds the second, screened solve (rules 19-23): the k_sc_* kernels build the stencil rows and the right
// side, described where they stand; the solve is the multigrid above with MgScreened, its smoother on the launched levels
// k_mg_smooth<MgPlain> followed by k_sc_smooth_rows over the rows.
// The reductions fold through wg_fold of poisson_dev.h (shuffles, then the waves in order).  Nothing but the integer atomics of the splats and the bitmap
// is unordered: two runs give the same bytes (tests/test_gpu_poisson_bits.py holds a build to recorded ones).
// The host side: PnCall (stitch.h) is the record of a call, whichever entry made it; PnRun its state on the device; reconstruct the device
// form of every entry and reconstruct_host the host form; the test hooks of include/mvs_test.h drive PnRun step by step.  What
// poisson_band.hip shares — the scan, the fold, the face count, the density of rules 14-17, the tail of a call — is declared in poisson_base.h.
#include "engine.h"
#include "trace.h"
#include "frontend_dev.h"
#include "poisson_dev.h"
#include "poisson_surface.h"
#include "knobs.h"
#include "stitch.h"
#include "poisson_base.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int PN_RED_NB = 1024;          // workgroups of a reduction over the points
constexpr int PN_ZC = 16;                // planes a thread of the smoother marches through
constexpr int PN_COARSE = 5;             // levels up to this one (33^3 nodes) run inside k_mg_coarse
constexpr int PN_COARSE_TPB = 1024;
constexpr int PN_MAX_D = MVS_POISSON_MAX_DEPTH;

// ------------------------------------------------------------------ rules 1-3 ----
__global__ __launch_bounds__(PN_TPB) void k_pn_bbox(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, double* __restrict__ part) {
    __shared__ double s_red[7][PN_WAVES];
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL}, cnt = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_TPB) {
        if (!pn_used(pts + 3 * i, nrm + 3 * i)) continue;
        cnt += 1.0;
        for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], pts[3 * i + a]); hi[a] = fmax(hi[a], pts[3 * i + a]); }
    }
    for (int a = 0; a < 3; ++a) {
        lo[a] = wg_fold<PN_WAVES>(lo[a], HUGE_VAL, s_red[a], threadIdx.x, FoldMin());
        hi[a] = wg_fold<PN_WAVES>(hi[a], -HUGE_VAL, s_red[3 + a], threadIdx.x, FoldMax());
    }
    cnt = wg_fold<PN_WAVES>(cnt, 0.0, s_red[6], threadIdx.x, FoldAdd());     // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) { part[7 * blockIdx.x + a] = lo[a]; part[7 * blockIdx.x + 3 + a] = hi[a]; }
        part[7 * blockIdx.x + 6] = cnt;
    }
}

struct PnOcc {                           // the candidate depths dmin .. dmax of rule 3: cell size and the first bitmap word of each
    int32_t dmin, dmax;
    double o[3], cs[PN_MAX_D + 1];
    int64_t word0[PN_MAX_D + 2];
};

__global__ __launch_bounds__(PN_TPB) void k_pn_occupy(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnOcc q,
                                                      unsigned* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    for (int d = q.dmin; d <= q.dmax; ++d) {
        const int m = 1 << d;
        const int64_t cell = ((int64_t)pn_cell(pts[3 * i + 2], q.o[2], q.cs[d], m) * m + pn_cell(pts[3 * i + 1], q.o[1], q.cs[d], m)) * m +
                             pn_cell(pts[3 * i], q.o[0], q.cs[d], m);
        atomicOr(bits + q.word0[d] + (cell >> 5), 1u << (cell & 31));
    }
}

__global__ __launch_bounds__(PN_TPB) void k_pn_popcount(PnOcc q, const unsigned* __restrict__ bits, unsigned long long* __restrict__ occupied) {
    const int64_t w = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (w >= q.word0[q.dmax + 1]) return;
    const unsigned v = bits[w];
    if (!v) return;
    int d = q.dmin;
    while (w >= q.word0[d + 1]) ++d;
    atomicAdd(occupied + d, (unsigned long long)__popc(v));
}

// ------------------------------------------------------------------ rules 5-6 ----
// WEIGHTED: rule 16, every normal scaled by the gain s_p of its point
template <bool WEIGHTED>
__global__ __launch_bounds__(PN_TPB) void k_pn_splat(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g,
                                                     unsigned long long* __restrict__ sums, const double* __restrict__ gain) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    const int64_t nn = (int64_t)(g.G + 1) * (g.G + 1) * (g.G + 1);
    int i0[3];
    double w[8], na[3];
    pn_corners_weights(pts + 3 * i, g, i0, w);
    for (int a = 0; a < 3; ++a) na[a] = WEIGHTED ? nrm[3 * i + a] * gain[i] : nrm[3 * i + a];
    for (int c = 0; c < 8; ++c) {
        const int64_t node = pn_corner_node(g.G, i0, c);
        for (int a = 0; a < 3; ++a) atomicAdd(sums + a * nn + node, (unsigned long long)pn_quant(w[c] * na[a]));
    }
}

// ------------------------------------------------------------------ rules 14-17 ----
// The node sums of the density grid are read and written through Sums, BdDenseSums (node order) or BdBlockSums (the stored blocks of a
// band level, rule 32; a node without storage reads as 0) of poisson_band_rules.h: the dense call instantiates the first only.
// rule 14: a thread per point, 8 int64 atomic adds into the node sums of the density grid
template <class Sums>
__global__ __launch_bounds__(PN_TPB) void k_pn_density_splat(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid gd, Sums d,
                                                             unsigned long long* __restrict__ dsum) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int i0[3];
    double w[8];
    pn_corners_weights(pts + 3 * i, gd, i0, w);
    for (int c = 0; c < 8; ++c) {
        const int64_t at = d.slot(i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
        if (!Sums::dense && at < 0) continue;                                // rule 32: cannot be, the block of the point's cell is marked
        atomicAdd(dsum + at, (unsigned long long)pn_quant(w[c]));
    }
}

// rule 15: rho_p of every row (0 for a row that is not used) and, per workgroup, the min, the max and the int64 sum of the quantised
// densities of its used rows — all three order-free; the host finishes.  part_d[2 b] = min, [2 b + 1] = max, part_q[b] = the sum.
template <class Sums>
__global__ __launch_bounds__(PN_TPB) void k_pn_point_density(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid gd, Sums d,
                                                             double* __restrict__ rho, double* __restrict__ part_d, long long* __restrict__ part_q) {
    __shared__ double s_lo[PN_WAVES], s_hi[PN_WAVES];
    __shared__ long long s_q[PN_WAVES];
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    long long q = 0;
    for (int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_TPB) {
        double r = 0.0;
        if (pn_used(pts + 3 * i, nrm + 3 * i)) {
            r = bd_density_at(pts + 3 * i, gd, d);
            lo = fmin(lo, r);
            hi = fmax(hi, r);
            q += pn_rho_quant(r);
        }
        rho[i] = r;
    }
    lo = wg_fold<PN_WAVES>(lo, HUGE_VAL, s_lo, threadIdx.x, FoldMin());
    hi = wg_fold<PN_WAVES>(hi, -HUGE_VAL, s_hi, threadIdx.x, FoldMax());
    q = wg_fold<PN_WAVES>(q, 0ll, s_q, threadIdx.x, FoldAdd());
    if (threadIdx.x == 0) {
        part_d[2 * blockIdx.x] = lo;
        part_d[2 * blockIdx.x + 1] = hi;
        part_q[blockIdx.x] = q;
    }
}

// rule 16: s_p of every row (0 for a row that is not used) and, per workgroup, the used rows whose gain was cut at max_gain
__global__ __launch_bounds__(PN_TPB) void k_pn_gain(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm,
                                                    const double* __restrict__ rho, double rho_mean, double max_gain, double* __restrict__ gain,
                                                    int32_t* __restrict__ part_c) {
    __shared__ int s_c[PN_WAVES];
    int cut = 0;
    for (int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_TPB) {
        double s = 0.0;
        if (pn_used(pts + 3 * i, nrm + 3 * i)) {
            s = pn_gain(rho_mean, rho[i], max_gain);
            cut += rho_mean / rho[i] > max_gain ? 1 : 0;
        }
        gain[i] = s;
    }
    cut = wg_fold<PN_WAVES>(cut, 0, s_c, threadIdx.x, FoldAdd());
    if (threadIdx.x == 0) part_c[blockIdx.x] = cut;
}

// rule 17: over the vertex list the scatter wrote
template <class Sums>
__global__ __launch_bounds__(PN_TPB) void k_pn_vertex_density(int64_t nv, const double* __restrict__ vertices, PnGrid gd, Sums d, double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (v >= nv) return;
    const double* p = vertices + 3 * v;
    out[v] = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) ? bd_density_at(p, gd, d) : NAN;      // a cell needs a finite position
}

__global__ __launch_bounds__(PN_TPB) void k_pn_rhs(PnGrid g, const long long* __restrict__ sums, double* __restrict__ b) {
    const int n1 = g.G + 1;
    const int64_t nn = (int64_t)n1 * n1 * n1, at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x, plane = (int64_t)n1 * n1;
    if (at >= nn) return;
    const int ix = (int)(at % n1), iy = (int)(at / n1 % n1), iz = (int)(at / plane);
    double v = 0.0;
    if (ix > 0 && ix < g.G && iy > 0 && iy < g.G && iz > 0 && iz < g.G) {
        const long long *sx = sums, *sy = sums + nn, *sz = sums + 2 * nn;
        v = (((pn_dequant(sx[at + 1]) - pn_dequant(sx[at - 1])) + (pn_dequant(sy[at + n1]) - pn_dequant(sy[at - n1]))) +
             (pn_dequant(sz[at + plane]) - pn_dequant(sz[at - plane]))) * (0.5 * g.h);
    }
    b[at] = v;
}

// ------------------------------------------------------------------ rules 8 and 22 ----
// One multigrid for the two operators, MgPlain (rule 8) and MgScreened (rule 22).  One node of a level of G cells (interior nodes only;
// the boundary holds 0 in every array), S the six neighbours of x:
//   smooth    MgPlain: y = (x + S - b) / 7, Jacobi damped by 6/7 for S - 6 x = b; MgScreened: y = x - r w, w = (6/7) / diagonal
//   residual  r = b - (S - 6 x), for MgScreened less the stencil term of a node that has a row
__device__ inline double pn_nbr_sum(const double* x, int64_t at, int n1, int64_t plane) {
    return ((x[at - 1] + x[at + 1]) + (x[at - n1] + x[at + n1])) + (x[at - plane] + x[at + plane]);
}
// full weighting of the fine residual r (level of 2 Gc cells) at coarse node (ix, iy, iz), times 4
__device__ inline double pn_restrict_at(const double* r, int Gc, int ix, int iy, int iz) {
    const int n1 = 2 * Gc + 1;
    const int64_t plane = (int64_t)n1 * n1, at = ((int64_t)(2 * iz) * n1 + 2 * iy) * n1 + 2 * ix;
    double acc = 0.0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const double w = (dz ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0);
                acc += w * r[at + dz * plane + dy * n1 + dx];
            }
    return 0.5 * acc;
}
// the trilinear interpolant of the coarse correction e (level of G / 2 cells) at fine node (ix, iy, iz)
__device__ inline double pn_prolong_at(const double* e, int G, int ix, int iy, int iz) {
    const int m1 = G / 2 + 1;
    double acc = 0.0;
    for (int c = 0; c < 8; ++c) {
        const int jx = (ix + (c & 1)) >> 1, jy = (iy + (c >> 1 & 1)) >> 1, jz = (iz + (c >> 2 & 1)) >> 1;
        acc += e[((int64_t)jz * m1 + jy) * m1 + jx];
    }
    return 0.125 * acc;
}

// the launches of the large levels: x fastest, 64 x 4 columns per workgroup, every thread marches through PN_ZC planes
__device__ inline bool pn_column(int G, int* ix, int* iy, int* z0, int* z1) {
    *ix = 1 + blockIdx.x * 64 + threadIdx.x;
    *iy = 1 + blockIdx.y * 4 + threadIdx.y;
    *z0 = 1 + blockIdx.z * PN_ZC;
    *z1 = *z0 + PN_ZC < G ? *z0 + PN_ZC : G;
    return *ix < G && *iy < G;
}
dim3 pn_column_grid(int G) { return dim3((unsigned)((G - 1 + 63) / 64), (unsigned)((G - 1 + 3) / 4), (unsigned)((G - 1 + PN_ZC - 1) / PN_ZC)); }

// The stencil rows of the screened operator (rules 19-22, below): a level keeps the number of every node's row (idx, -1: the node has
// none) and the rows, SC_ROW doubles each: the 27 entries in the offset order of rule 20, then the row sum.
constexpr int SC_ROW = 28;
// the smoother of the launched levels of M: 0 the fused kernel k_mg_smooth<MgScreened>, 1 k_mg_smooth<MgPlain> and then k_sc_smooth_rows
// over the rows.  A compile-time constant in the product build; the diagnostics build reads MVS_SC_SMOOTH_BY_ROWS once (scripts/bench_poisson_screened.py)
#define SC_SMOOTH_BY_ROWS (MVS_KNOB("MVS_SC_SMOOTH_BY_ROWS", 1, 0, 1) != 0.0)
constexpr int SC_DIAG_HALF_ROW_SUM = 0, SC_DIAG_PLAIN = 1, SC_DIAG_ROW_SUM = 2;    // the Jacobi diagonal 6 + rs / 2 (kept), 6 + S_{i,0}, 6 + rs
struct ScLevels { const int32_t* idx[PN_MAX_D + 1]; const double* tab[PN_MAX_D + 1]; };

// sum_o S_{i,o} x_{i+o} of an interior node with a row
__device__ inline double sc_apply(const double* __restrict__ x, int64_t at, int n1, int64_t plane, const double* __restrict__ row) {
    double acc = 0.0;
    int k = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) acc = acc + row[k++] * x[at + dz * plane + dy * n1 + dx];
    return acc;
}
// one interior node of M x = b, c = x[at] and S6 the sum of its six neighbours: the residual, and the Jacobi weight (6/7) / diagonal
__device__ inline double sc_residual_at(const double* __restrict__ x, int64_t at, int n1, int64_t plane, double c, double S6, double b,
                                        const double* __restrict__ row) {
    double m = S6 - 6.0 * c;
    if (row) m = m - sc_apply(x, at, n1, plane, row);
    return b - m;
}
template <int DIAG>
__device__ inline double sc_weight(const double* __restrict__ row) {
    if (!row) return 1.0 / 7.0;
    return (6.0 / 7.0) / (6.0 + (DIAG == SC_DIAG_PLAIN ? row[13] : DIAG == SC_DIAG_ROW_SUM ? row[27] : 0.5 * row[27]));
}
__device__ inline const double* sc_row(const int32_t* __restrict__ idx, const double* __restrict__ tab, int64_t at) {
    const int a = idx[at];
    return a < 0 ? nullptr : tab + (int64_t)SC_ROW * a;
}

// The operator of a level, the parameter of the multigrid kernels and of the solver on the host.  Of one interior node `at` of the
// system Op x = b, c = x[at] and S the sum of its six neighbours: relax, the damped Jacobi step; residual; solve1, the level of one
// unknown.  A kernel builds its Op from its trailing arguments — none for MgPlain, so those instantiations take and load nothing more.
// The two relax steps round differently at a node without a row: each operator keeps its own.
struct MgPlain {                         // A x = S - 6 x
    static constexpr bool screened = false;
    __device__ static MgPlain level(int) { return {}; }
    __device__ double relax(const double*, int64_t, int, int64_t, double c, double S, double b) const { return ((c + S) - b) * (1.0 / 7.0); }
    __device__ double residual(const double*, int64_t, int, int64_t, double c, double S, double b) const { return b - (S - 6.0 * c); }
    __device__ double solve1(int64_t, double b) const { return b / -6.0; }
    template <class F> static void level_args(const ScLevels&, int, F f) { f(); }
    template <class F> static void all_args(const ScLevels&, F f) { f(); }
};
template <int DIAG>
struct MgScreened {                      // M x = A x - sum_o S_{i,o} x_{i+o} at the nodes that have a row (rules 19-22, below); DIAG: the Jacobi diagonal
    static constexpr bool screened = true;
    static constexpr int diag = DIAG;
    const int32_t* idx;                  // of this level
    const double* tab;
    __device__ static MgScreened level(int l, const ScLevels& Sc) { return {Sc.idx[l], Sc.tab[l]}; }
    __device__ double relax(const double* __restrict__ x, int64_t at, int n1, int64_t plane, double c, double S, double b) const {
        const double* row = sc_row(idx, tab, at);
        return c - sc_residual_at(x, at, n1, plane, c, S, b, row) * sc_weight<DIAG>(row);
    }
    __device__ double residual(const double* __restrict__ x, int64_t at, int n1, int64_t plane, double c, double S, double b) const {
        return sc_residual_at(x, at, n1, plane, c, S, b, sc_row(idx, tab, at));
    }
    __device__ double solve1(int64_t at, double b) const {                   // its neighbours are boundary nodes
        const double* row = sc_row(idx, tab, at);
        return b / -(6.0 + (row ? row[13] : 0.0));
    }
    template <class F> static void level_args(const ScLevels& Sc, int l, F f) { f(Sc.idx[l], Sc.tab[l]); }
    template <class F> static void all_args(const ScLevels& Sc, F f) { f(Sc); }
};
// the diagonal chosen at run time as the template argument: f(MgScreened<diag>()), the value only names the type
template <class F>
int with_diagonal(int diag, F f) {
    if (diag == SC_DIAG_PLAIN) return f(MgScreened<SC_DIAG_PLAIN>());
    if (diag == SC_DIAG_ROW_SUM) return f(MgScreened<SC_DIAG_ROW_SUM>());
    return f(MgScreened<SC_DIAG_HALF_ROW_SUM>());
}

template <class Op, class... A>
__global__ __launch_bounds__(PN_TPB) void k_mg_smooth(int G, const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ y, A... a) {
    const Op op{a...};
    int ix, iy, z0, z1;
    if (!pn_column(G, &ix, &iy, &z0, &z1)) return;
    const int n1 = G + 1;
    const int64_t plane = (int64_t)n1 * n1;
    int64_t at = pn_node(G, ix, iy, z0);
    double lo = x[at - plane], c = x[at];
    for (int iz = z0; iz < z1; ++iz, at += plane) {
        const double hi = x[at + plane];
        const double S = ((x[at - 1] + x[at + 1]) + (x[at - n1] + x[at + n1])) + (lo + hi);
        y[at] = op.relax(x, at, n1, plane, c, S, b[at]);
        lo = c;
        c = hi;
    }
}

// r = b - Op x; with out == NULL only the squared norm: one partial per workgroup, part[(z * gridDim.y + y) * gridDim.x + x]
template <class Op, class... A>
__global__ __launch_bounds__(PN_TPB) void k_mg_residual(int G, const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ out,
                                                        double* __restrict__ part, A... a) {
    __shared__ double s_part[PN_WAVES];
    const Op op{a...};
    int ix, iy, z0, z1;
    double acc = 0.0;
    if (pn_column(G, &ix, &iy, &z0, &z1)) {
        const int n1 = G + 1;
        const int64_t plane = (int64_t)n1 * n1;
        int64_t at = pn_node(G, ix, iy, z0);
        double lo = x[at - plane], c = x[at];
        for (int iz = z0; iz < z1; ++iz, at += plane) {
            const double hi = x[at + plane];
            const double S = ((x[at - 1] + x[at + 1]) + (x[at - n1] + x[at + n1])) + (lo + hi);
            const double r = op.residual(x, at, n1, plane, c, S, b[at]);
            if (out) out[at] = r;
            acc += r * r;
            lo = c;
            c = hi;
        }
    }
    if (!part) return;
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.y * 64 + threadIdx.x);
    if (threadIdx.x == 0 && threadIdx.y == 0) part[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// the sum of n partials by ONE workgroup, in the order of wg_sum_partials
__global__ __launch_bounds__(PN_TPB) void k_pn_fold(const double* __restrict__ part, int n, double* __restrict__ out) {
    __shared__ double s_part[PN_WAVES];
    const double t = wg_sum_partials(part, n, s_part);
    if (threadIdx.x == 0) *out = t;
}

__global__ __launch_bounds__(PN_TPB) void k_mg_restrict(int Gc, const double* __restrict__ r, double* __restrict__ bc) {
    const int ix = 1 + blockIdx.x * 64 + threadIdx.x, iy = 1 + blockIdx.y * 4 + threadIdx.y, iz = 1 + blockIdx.z;
    if (ix >= Gc || iy >= Gc || iz >= Gc) return;
    bc[pn_node(Gc, ix, iy, iz)] = pn_restrict_at(r, Gc, ix, iy, iz);
}

__global__ __launch_bounds__(PN_TPB) void k_mg_prolong(int G, const double* __restrict__ e, double* __restrict__ x) {
    const int ix = 1 + blockIdx.x * 64 + threadIdx.x, iy = 1 + blockIdx.y * 4 + threadIdx.y, iz = 1 + blockIdx.z;
    if (ix >= G || iy >= G || iz >= G) return;
    x[pn_node(G, ix, iy, iz)] += pn_prolong_at(e, G, ix, iy, iz);
}

struct PnLevels { double *x[PN_MAX_D + 1], *t[PN_MAX_D + 1], *b[PN_MAX_D + 1]; };     // level l has 2^l cells; t: second buffer of the smoother, residual

// f(at, ix, iy, iz) for every interior node of a level of G cells, the workgroup's threads striding over them
template <class F>
__device__ inline void pn_each_interior(int G, F f) {
    const int m = G - 1, tot = m * m * m;
    for (int q = threadIdx.x; q < tot; q += blockDim.x) {
        const int ix = 1 + q % m, iy = 1 + q / m % m, iz = 1 + q / (m * m);
        f(pn_node(G, ix, iy, iz), ix, iy, iz);
    }
    __syncthreads();                                                        // the level's arrays are global memory of this one workgroup
}

// two sweeps of the smoother inside the one workgroup: x -> t -> x
template <class Op>
__device__ inline void mg_coarse_smooth2(const Op& op, int G, double* x, double* t, const double* b) {
    const int n1 = G + 1;
    const int64_t plane = (int64_t)n1 * n1;
    pn_each_interior(G, [&](int64_t at, int, int, int) { t[at] = op.relax(x, at, n1, plane, x[at], pn_nbr_sum(x, at, n1, plane), b[at]); });
    pn_each_interior(G, [&](int64_t at, int, int, int) { x[at] = op.relax(t, at, n1, plane, t[at], pn_nbr_sum(t, at, n1, plane), b[at]); });
}

// One V(2,2) cycle over the levels top .. 1 (top <= PN_COARSE) by ONE workgroup.  x[top] is the iterate to improve; the levels
// below start from zero.  a: nothing, or the ScLevels of the screened operator.
template <class Op, class... A>
__global__ __launch_bounds__(PN_COARSE_TPB) void k_mg_coarse(PnLevels L, int top, A... a) {
    for (int l = top; l >= 2; --l) {
        const int G = 1 << l, n1 = G + 1;
        const int64_t plane = (int64_t)n1 * n1;
        double *x = L.x[l], *t = L.t[l], *bc = L.b[l - 1], *xc = L.x[l - 1];
        const double* b = L.b[l];
        const Op op = Op::level(l, a...);
        mg_coarse_smooth2(op, G, x, t, b);
        pn_each_interior(G, [&](int64_t at, int, int, int) { t[at] = op.residual(x, at, n1, plane, x[at], pn_nbr_sum(x, at, n1, plane), b[at]); });
        pn_each_interior(G / 2, [&](int64_t at, int ix, int iy, int iz) { bc[at] = pn_restrict_at(t, G / 2, ix, iy, iz); xc[at] = 0.0; });
    }
    if (threadIdx.x == 0) {                                                 // level 1: one unknown
        const int64_t at = pn_node(2, 1, 1, 1);
        L.x[1][at] = Op::level(1, a...).solve1(at, L.b[1][at]);
    }
    __syncthreads();
    for (int l = 2; l <= top; ++l) {
        const int G = 1 << l;
        double* x = L.x[l];
        const double* e = L.x[l - 1];
        pn_each_interior(G, [&](int64_t at, int ix, int iy, int iz) { x[at] += pn_prolong_at(e, G, ix, iy, iz); });
        mg_coarse_smooth2(Op::level(l, a...), G, x, L.t[l], L.b[l]);
    }
}

// ------------------------------------------------------------------ rules 19-21 ----
// The stencils of MgScreened and the right side of rule 21.  The screened operator of level l is M_l = A_l - S_l with S_l = 1/2 P^T S_(l+1) P, P the trilinear prolongation: pn_restrict_at is HALF
// the transposed prolongation, and under it the Laplacian reproduces itself.  (The trilinear bases nest, so S_l is also the stencil of
// rule 20 splatted with the weights of level l and lambda * 2^-(D - l).)  A level keeps the number of every node's stencil row (idx, -1: the node has none) and the rows of the
// nodes that a point touches, SC_ROW doubles each: the 27 entries in the offset order of rule 20, then the row sum.
//   k_sc_flag / k_sc_count / k_sc_number   plain byte stores of 1, then the ordered compaction of the edges and faces: no atomic counter
//   k_sc_splat / k_sc_convert              rule 20 on the finest level: 64 int64 atomic adds per point; the sums become doubles in place
//   k_sc_flag_coarse / k_sc_coarsen        the rows of a level below the finest, gathered from the level above
//   k_sc_rhs                               rule 21: f = b - T rs
//   k_sc_smooth_rows                       the smoother of the launched levels is k_mg_smooth<MgPlain>, then this pass over the rows
//                                          (measured against the fused k_mg_smooth<MgScreened>, which the diagnostics build can still select)
//   the solve                              the multigrid kernels above with MgScreened, the stencil term at the nodes that have a row:
//                                          Jacobi damped by 6/7 over the diagonal d = 6 + rs / 2.  Every entry of S is >= 0, so the
//                                          absolute row sum of M is at most 12 + rs, and the eigenvalues of the iteration's
//                                          (7/6 d)^-1 M lie below (12 + rs) / (7 + 7/12 rs) < 2: it converges.  6 + rs converges too
//                                          but smooths the S part half as fast; the plain diagonal 6 + S_{i,0} can diverge where the
//                                          points are dense (S is then lambda rho times a mass matrix, whose Jacobi spectrum reaches
//                                          27/8).  The diagonal is a template parameter: the public call instantiates this one only,
//                                          mvs_test_poisson_screened the other two for the measurement behind the choice.
__global__ __launch_bounds__(PN_TPB) void k_sc_flag(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g,
                                                    uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int i0[3];
    double w[8];
    pn_corners_weights(pts + 3 * i, g, i0, w);
    for (int c = 0; c < 8; ++c) flag[pn_corner_node(g.G, i0, c)] = 1;
}

__global__ __launch_bounds__(PN_TPB) void k_sc_count(int64_t nn, const uint8_t* __restrict__ flag, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const WgRank k = wg_rank<PN_WAVES>(at < nn && flag[at], s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

// idx[node] = the number of the node's row or -1; node_of[row] = its node
__global__ __launch_bounds__(PN_TPB) void k_sc_number(int64_t nn, const uint8_t* __restrict__ flag, const int32_t* __restrict__ base,
                                                      int32_t* __restrict__ idx, int32_t* __restrict__ node_of) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const bool f = at < nn && flag[at];
    const int pos = base[blockIdx.x] + wg_rank<PN_WAVES>(f, s_wsum).rank;
    if (at < nn) idx[at] = f ? pos : -1;
    if (f) node_of[pos] = (int32_t)at;
}

__global__ __launch_bounds__(PN_TPB) void k_sc_splat(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g, double lambda,
                                                     const int32_t* __restrict__ idx, unsigned long long* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n || !pn_used(pts + 3 * i, nrm + 3 * i)) return;
    int i0[3];
    double w[8];
    int64_t row[8];
    pn_corners_weights(pts + 3 * i, g, i0, w);
    for (int c = 0; c < 8; ++c) row[c] = (int64_t)SC_ROW * idx[pn_corner_node(g.G, i0, c)];   // flagged: >= 0
    for (int c1 = 0; c1 < 8; ++c1)
        for (int c2 = c1; c2 < 8; ++c2) {
            int o12, o21;
            const unsigned long long q = (unsigned long long)pn_screen_pair(lambda, w, c1, c2, &o12, &o21);
            atomicAdd(tab + row[c1] + o12, q);
            if (c1 != c2) atomicAdd(tab + row[c2] + o21, q);
        }
}

// The levels below the finest take their rows from the level above, T_c = 1/2 P^T T_f P, gathered: a coarse node has a row when one of
// the 27 fine nodes around its own fine node has one (the same nodes the points touch on the coarse level), and a thread per coarse
// row adds, in a fixed order, the products it is made of.  Per axis the trilinear weight of fine offset e from a coarse node is
// 1 - |e| / 2 for |e| <= 1.  No atomics: a splat of 2 M points into the few rows of a coarse level would queue on them.
__global__ __launch_bounds__(PN_TPB) void k_sc_flag_coarse(int Gc, const int32_t* __restrict__ idx_f, uint8_t* __restrict__ flag) {
    const int n1 = Gc + 1, m1 = 2 * Gc + 1;
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= (int64_t)n1 * n1 * n1) return;
    const int ix = (int)(at % n1), iy = (int)(at / n1 % n1), iz = (int)(at / ((int64_t)n1 * n1));
    bool any = false;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int fx = 2 * ix + dx, fy = 2 * iy + dy, fz = 2 * iz + dz;
                if (fx < 0 || fx >= m1 || fy < 0 || fy >= m1 || fz < 0 || fz >= m1) continue;
                any = any || idx_f[((int64_t)fz * m1 + fy) * m1 + fx] >= 0;
            }
    flag[at] = any ? 1 : 0;
}

__device__ inline double sc_hat(int e) { return e == 0 ? 1.0 : e == 1 || e == -1 ? 0.5 : 0.0; }

__global__ __launch_bounds__(PN_TPB) void k_sc_coarsen(int64_t rows, const int32_t* __restrict__ node_c, int Gc, const int32_t* __restrict__ idx_f,
                                                       const double* __restrict__ tab_f, double* __restrict__ tab_c) {
    const int64_t a = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (a >= rows) return;
    const int n1 = Gc + 1, m1 = 2 * Gc + 1;
    const int64_t at = node_c[a];
    const int ix = (int)(at % n1), iy = (int)(at / n1 % n1), iz = (int)(at / ((int64_t)n1 * n1));
    double* out = tab_c + SC_ROW * a;
    double acc[27];
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {                                // the fine node 2 I + d and its weight in the coarse basis of I
                const int fx = 2 * ix + dx, fy = 2 * iy + dy, fz = 2 * iz + dz;
                if (fx < 0 || fx >= m1 || fy < 0 || fy >= m1 || fz < 0 || fz >= m1) continue;
                const int fa = idx_f[((int64_t)fz * m1 + fy) * m1 + fx];
                if (fa < 0) continue;
                const double* row = tab_f + (int64_t)SC_ROW * fa;
                const double wd = (sc_hat(dx) * sc_hat(dy)) * sc_hat(dz);
                for (int oz = -1; oz <= 1; ++oz)
                    for (int oy = -1; oy <= 1; ++oy)
                        for (int ox = -1; ox <= 1; ++ox) {                    // its entry o lands on the coarse nodes I + O with |d + o - 2 O| <= 1
                            const double v = wd * row[pn_screen_offset(ox, oy, oz)];
                            if (v == 0.0) continue;
                            for (int Oz = -1; Oz <= 1; ++Oz) {
                                const double wz = sc_hat(dz + oz - 2 * Oz);
                                if (wz == 0.0) continue;
                                for (int Oy = -1; Oy <= 1; ++Oy) {
                                    const double wy = sc_hat(dy + oy - 2 * Oy);
                                    if (wy == 0.0) continue;
                                    for (int Ox = -1; Ox <= 1; ++Ox) {
                                        const double wx = sc_hat(dx + ox - 2 * Ox);
                                        if (wx != 0.0) acc[pn_screen_offset(Ox, Oy, Oz)] += v * ((wx * wy) * wz);
                                    }
                                }
                            }
                        }
            }
    double rs = 0.0;
    for (int k = 0; k < 27; ++k) { out[k] = 0.5 * acc[k]; rs += 0.5 * acc[k]; }
    out[27] = rs;
}

// the hook's dense copy of the finest level's sums, before k_sc_convert: out[node][27]
__global__ __launch_bounds__(PN_TPB) void k_sc_dense(int64_t nn, const int32_t* __restrict__ idx, const long long* __restrict__ tab,
                                                     long long* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (e >= 27 * nn) return;
    const int a = idx[e / 27];
    out[e] = a < 0 ? 0 : tab[(int64_t)SC_ROW * a + e % 27];
}

// a thread per row: the 27 int64 sums and their int64 sum become doubles in place (the bits of a double stored as the int64 they were)
__global__ __launch_bounds__(PN_TPB) void k_sc_convert(int64_t rows, long long* __restrict__ tab) {
    const int64_t a = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (a >= rows) return;
    long long* row = tab + SC_ROW * a;
    long long rs = 0;
    for (int k = 0; k < 27; ++k) {
        const long long v = row[k];
        rs += v;
        row[k] = __double_as_longlong(pn_screen_dequant(v));
    }
    row[27] = __double_as_longlong(pn_screen_dequant(rs));
}

__global__ __launch_bounds__(PN_TPB) void k_sc_rhs(int64_t nn, const int32_t* __restrict__ idx, const double* __restrict__ tab, double T,
                                                   double* __restrict__ b) {
    const int64_t at = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (at >= nn) return;
    const int a = idx[at];
    if (a >= 0) b[at] = b[at] - T * tab[(int64_t)SC_ROW * a + 27];
}

// The chosen form of the smoother of M: k_mg_smooth<MgPlain> writes every node of y as if S were zero, then this pass, a thread per row, writes the
// nodes that have a row again, from the same old iterate x.  node_of[row] = the row's node; a row at a boundary node is skipped.
template <int DIAG>
__global__ __launch_bounds__(PN_TPB) void k_sc_smooth_rows(int64_t rows, const int32_t* __restrict__ node_of, int G, const double* __restrict__ x,
                                                           const double* __restrict__ b, double* __restrict__ y, const double* __restrict__ tab) {
    const int64_t a = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (a >= rows) return;
    const int n1 = G + 1;
    const int64_t plane = (int64_t)n1 * n1, at = node_of[a];
    const int ix = (int)(at % n1), iy = (int)(at / n1 % n1), iz = (int)(at / plane);
    if (ix < 1 || ix >= G || iy < 1 || iy >= G || iz < 1 || iz >= G) return;
    const double* row = tab + SC_ROW * a;
    const double c = x[at];
    y[at] = c - sc_residual_at(x, at, n1, plane, c, pn_nbr_sum(x, at, n1, plane), b[at], row) * sc_weight<DIAG>(row);
}

// ------------------------------------------------------------------ rule 9 ----
__global__ __launch_bounds__(PN_TPB) void k_pn_iso(int64_t n, const double* __restrict__ pts, const double* __restrict__ nrm, PnGrid g,
                                                   const double* __restrict__ chi, double* __restrict__ part) {
    __shared__ double s_part[PN_WAVES];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_TPB) {
        if (!pn_used(pts + 3 * i, nrm + 3 * i)) continue;
        int i0[3];
        double w[8], v = 0.0;
        pn_corners_weights(pts + 3 * i, g, i0, w);
        for (int c = 0; c < 8; ++c) v = v + w[c] * chi[pn_corner_node(g.G, i0, c)];
        acc += v;
    }
    const double t = wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ------------------------------------------------------------------ rules 10-12 ----
// The kernels are poisson_surface.h's over PnDenseSurf; what stays here serves the band levels too (PnScan, poisson_face_count).
// The scan between a count and a scatter kernel, in two levels: the compactions here have millions of workgroups, too many for the one
// workgroup of compact.hip's tail.  A workgroup scans PN_SCAN_CH counts into its own row of `local` (CH + 1 entries, the last one the
// row's total), one workgroup scans the totals, and the third launch adds the two: base[b] = survivors in the workgroups before b,
// base[nb] = all survivors.
constexpr int PN_SCAN_CH = 4096;
__global__ __launch_bounds__(PN_TPB) void k_pn_scan_rows(const int32_t* __restrict__ cnt, int nb, int32_t* __restrict__ local, int32_t* __restrict__ tot) {
    const int c0 = blockIdx.x * PN_SCAN_CH, len = nb - c0 < PN_SCAN_CH ? nb - c0 : PN_SCAN_CH;
    int32_t* row = local + (int64_t)blockIdx.x * (PN_SCAN_CH + 1);
    wg_scan_counts<PN_WAVES>(cnt + c0, len, row);
    if (threadIdx.x == 0) tot[blockIdx.x] = row[len];                        // written by this thread
}
__global__ __launch_bounds__(PN_TPB) void k_pn_scan_totals(const int32_t* __restrict__ tot, int rows, int32_t* __restrict__ rbase) {
    wg_scan_counts<PN_WAVES>(tot, rows, rbase);
}
__global__ __launch_bounds__(PN_TPB) void k_pn_scan_add(const int32_t* __restrict__ local, const int32_t* __restrict__ rbase, int nb, int rows,
                                                        int32_t* __restrict__ base) {
    const int64_t i = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (i < nb) base[i] = local[(i / PN_SCAN_CH) * (PN_SCAN_CH + 1) + i % PN_SCAN_CH] + rbase[i / PN_SCAN_CH];
    if (i == nb) base[nb] = rbase[rows];
}

__global__ __launch_bounds__(PN_TPB) void k_pn_face_count(const uint8_t* __restrict__ mask, int64_t items, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t r = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const WgRank k = wg_rank<PN_WAVES>(pn_face_item(mask, r, items) >= 0, s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

// ------------------------------------------------------------------ host ----
int check_pn(const char* fn, int64_t n, const void* points, const void* normals, const mvs_poisson_params* p, const void* info,
             const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b, int max_depth = PN_MAX_D) {
    if (!points || !normals || !p || !info) return bad(fn, "points, normals, params or info is NULL");
    if (n < 0) return bad(fn, "n is negative");
    if (cap_a < 0 || cap_b < 0) return bad(fn, "a capacity is negative");
    if ((cap_a > 0 && !out_a) || (cap_b > 0 && !out_b)) return bad(fn, "an output with a capacity above 0 is NULL");
    if (!std::isfinite(p->scale) || !std::isfinite(p->samples_per_node) || !std::isfinite(p->solve_tol)) return bad(fn, "a parameter is not finite");
    if (p->scale <= 0.0 || p->samples_per_node <= 0.0 || p->solve_tol <= 0.0) return bad(fn, "need scale, samples_per_node, solve_tol > 0");
    if (p->depth_min < 3) return bad(fn, "need depth_min >= 3");
    if (p->depth_min > p->depth_max) return bad(fn, "depth_min exceeds depth_max");
    if (p->depth_min > max_depth) return bad(fn, max_depth == PN_MAX_D ? "depth_min exceeds MVS_POISSON_MAX_DEPTH" : "depth_min exceeds the call's largest depth");
    if (p->scale <= 1.0 + 4.0 / (double)(1 << p->depth_min)) return bad(fn, "need scale > 1 + 4 / 2^depth_min: every point a cell from the boundary");
    if (p->max_cycles < 1) return bad(fn, "need max_cycles >= 1");
    return MVS_OK;
}

int check_pn_density(const char* fn, int64_t n, const mvs_poisson_density_params* dp, const void* dinfo) {
    if (!dp || !dinfo) return bad(fn, "dparams or dinfo is NULL");
    if (!std::isfinite(dp->max_gain) || dp->max_gain < 1.0 || dp->max_gain > 16.0) return bad(fn, "need max_gain in [1, 16]");
    if (dp->density_drop < 0 || dp->density_drop > 8) return bad(fn, "need density_drop in [0, 8]");
    if (dp->flags & ~MVS_POISSON_WEIGHT_NORMALS) return bad(fn, "flags holds a bit other than MVS_POISSON_WEIGHT_NORMALS");
    if ((dp->flags & MVS_POISSON_WEIGHT_NORMALS) && n > (1ll << 22)) return bad(fn, "more than 2^22 points with MVS_POISSON_WEIGHT_NORMALS");
    return MVS_OK;
}

int check_pn_screen(const char* fn, const mvs_poisson_screen_params* sp, const void* sinfo) {
    if (!sp || !sinfo) return bad(fn, "sparams or sinfo is NULL");
    if (!std::isfinite(sp->alpha) || sp->alpha < 0.0 || sp->alpha > 64.0) return bad(fn, "need alpha in [0, 64]");
    if (sp->reserved != 0) return bad(fn, "sparams.reserved is not 0");
    return MVS_OK;
}

// the arguments of a call and two of its outputs with their capacities (an entry names its own pair), before need_device
int check_call(const PnCall& c, const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b) {
    int rc = check_pn(c.fn, c.n, c.points, c.normals, c.p, c.info, out_a, cap_a, out_b, cap_b);
    if (!rc && c.rules >= PN_DENSITY) rc = check_pn_density(c.fn, c.n, c.dp, c.dinfo);
    if (!rc && c.rules >= PN_SCREENED) rc = check_pn_screen(c.fn, c.sp, c.sinfo);
    return rc;
}

// One call: the grid, the field and the counts; the scatter once the caller's capacities are known to suffice.
struct PnRun {
    const mvs_poisson_params& p;
    mvs_poisson_info& info;
    int64_t n;
    const double *pts, *nrm;              // on the device
    hipStream_t s;
    PnGrid g{};
    int64_t nn = 0;                       // nodes of the finest level
    double side = 0.0;                    // rule 2
    Scratch part, sums, rhs, coarse, red, mask, words;
    // rules 14-17 (mvs_poisson_reconstruct_density): absent for the plain call
    const mvs_poisson_density_params* dp = nullptr;
    mvs_poisson_density_info* dinfo = nullptr;
    PnGrid gd{};
    int64_t nnd = 0;                      // nodes of the density grid
    Scratch dsum, rho, gain, dpart;
    const double* row_gain = nullptr;     // s_p per row from outside (PnBaseField::solve for the band levels): rule 16's splat without dp
    PnScan ve, fa;
    // rules 19-23 (mvs_poisson_reconstruct_screened): absent for the other calls
    const mvs_poisson_screen_params* sp = nullptr;
    mvs_poisson_screen_info* sinfo = nullptr;
    int diag = SC_DIAG_HALF_ROW_SUM;      // another one through mvs_test_poisson_screened only
    Scratch sc_flag, sc_idx[PN_MAX_D + 1], sc_tab[PN_MAX_D + 1], sc_node[PN_MAX_D + 1];   // sc_node[l][row] = the row's node
    ScLevels Sc{};
    int64_t sc_rows[PN_MAX_D + 1] = {};   // nodes with a stencil row, per level
    PnScan sn;
    PnLevels L{};
    double iso = 0.0;
    int64_t edge_items = 0, face_items = 0;
    // a checked call and its points on the device; every info struct of the call starts from zero
    PnRun(const PnCall& c, const double* pd, const double* nd, hipStream_t st)
        : p(*c.p), info(*c.info), n(c.n), pts(pd), nrm(nd), s(st), dp(c.dp), dinfo(c.dinfo), sp(c.sp), sinfo(c.sinfo) {
        std::memset(&info, 0, sizeof info);
        if (dinfo) std::memset(dinfo, 0, sizeof *dinfo);
        if (sinfo) std::memset(sinfo, 0, sizeof *sinfo);
    }

    int fetch(void* dst, const void* src, size_t bytes) {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MVS_OK;
    }

    // hocc[d] = the occupied cells of the cube (side and g.o of rule 2) at every depth d = dmin .. dmax: rule 3, and occupied(D) of rule 19
    int occupancy(int dmin, int dmax, unsigned long long hocc[PN_MAX_D + 1]) {
        int rc;
        PnOcc q{};
        q.dmin = dmin; q.dmax = dmax;
        int64_t w = 0;
        for (int d = dmin; d <= dmax; ++d) { q.cs[d] = side / (double)(1 << d); q.word0[d] = w; w += ((int64_t)1 << (3 * d)) / 32; }
        q.word0[dmax + 1] = w;
        for (int a = 0; a < 3; ++a) q.o[a] = g.o[a];
        Scratch bits, occ;
        const size_t occ_bytes = sizeof(unsigned long long) * (PN_MAX_D + 1);
        if ((rc = bits.alloc(sizeof(unsigned) * (size_t)w, s)) || (rc = occ.alloc(occ_bytes, s))) return rc;
        HIPCHK(hipMemsetAsync(bits.p, 0, sizeof(unsigned) * (size_t)w, s));
        HIPCHK(hipMemsetAsync(occ.p, 0, occ_bytes, s));
        k_pn_occupy<<<dim3((unsigned)((n + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, q, bits.as<unsigned>());
        k_pn_popcount<<<dim3((unsigned)((w + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(q, bits.as<unsigned>(), occ.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        return fetch(hocc, occ.p, occ_bytes);
    }

    // rules 1-4
    int grid(const char* fn) {
        int rc;
        if (n < 2) { mvs_set_error("%s: fewer than 2 points", fn); return MVS_E_DEGENERATE; }
        const int nb = (int)std::min<int64_t>(PN_RED_NB, (n + PN_TPB - 1) / PN_TPB);
        if ((rc = part.alloc(sizeof(double) * 7 * PN_RED_NB, s))) return rc;
        k_pn_bbox<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(n, pts, nrm, part.as<double>());
        HIPCHK(hipGetLastError());
        std::vector<double> hp((size_t)7 * nb);
        if ((rc = fetch(hp.data(), part.p, sizeof(double) * hp.size()))) return rc;
        double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL}, cnt = 0.0;
        for (int b = 0; b < nb; ++b) {
            for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], hp[7 * b + a]); hi[a] = std::fmax(hi[a], hp[7 * b + 3 + a]); }
            cnt += hp[7 * b + 6];
        }
        info.n_used = (int64_t)cnt;
        if (info.n_used > (1ll << 26)) return bad(fn, "more than 2^26 used points");
        double ext = 0.0;
        for (int a = 0; a < 3; ++a) ext = std::fmax(ext, hi[a] - lo[a]);
        if (info.n_used < 2 || !(ext > 0.0)) { mvs_set_error("%s: fewer than 2 used points, or a bounding box of zero extent", fn); return MVS_E_DEGENERATE; }
        side = p.scale * ext;                                                                    // rule 2
        for (int a = 0; a < 3; ++a) g.o[a] = 0.5 * (lo[a] + hi[a]) - 0.5 * side;
        const int dmax = p.depth_max < PN_MAX_D ? p.depth_max : PN_MAX_D;
        int D = p.depth_min;
        if (dmax > p.depth_min) {                                                                // rule 3
            unsigned long long hocc[PN_MAX_D + 1];
            if ((rc = occupancy(p.depth_min, dmax, hocc))) return rc;
            for (int d = p.depth_min; d <= dmax; ++d)
                if ((double)info.n_used >= p.samples_per_node * (double)hocc[d]) D = d;
        }
        g.G = 1 << D;                                                                            // rule 4
        g.h = side / (double)g.G;
        nn = (int64_t)(g.G + 1) * (g.G + 1) * (g.G + 1);
        info.depth = D;
        info.h = g.h;
        for (int a = 0; a < 3; ++a) info.origin[a] = g.o[a];
        return MVS_OK;
    }

    int levels() {
        // the finest level: three planar arrays of 8 bytes per node — the int64 sums of the splat, then x, t and a spare — and b;
        // the levels below in one block, x | t | b each
        int rc;
        const int D = info.depth;
        if ((rc = sums.alloc(24 * (size_t)nn, s)) || (rc = rhs.alloc(8 * (size_t)nn, s))) return rc;
        size_t below = 0;
        for (int l = 1; l < D; ++l) below += 3 * (size_t)((1 << l) + 1) * ((1 << l) + 1) * ((1 << l) + 1);
        if ((rc = coarse.alloc(8 * below, s))) return rc;
        HIPCHK(hipMemsetAsync(coarse.p, 0, 8 * below, s));                    // depth >= 3: there are levels below
        double* at = coarse.as<double>();
        for (int l = 1; l < D; ++l) {
            const size_t m = (size_t)((1 << l) + 1) * ((1 << l) + 1) * ((1 << l) + 1);
            L.x[l] = at; L.t[l] = at + m; L.b[l] = at + 2 * m;
            at += 3 * m;
        }
        L.x[D] = sums.as<double>(); L.t[D] = sums.as<double>() + nn; L.b[D] = rhs.as<double>();
        return MVS_OK;
    }

    // The solver, for Op = MgPlain or MgScreened<the diagonal>: Op x = L.b[l] on every level l.
    template <class Op>
    int norm2(const double* x, double* out) {                                // |b - Op x|^2 of the finest level, on the host
        const int D = info.depth;
        const dim3 gr = pn_column_grid(g.G);
        const int np = (int)(gr.x * gr.y * gr.z);
        Op::level_args(Sc, D, [&](auto... lv) { k_mg_residual<Op><<<gr, dim3(64, 4), 0, s>>>(g.G, x, L.b[D], nullptr, red.as<double>() + 1, lv...); });
        k_pn_fold<<<dim3(1), dim3(PN_TPB), 0, s>>>(red.as<double>() + 1, np, red.as<double>());
        HIPCHK(hipGetLastError());
        return fetch(out, red.p, sizeof(double));
    }

    template <class Op>
    void smooth(int l, const double* x, double* y) {                         // one sweep of a launched level
        const int G = 1 << l;
        if constexpr (Op::screened)
            if (SC_SMOOTH_BY_ROWS) {
                k_mg_smooth<MgPlain><<<pn_column_grid(G), dim3(64, 4), 0, s>>>(G, x, L.b[l], y);
                if (sc_rows[l] > 0)
                    k_sc_smooth_rows<Op::diag><<<dim3((unsigned)((sc_rows[l] + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(sc_rows[l], sc_node[l].as<int32_t>(), G, x,
                                                                                                                        L.b[l], y, Sc.tab[l]);
                return;
            }
        Op::level_args(Sc, l, [&](auto... lv) { k_mg_smooth<Op><<<pn_column_grid(G), dim3(64, 4), 0, s>>>(G, x, L.b[l], y, lv...); });
    }
    template <class Op>
    void smooth2(int l) {
        smooth<Op>(l, L.x[l], L.t[l]);
        smooth<Op>(l, L.t[l], L.x[l]);
    }

    template <class Op>
    int vcycle() {
        const int D = info.depth;
        for (int l = D; l > PN_COARSE; --l) {
            const int G = 1 << l, Gc = G / 2;
            smooth2<Op>(l);
            Op::level_args(Sc, l, [&](auto... lv) { k_mg_residual<Op><<<pn_column_grid(G), dim3(64, 4), 0, s>>>(G, L.x[l], L.b[l], L.t[l], nullptr, lv...); });
            k_mg_restrict<<<dim3((unsigned)((Gc - 1 + 63) / 64), (unsigned)((Gc - 1 + 3) / 4), (unsigned)(Gc - 1)), dim3(64, 4), 0, s>>>(Gc, L.t[l], L.b[l - 1]);
            HIPCHK(hipMemsetAsync(L.x[l - 1], 0, 8 * (size_t)(Gc + 1) * (Gc + 1) * (Gc + 1), s));
        }
        Op::all_args(Sc, [&](auto... a) { k_mg_coarse<Op><<<dim3(1), dim3(PN_COARSE_TPB), 0, s>>>(L, D < PN_COARSE ? D : PN_COARSE, a...); });
        for (int l = PN_COARSE + 1; l <= D; ++l) {
            const int G = 1 << l;
            k_mg_prolong<<<dim3((unsigned)((G - 1 + 63) / 64), (unsigned)((G - 1 + 3) / 4), (unsigned)(G - 1)), dim3(64, 4), 0, s>>>(G, L.x[l - 1], L.x[l]);
            smooth2<Op>(l);
        }
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }

    // V cycles from the iterate in L.x[D] until the residual is at most solve_tol times the norm of the right side, which is the
    // residual of `zero`, a buffer that holds 0.  MVS_E_SOLVER comes without an error text: the caller has the words for its solve.
    template <class Op>
    int solve(const double* zero, int32_t* cycles, double* rel_residual) {
        int rc;
        const int D = info.depth;
        double b2 = 0.0, r2 = 0.0;
        if ((rc = norm2<Op>(zero, &b2))) return rc;
        if (!(b2 > 0.0)) return MVS_OK;                                       // b = 0 (or not finite): 0 solves it
        for (int c = 1; c <= p.max_cycles; ++c) {
            if ((rc = vcycle<Op>()) || (rc = norm2<Op>(L.x[D], &r2))) return rc;
            *cycles = c;
            *rel_residual = std::sqrt(r2) / std::sqrt(b2);
            if (std::sqrt(r2) <= p.solve_tol * std::sqrt(b2)) return MVS_OK;
        }
        return MVS_E_SOLVER;
    }

    // rules 5-6 (with rule 16 when the call weights): the levels, then b
    int right_side() {
        int rc;
        if ((rc = levels())) return rc;
        const unsigned nblk = (unsigned)((nn + PN_TPB - 1) / PN_TPB);
        HIPCHK(hipMemsetAsync(sums.p, 0, 24 * (size_t)nn, s));
        const dim3 pgrid((unsigned)((n + PN_TPB - 1) / PN_TPB));
        if (row_gain || (dp && (dp->flags & MVS_POISSON_WEIGHT_NORMALS)))
            k_pn_splat<true><<<pgrid, dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, sums.as<unsigned long long>(), row_gain ? row_gain : gain.as<double>());
        else
            k_pn_splat<false><<<pgrid, dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, sums.as<unsigned long long>(), nullptr);
        k_pn_rhs<<<dim3(nblk), dim3(PN_TPB), 0, s>>>(g, sums.as<long long>(), rhs.as<double>());
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }

    // rules 5-8
    int field(const char* fn) {
        int rc;
        if ((rc = right_side())) return rc;
        const int D = info.depth;
        HIPCHK(hipMemsetAsync(sums.p, 0, 16 * (size_t)nn, s));                // the sums are spent: x = 0 and the smoother's second buffer
        const dim3 gr = pn_column_grid(g.G);
        if ((rc = red.alloc(sizeof(double) * (1 + (size_t)gr.x * gr.y * gr.z), s))) return rc;
        rc = solve<MgPlain>(L.x[D], &info.cycles, &info.rel_residual);        // x = 0 is the start and the zero
        if (rc == MVS_E_SOLVER)
            mvs_set_error("%s: relative residual %.3e after %d cycles, above solve_tol %.3e", fn, info.rel_residual, info.cycles, p.solve_tol);
        return rc;
    }

    // rules 14-16: the density grid, rho_p, rho_mean and s_p
    int density() {
        int rc, Dd = 0;
        gd = pn_density_grid(g, side, info.depth, dp->density_drop, &Dd);
        nnd = (int64_t)(gd.G + 1) * (gd.G + 1) * (gd.G + 1);
        dinfo->density_depth = Dd;
        if ((rc = dsum.alloc(8 * (size_t)nnd, s)) || (rc = rho.alloc(8 * (size_t)n, s)) || (rc = gain.alloc(8 * (size_t)n, s)) ||
            (rc = dpart.alloc(24 * (size_t)PN_RED_NB, s))) return rc;
        HIPCHK(hipMemsetAsync(dsum.p, 0, 8 * (size_t)nnd, s));
        return poisson_density_rows(n, pts, nrm, density_sums(), info.n_used, dp->max_gain, rho.as<double>(), gain.as<double>(), dpart, dinfo, s);
    }
    PnDensitySums density_sums() const { return PnDensitySums{gd, nullptr, 0, dsum.as<long long>()}; }

    // rule 17, after scatter
    int vertex_density(const double* vertices, double* out) {
        return out && info.n_vertices > 0 ? poisson_vertex_density(info.n_vertices, vertices, density_sums(), out, s) : MVS_OK;
    }

    // rule 9
    int iso_value() {
        const int nb = (int)std::min<int64_t>(PN_RED_NB, (n + PN_TPB - 1) / PN_TPB);
        k_pn_iso<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, L.x[info.depth], part.as<double>() + 1);
        k_pn_fold<<<dim3(1), dim3(PN_TPB), 0, s>>>(part.as<double>() + 1, nb, part.as<double>());
        HIPCHK(hipGetLastError());
        double sum = 0.0;
        int rc = fetch(&sum, part.p, sizeof(double));
        if (rc) return rc;
        info.iso = iso = sum / (double)info.n_used;
        return MVS_OK;
    }

    PnDenseSurf surf() const { return PnDenseSurf{g, L.x[info.depth], iso}; }

    // rules 10-12 up to the counts
    int count() {
        int rc;
        const PnDenseSurf q = surf();
        const int64_t cubes = q.cube_items();
        edge_items = 7 * q.node_items();
        face_items = 12 * cubes;
        const int64_t nbe = (edge_items + PN_TPB - 1) / PN_TPB, nbf = (face_items + PN_TPB - 1) / PN_TPB;
        if ((rc = mask.alloc((size_t)cubes, s)) || (rc = words.alloc(sizeof(unsigned long long) * PN_WAVES * (size_t)nbe, s)) ||
            (rc = ve.alloc((size_t)nbe, s)) || (rc = fa.alloc((size_t)nbf, s))) return rc;
        k_pn_cubemask<<<dim3((unsigned)((cubes + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(q, mask.as<uint8_t>());
        k_pn_edge_count<<<dim3((unsigned)nbe), dim3(PN_TPB), 0, s>>>(q, edge_items, words.as<unsigned long long>(), ve.cnt.as<int32_t>());
        ve.run((int)nbe, s);
        k_pn_face_count<<<dim3((unsigned)nbf), dim3(PN_TPB), 0, s>>>(mask.as<uint8_t>(), face_items, fa.cnt.as<int32_t>());
        fa.run((int)nbf, s);
        HIPCHK(hipGetLastError());
        int32_t nv = 0, nf = 0;                                               // base[nb]: all survivors
        HIPCHK(hipMemcpyAsync(&nv, ve.base.as<int32_t>() + nbe, 4, hipMemcpyDeviceToHost, s));
        if ((rc = fetch(&nf, fa.base.as<int32_t>() + nbf, 4))) return rc;
        info.n_vertices = nv;
        info.n_faces = nf;
        return MVS_OK;
    }

    int scatter(double* vertices, int32_t* faces) {
        if (info.n_vertices == 0) return MVS_OK;
        const int64_t nbe = (edge_items + PN_TPB - 1) / PN_TPB, nbf = (face_items + PN_TPB - 1) / PN_TPB;
        const PnDenseSurf q = surf();
        k_pn_vertex_scatter<<<dim3((unsigned)nbe), dim3(PN_TPB), 0, s>>>(q, edge_items, words.as<unsigned long long>(), ve.base.as<int32_t>(), vertices);
        k_pn_face_scatter<<<dim3((unsigned)nbf), dim3(PN_TPB), 0, s>>>(q, mask.as<uint8_t>(), face_items, words.as<unsigned long long>(),
                                                                      ve.base.as<int32_t>(), vertices, fa.base.as<int32_t>(), faces);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        return MVS_OK;
    }

    // rule 20 on the finest level, and the rows of every level below from the level above; dense (may be NULL): [nn][27] int64 on the
    // device, the sums of the finest level
    int stencils(double lambda, long long* dense) {
        int rc;
        const int D = info.depth;
        const dim3 pgrid((unsigned)((n + PN_TPB - 1) / PN_TPB));
        if ((rc = sc_flag.alloc((size_t)nn, s)) || (rc = sn.alloc((size_t)((nn + PN_TPB - 1) / PN_TPB), s))) return rc;
        for (int l = D; l >= 1; --l) {
            const int G = 1 << l;
            const int64_t nl = (int64_t)(G + 1) * (G + 1) * (G + 1), nb = (nl + PN_TPB - 1) / PN_TPB;
            if ((rc = sc_idx[l].alloc(4 * (size_t)nl, s))) return rc;
            if (l == D) {
                HIPCHK(hipMemsetAsync(sc_flag.p, 0, (size_t)nl, s));
                k_sc_flag<<<pgrid, dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, sc_flag.as<uint8_t>());
            } else {
                k_sc_flag_coarse<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(G, sc_idx[l + 1].as<int32_t>(), sc_flag.as<uint8_t>());
            }
            k_sc_count<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(nl, sc_flag.as<uint8_t>(), sn.cnt.as<int32_t>());
            sn.run((int)nb, s);
            HIPCHK(hipGetLastError());
            int32_t rows = 0;                                                 // base[nb]: all flagged nodes
            if ((rc = fetch(&rows, sn.base.as<int32_t>() + nb, 4))) return rc;
            sc_rows[l] = rows;
            if ((rc = sc_tab[l].alloc(8 * (size_t)SC_ROW * (size_t)rows, s)) || (rc = sc_node[l].alloc(4 * (size_t)rows, s))) return rc;
            k_sc_number<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(nl, sc_flag.as<uint8_t>(), sn.base.as<int32_t>(), sc_idx[l].as<int32_t>(),
                                                                   sc_node[l].as<int32_t>());
            if (l == D) {
                HIPCHK(hipMemsetAsync(sc_tab[l].p, 0, 8 * (size_t)SC_ROW * (size_t)rows, s));
                k_sc_splat<<<pgrid, dim3(PN_TPB), 0, s>>>(n, pts, nrm, g, lambda, sc_idx[l].as<int32_t>(), sc_tab[l].as<unsigned long long>());
                if (dense)
                    k_sc_dense<<<dim3((unsigned)((27 * nl + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(nl, sc_idx[l].as<int32_t>(), sc_tab[l].as<long long>(), dense);
                if (rows > 0) k_sc_convert<<<dim3((unsigned)((rows + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(rows, sc_tab[l].as<long long>());
            } else if (rows > 0) {
                k_sc_coarsen<<<dim3((unsigned)((rows + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(rows, sc_node[l].as<int32_t>(), G, sc_idx[l + 1].as<int32_t>(),
                                                                                                    sc_tab[l + 1].as<double>(), sc_tab[l].as<double>());
            }
            HIPCHK(hipGetLastError());
            Sc.idx[l] = sc_idx[l].as<int32_t>();
            Sc.tab[l] = sc_tab[l].as<double>();
        }
        return MVS_OK;
    }

    // rules 19-21, after rule 9: sinfo, the stencils and f in the place of b.  alpha = 0 stops after rule 19.
    int screen_setup(long long* dense) {
        int rc;
        unsigned long long hocc[PN_MAX_D + 1];
        sinfo->target = sinfo->iso_unscreened = iso;
        if ((rc = occupancy(info.depth, info.depth, hocc))) return rc;         // occupied(D), whether or not rule 3 had a choice
        sinfo->occupied = (int64_t)hocc[info.depth];
        if (!(sp->alpha > 0.0)) return MVS_OK;
        sinfo->lambda = pn_screen_lambda(sp->alpha, info.n_used, sinfo->occupied);
        if ((rc = stencils(sinfo->lambda, dense))) return rc;
        sinfo->active_nodes = sc_rows[info.depth];
        k_sc_rhs<<<dim3((unsigned)((nn + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(nn, Sc.idx[info.depth], Sc.tab[info.depth], sinfo->target, rhs.as<double>());
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }

    // rule 22: from chi0 in L.x[D], with f in L.b[D]
    int screen_solve(const char* fn) {
        const int D = info.depth;
        HIPCHK(hipMemsetAsync(L.t[D], 0, 8 * (size_t)nn, s));                 // M 0 = 0: the residual of zero is f
        const int rc = with_diagonal(diag, [&](auto op) { return solve<decltype(op)>(L.t[D], &sinfo->cycles, &sinfo->rel_residual); });
        if (rc == MVS_E_SOLVER)
            mvs_set_error("%s: screened solve: relative residual %.3e after %d cycles, above solve_tol %.3e", fn, sinfo->rel_residual, sinfo->cycles, p.solve_tol);
        return rc;
    }

    int counts(const char* fn) {
        int rc;
        if ((rc = grid(fn)) || (dp && (rc = density())) || (rc = field(fn)) || (rc = iso_value())) return rc;
        if (sp) {                                                             // rules 19-23
            if ((rc = screen_setup(nullptr))) return rc;
            if (sp->alpha > 0.0 && ((rc = screen_solve(fn)) || (rc = iso_value()))) return rc;
        }
        return count();
    }
};

// The device form of every entry, after its checks: the counts, the capacity test, the scatter and the vertex densities.
int reconstruct(const PnCall& c, const double* pts_dev, const double* nrm_dev, PnOut o, hipStream_t s) {
    int rc;
    PnRun run(c, pts_dev, nrm_dev, s);
    if ((rc = run.counts(c.fn))) return rc;
    return poisson_finish(c.fn, run, *c.info, o);
}

// what every entry opens with
int open_call(const PnCall& c, const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b) {
    const int rc = check_call(c, out_a, cap_a, out_b, cap_b);
    return rc ? rc : need_device();
}
int up_points(const PnCall& c, Scratch& dp, Scratch& dn) {
    const int rc = up(dp, c.points, 3 * (size_t)c.n);
    return rc ? rc : up(dn, c.normals, 3 * (size_t)c.n);
}

// The host form of every entry: the points go up, the device form fills blocks, the blocks come down.
int reconstruct_host(const PnCall& c, double* vertices, double* density, int64_t vcap, int32_t* faces, int64_t fcap) {
    int rc;
    Scratch dp, dn, dv, dd, df;
    if ((rc = open_call(c, vertices, vcap, faces, fcap)) || (rc = up_points(c, dp, dn)) ||
        (rc = reconstruct(c, dp.as<double>(), dn.as<double>(), PnOut{nullptr, nullptr, nullptr, vcap, fcap, &dv, density ? &dd : nullptr, &df}, nullptr)))
        return rc;
    const size_t V = (size_t)c.info->n_vertices, F = (size_t)c.info->n_faces;
    if ((density && (rc = down(density, dd, V))) || (rc = down(vertices, dv, 3 * V))) return rc;
    return down(faces, df, 3 * F);
}

}  // namespace

// the device form for a caller inside the library that cannot know the counts in advance (mvs_processor_poisson and its kin)
int poisson_blocks(const PnCall& c, Scratch* vertices, Scratch* density, Scratch* faces) {
    const int rc = check_call(c, nullptr, 0, nullptr, 0);
    if (rc) return rc;
    return reconstruct(c, c.points, c.normals, PnOut{nullptr, nullptr, nullptr, INT64_MAX, INT64_MAX, vertices, c.rules >= PN_DENSITY ? density : nullptr, faces},
                       nullptr);
}

// ------------------------------------------------------------------ for poisson_band.hip (poisson_base.h) ----
int poisson_check_plain(const PnCall& c, int max_depth, const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b) {
    return check_pn(c.fn, c.n, c.points, c.normals, c.p, c.info, out_a, cap_a, out_b, cap_b, max_depth);
}

int poisson_check_density(const char* fn, int64_t n, const mvs_poisson_density_params* dp, const void* dinfo) { return check_pn_density(fn, n, dp, dinfo); }

int poisson_check_screen(const char* fn, const mvs_poisson_screen_params* sp, const void* sinfo) { return check_pn_screen(fn, sp, sinfo); }

// PnScan: counts, their scan and its two levels
int PnScan::alloc(size_t nb, hipStream_t s) {
    const size_t rows = (nb + PN_SCAN_CH - 1) / PN_SCAN_CH;
    int rc;
    bytes = (int64_t)(4 * nb + 4 * (nb + 1) + 4 * rows * (PN_SCAN_CH + 1) + 4 * rows + 4 * (rows + 1));
    if ((rc = cnt.alloc(4 * nb, s)) || (rc = base.alloc(4 * (nb + 1), s)) || (rc = local.alloc(4 * rows * (PN_SCAN_CH + 1), s)) ||
        (rc = tot.alloc(4 * rows, s))) return rc;
    return rbase.alloc(4 * (rows + 1), s);
}
void PnScan::run(int nb, hipStream_t s) {
    const int rows = (nb + PN_SCAN_CH - 1) / PN_SCAN_CH;
    k_pn_scan_rows<<<dim3((unsigned)rows), dim3(PN_TPB), 0, s>>>(cnt.as<int32_t>(), nb, local.as<int32_t>(), tot.as<int32_t>());
    k_pn_scan_totals<<<dim3(1), dim3(PN_TPB), 0, s>>>(tot.as<int32_t>(), rows, rbase.as<int32_t>());
    k_pn_scan_add<<<dim3((unsigned)(nb / PN_TPB + 1)), dim3(PN_TPB), 0, s>>>(local.as<int32_t>(), rbase.as<int32_t>(), nb, rows, base.as<int32_t>());
}

void poisson_fold(const double* part_dev, int n, double* out_dev, hipStream_t s) { k_pn_fold<<<dim3(1), dim3(PN_TPB), 0, s>>>(part_dev, n, out_dev); }

static_assert(PN_SC_ROW == SC_ROW, "one row layout");
void poisson_screen_convert(int64_t rows, long long* tab_dev, hipStream_t s) {
    if (rows > 0) k_sc_convert<<<dim3((unsigned)((rows + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(rows, tab_dev);
}

void poisson_face_count(const uint8_t* mask_dev, int64_t items, int32_t* cnt_dev, hipStream_t s) {
    k_pn_face_count<<<dim3((unsigned)((items + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(mask_dev, items, cnt_dev);
}

// f(the accessor of d's storage): the one run-time choice between the two instantiations of the density kernels
template <class F>
static void with_sums(const PnDensitySums& d, F f) {
    if (d.num) f(BdBlockSums{d.num, d.T, d.sums});
    else f(BdDenseSums{d.g.G, d.sums});
}

int poisson_density_rows(int64_t n, const double* pts, const double* nrm, const PnDensitySums& d, int64_t n_used, double max_gain, double* rho,
                         double* gain, Scratch& part, mvs_poisson_density_info* dinfo, hipStream_t s) {
    const int nb = (int)std::min<int64_t>(PN_RED_NB, (n + PN_TPB - 1) / PN_TPB);
    double* part_d = part.as<double>();
    long long* part_q = part.as<long long>() + 2 * PN_RED_NB;
    with_sums(d, [&](auto sums) {
        k_pn_density_splat<<<dim3((unsigned)((n + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(n, pts, nrm, d.g, sums, (unsigned long long*)d.sums);
        k_pn_point_density<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(n, pts, nrm, d.g, sums, rho, part_d, part_q);
    });
    HIPCHK(hipGetLastError());
    std::vector<double> hd((size_t)2 * nb);
    std::vector<long long> hq((size_t)nb);
    HIPCHK(hipMemcpyAsync(hd.data(), part_d, 16 * (size_t)nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hq.data(), part_q, 8 * (size_t)nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    long long q = 0;
    for (int b = 0; b < nb; ++b) { lo = std::fmin(lo, hd[2 * b]); hi = std::fmax(hi, hd[2 * b + 1]); q += hq[b]; }
    dinfo->mean_density = pn_rho_mean(q, n_used);
    dinfo->min_point_density = lo;
    dinfo->max_point_density = hi;
    // rule 16: s_p of every row and the count of the used rows cut at max_gain; the partials above are spent
    int32_t* part_c = part.as<int32_t>();
    k_pn_gain<<<dim3((unsigned)nb), dim3(PN_TPB), 0, s>>>(n, pts, nrm, rho, dinfo->mean_density, max_gain, gain, part_c);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hc((size_t)nb);
    HIPCHK(hipMemcpyAsync(hc.data(), part_c, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    dinfo->n_clamped = 0;
    for (int b = 0; b < nb; ++b) dinfo->n_clamped += hc[b];
    return MVS_OK;
}

int poisson_vertex_density(int64_t nv, const double* vertices, const PnDensitySums& d, double* out, hipStream_t s) {
    with_sums(d, [&](auto sums) { k_pn_vertex_density<<<dim3((unsigned)((nv + PN_TPB - 1) / PN_TPB)), dim3(PN_TPB), 0, s>>>(nv, vertices, d.g, sums, out); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

int poisson_cube(const PnCall& c, const double* pts_dev, const double* nrm_dev, hipStream_t s, double origin[3], double* side) {
    mvs_poisson_params p3 = *c.p;
    p3.depth_min = p3.depth_max = 3;      // rule 3 has no choice to make: no occupancy pass
    PnCall c3 = c;
    c3.p = &p3;
    PnRun run(c3, pts_dev, nrm_dev, s);
    const int rc = run.grid(c.fn);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) origin[a] = run.g.o[a];
    *side = run.side;
    return MVS_OK;
}

PnBaseField::~PnBaseField() { delete (PnRun*)run; }

int PnBaseField::solve(const PnCall& c, const double* pts_dev, const double* nrm_dev, hipStream_t s, const double* gain_dev) {
    int rc;
    PnRun* r = new PnRun(c, pts_dev, nrm_dev, s);
    run = r;
    r->row_gain = gain_dev;
    if ((rc = r->grid(c.fn)) || (rc = r->field(c.fn))) return rc;
    if (c.info->cycles > 0) {
        // One cycle past the criterion.  The finer levels take this field as their fixed values and in their right sides and cannot
        // reduce its error; a cycle costs a thirteenth of this solve and takes the error down by the cycle's contraction.
        double before = 0.0, after = 0.0;
        double* x = r->L.x[c.info->depth];
        if ((rc = r->norm2<MgPlain>(x, &before))) return rc;
        if (before > 0.0) {
            if ((rc = r->vcycle<MgPlain>()) || (rc = r->norm2<MgPlain>(x, &after))) return rc;
            c.info->cycles += 1;
            c.info->rel_residual *= std::sqrt(after) / std::sqrt(before);
        }
    }
    g = r->g;
    chi = r->L.x[c.info->depth];
    size_t below = 0;
    for (int l = 1; l < c.info->depth; ++l) below += 3 * (size_t)((1 << l) + 1) * ((1 << l) + 1) * ((1 << l) + 1);
    bytes = (int64_t)(32 * (size_t)r->nn + 8 * below);
    if (c.sp && c.sinfo) {                                                    // rule 37: rules 19-22 on this field, from it
        if ((rc = r->iso_value()) || (rc = r->screen_setup(nullptr))) return rc;
        bytes += (int64_t)r->nn + r->sn.bytes;
        for (int l = 1; l <= c.info->depth; ++l) bytes += 4 * (int64_t)((1 << l) + 1) * ((1 << l) + 1) * ((1 << l) + 1) + (8 * SC_ROW + 4) * r->sc_rows[l];
        if (c.sp->alpha > 0.0) {
            if ((rc = r->screen_solve(c.fn))) return rc;
            if (c.sinfo->cycles > 0) {
                double before = 0.0, after = 0.0;
                double* x = r->L.x[c.info->depth];
                rc = with_diagonal(r->diag, [&](auto op) -> int {
                    using Op = decltype(op);
                    int q = r->template norm2<Op>(x, &before);
                    if (q || !(before > 0.0)) return q;
                    if ((q = r->template vcycle<Op>()) || (q = r->template norm2<Op>(x, &after))) return q;
                    c.sinfo->cycles += 1;
                    c.sinfo->rel_residual *= std::sqrt(after) / std::sqrt(before);
                    return MVS_OK;
                });
                if (rc) return rc;
            }
        }
    }
    return MVS_OK;
}

int poisson_dense_dev(const PnCall& c, const double* pts_dev, const double* nrm_dev, PnOut o, hipStream_t s) { return reconstruct(c, pts_dev, nrm_dev, o, s); }

extern "C" {

void mvs_poisson_default_params(mvs_poisson_params* p) {
    if (!p) return;
    p->scale = 1.1; p->samples_per_node = 1.5; p->solve_tol = 1e-8;
    p->depth_max = 10; p->depth_min = 7; p->max_cycles = 64; p->reserved = 0;
}

int mvs_poisson_reconstruct_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p, mvs_poisson_info* info,
                                double* vertices_dev, int64_t vertex_capacity, int32_t* faces_dev, int64_t face_capacity, void* hip_stream) {
    MVS_TRACE();
    const PnCall c{__func__, PN_PLAIN, n, points_dev, normals_dev, p, info, nullptr, nullptr, nullptr, nullptr};
    const int rc = open_call(c, vertices_dev, vertex_capacity, faces_dev, face_capacity);
    return rc ? rc : reconstruct(c, points_dev, normals_dev, PnOut{vertices_dev, nullptr, faces_dev, vertex_capacity, face_capacity}, (hipStream_t)hip_stream);
}

int mvs_poisson_reconstruct(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p, mvs_poisson_info* info,
                            double* vertices, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity) {
    MVS_TRACE();
    return reconstruct_host(PnCall{__func__, PN_PLAIN, n, points, normals, p, info, nullptr, nullptr, nullptr, nullptr}, vertices, nullptr, vertex_capacity,
                            faces, face_capacity);
}

// MVS_E_SOLVER still hands out the field the solve reached: the hooks go on after it
int mvs_test_poisson_field(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p, mvs_poisson_info* info, double* rhs,
                           double* chi, int64_t node_capacity) {
    MVS_TRACE();
    const PnCall c{__func__, PN_PLAIN, n, points, normals, p, info, nullptr, nullptr, nullptr, nullptr};
    Scratch dp, dn;
    int rc = open_call(c, rhs, node_capacity, chi, node_capacity);
    if (rc || (rc = up_points(c, dp, dn))) return rc;
    PnRun run(c, dp.as<double>(), dn.as<double>(), nullptr);
    if ((rc = run.grid(__func__))) return rc;
    if (run.nn > node_capacity) return bad(__func__, "node_capacity is below (2^depth + 1)^3 (info holds the depth)");
    const int frc = run.field(__func__);
    if (frc && frc != MVS_E_SOLVER) return frc;
    if (!frc && (rc = run.iso_value())) return rc;
    HIPCHK(hipMemcpy(rhs, run.rhs.p, 8 * (size_t)run.nn, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(chi, run.L.x[info->depth], 8 * (size_t)run.nn, hipMemcpyDeviceToHost));
    return frc;
}

// ------------------------------------------------------------------ rules 14-17 ----
void mvs_poisson_density_default_params(mvs_poisson_density_params* p) {
    if (!p) return;
    p->max_gain = 4.0; p->flags = 0; p->density_drop = 1;
}

int mvs_poisson_reconstruct_density_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                        const mvs_poisson_density_params* dparams, mvs_poisson_info* info, mvs_poisson_density_info* dinfo,
                                        double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                        int64_t face_capacity, void* hip_stream) {
    MVS_TRACE();
    const PnCall c{__func__, PN_DENSITY, n, points_dev, normals_dev, p, info, dparams, dinfo, nullptr, nullptr};
    const int rc = open_call(c, vertices_dev, vertex_capacity, faces_dev, face_capacity);
    return rc ? rc : reconstruct(c, points_dev, normals_dev, PnOut{vertices_dev, vertex_density_dev, faces_dev, vertex_capacity, face_capacity},
                                 (hipStream_t)hip_stream);
}

int mvs_poisson_reconstruct_density(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                    const mvs_poisson_density_params* dparams, mvs_poisson_info* info, mvs_poisson_density_info* dinfo,
                                    double* vertices, double* vertex_density, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity) {
    MVS_TRACE();
    return reconstruct_host(PnCall{__func__, PN_DENSITY, n, points, normals, p, info, dparams, dinfo, nullptr, nullptr}, vertices, vertex_density,
                            vertex_capacity, faces, face_capacity);
}

int mvs_test_poisson_density(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                             const mvs_poisson_density_params* dparams, mvs_poisson_info* info, mvs_poisson_density_info* dinfo,
                             int64_t* node_sums, int64_t density_node_capacity, double* rho, double* gain, double* rhs, double* chi,
                             int64_t node_capacity) {
    MVS_TRACE();
    const PnCall c{__func__, PN_DENSITY, n, points, normals, p, info, dparams, dinfo, nullptr, nullptr};
    Scratch dp, dn;
    int rc = check_call(c, node_sums, density_node_capacity, rhs, node_capacity);
    if (rc) return rc;
    if (!rho || !gain) return bad(__func__, "rho or gain is NULL");
    if ((rc = need_device()) || (rc = up_points(c, dp, dn))) return rc;
    PnRun run(c, dp.as<double>(), dn.as<double>(), nullptr);
    if ((rc = run.grid(__func__))) return rc;
    int Dd = 0;
    const PnGrid gd = pn_density_grid(run.g, run.side, info->depth, dparams->density_drop, &Dd);
    dinfo->density_depth = Dd;
    if ((int64_t)(gd.G + 1) * (gd.G + 1) * (gd.G + 1) > density_node_capacity || run.nn > node_capacity)
        return bad(__func__, "a node capacity is below (2^depth + 1)^3 (info and dinfo hold the depths)");
    if ((rc = run.density())) return rc;
    int frc = MVS_OK;
    if (chi) {
        frc = run.field(__func__);
        if (frc && frc != MVS_E_SOLVER) return frc;
        if (!frc && (rc = run.iso_value())) return rc;
        HIPCHK(hipMemcpy(chi, run.L.x[info->depth], 8 * (size_t)run.nn, hipMemcpyDeviceToHost));
    } else if ((rc = run.right_side())) return rc;
    HIPCHK(hipMemcpy(node_sums, run.dsum.p, 8 * (size_t)run.nnd, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rho, run.rho.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(gain, run.gain.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rhs, run.rhs.p, 8 * (size_t)run.nn, hipMemcpyDeviceToHost));
    return frc;
}

// ------------------------------------------------------------------ rules 19-23 ----
void mvs_poisson_screen_default_params(mvs_poisson_screen_params* p) {
    if (!p) return;
    p->alpha = 4.0; p->reserved = 0;
}

int mvs_poisson_reconstruct_screened_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                         const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams,
                                         mvs_poisson_info* info, mvs_poisson_density_info* dinfo, mvs_poisson_screen_info* sinfo,
                                         double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                         int64_t face_capacity, void* hip_stream) {
    MVS_TRACE();
    const PnCall c{__func__, PN_SCREENED, n, points_dev, normals_dev, p, info, dparams, dinfo, sparams, sinfo};
    const int rc = open_call(c, vertices_dev, vertex_capacity, faces_dev, face_capacity);
    return rc ? rc : reconstruct(c, points_dev, normals_dev, PnOut{vertices_dev, vertex_density_dev, faces_dev, vertex_capacity, face_capacity},
                                 (hipStream_t)hip_stream);
}

int mvs_poisson_reconstruct_screened(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                     const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams, mvs_poisson_info* info,
                                     mvs_poisson_density_info* dinfo, mvs_poisson_screen_info* sinfo, double* vertices, double* vertex_density,
                                     int64_t vertex_capacity, int32_t* faces, int64_t face_capacity) {
    MVS_TRACE();
    return reconstruct_host(PnCall{__func__, PN_SCREENED, n, points, normals, p, info, dparams, dinfo, sparams, sinfo}, vertices, vertex_density,
                            vertex_capacity, faces, face_capacity);
}

int mvs_test_poisson_screened(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                              const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams, mvs_poisson_info* info,
                              mvs_poisson_density_info* dinfo, mvs_poisson_screen_info* sinfo, int64_t* stencil, double* f, double* chi0, double* chi,
                              int64_t node_capacity, int32_t diagonal) {
    MVS_TRACE();
    const PnCall c{__func__, PN_SCREENED, n, points, normals, p, info, dparams, dinfo, sparams, sinfo};
    Scratch dp, dn, dense;
    int rc = check_call(c, f, node_capacity, chi, node_capacity);
    if (rc) return rc;
    if (!stencil || !chi0) return bad(__func__, "stencil or chi0 is NULL");
    if (diagonal < 0 || diagonal > 2) return bad(__func__, "diagonal is not 0, 1 or 2");
    if ((rc = need_device()) || (rc = up_points(c, dp, dn))) return rc;
    PnRun run(c, dp.as<double>(), dn.as<double>(), nullptr);
    run.diag = diagonal;
    if ((rc = run.grid(__func__))) return rc;
    if (run.nn > node_capacity) return bad(__func__, "node_capacity is below (2^depth + 1)^3 (info holds the depth)");
    const size_t nn = (size_t)run.nn;
    if ((rc = run.density()) || (rc = run.field(__func__)) || (rc = run.iso_value())) return rc;
    HIPCHK(hipMemcpy(chi0, run.L.x[info->depth], 8 * nn, hipMemcpyDeviceToHost));
    if ((rc = dense.alloc(8 * 27 * nn))) return rc;
    HIPCHK(hipMemset(dense.p, 0, 8 * 27 * nn));                              // alpha = 0: no stencil
    if ((rc = run.screen_setup(dense.as<long long>()))) return rc;
    HIPCHK(hipMemcpy(stencil, dense.p, 8 * 27 * nn, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(f, run.rhs.p, 8 * nn, hipMemcpyDeviceToHost));
    int src = MVS_OK;
    if (sparams->alpha > 0.0) {
        src = run.screen_solve(__func__);
        if (src && src != MVS_E_SOLVER) return src;
        if (!src && (rc = run.iso_value())) return rc;
    }
    HIPCHK(hipMemcpy(chi, run.L.x[info->depth], 8 * nn, hipMemcpyDeviceToHost));
    return src;
}

}  // extern "C"

