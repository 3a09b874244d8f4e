// poisson_rules.h — the per-point and per-tetrahedron rules of mvs_poisson_reconstruct (include/mvs.h): the cell of a point (3), its
// corners, weights and quantised contributions (5), the seven edge types and the six Kuhn tetrahedra of a cube (10), the vertex of a
// crossed edge (11) and the polygon of a tetrahedron (12); of mvs_poisson_reconstruct_density the density grid (14), the density at a
// point or a vertex (15, 17), the gain (16) and the pass test of the trim (18).  One body for the kernels of poisson.hip and for host code:
// tests/poisson_rules.cpp and tests/poisson_density_rules.cpp run it as programs of their own, tests/ref_poisson.py and
// tests/ref_poisson_density.py restate it.  Every operation is an fp64 + - * / in
// the order written; the library is built with -ffp-contract=off.
#ifndef MVS_POISSON_RULES_H_
#define MVS_POISSON_RULES_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

struct PnGrid {                         // rule 4: nodes (ix, iy, iz) in [0, G]^3 at o + h * i
    double o[3], h;
    int32_t G;
};

__host__ __device__ inline int64_t pn_node(int32_t G, int ix, int iy, int iz) { return ((int64_t)iz * (G + 1) + iy) * (G + 1) + ix; }
// corner c = bx + 2 by + 4 bz of the cube whose lower corner is node i0
__host__ __device__ inline int64_t pn_corner_node(int32_t G, const int i0[3], int c) {
    return pn_node(G, i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
}

// rule 1
__host__ __device__ inline bool pn_used(const double* p, const double* n) {
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
}

// rule 3: the cell of coordinate p along one axis of a cube cut into n cells of size cs from o
__host__ __device__ inline int pn_cell(double p, double o, double cs, int n) {
    const double c = floor((p - o) / cs);
    return c < 0.0 ? 0 : c > (double)(n - 1) ? n - 1 : (int)c;
}

// rule 5: the lower corner i0 of the point's cube and the eight weights, corner c = bx + 2 by + 4 bz
__host__ __device__ inline void pn_corners_weights(const double* p, const PnGrid& g, int i0[3], double w[8]) {
    double f[3];
    for (int a = 0; a < 3; ++a) {
        const double q = (p[a] - g.o[a]) / g.h;
        i0[a] = pn_cell(p[a], g.o[a], g.h, g.G);
        f[a] = q - (double)i0[a];
    }
    for (int c = 0; c < 8; ++c) {
        const double wx = c & 1 ? f[0] : 1.0 - f[0], wy = c & 2 ? f[1] : 1.0 - f[1], wz = c & 4 ? f[2] : 1.0 - f[2];
        w[c] = (wx * wy) * wz;
    }
}

// rule 5: a contribution x = w * n_a in units of 2^-36, round to nearest even (the default rounding mode)
__host__ __device__ inline long long pn_quant(double x) { return llrint(x * 68719476736.0); }
__host__ __device__ inline double pn_dequant(long long s) { return (double)s * (1.0 / 68719476736.0); }

// rule 14: the density grid of a cube of this side at depth D: Dd = max(D - drop, 2), the origin of rule 2
__host__ __device__ inline PnGrid pn_density_grid(const PnGrid& g, double side, int D, int drop, int* Dd) {
    PnGrid d = g;
    *Dd = D - drop > 2 ? D - drop : 2;
    d.G = 1 << *Dd;
    d.h = side / (double)d.G;
    return d;
}

// rule 15: the trilinear W at p over the int64 node sums of rule 14 (corners and weights of rule 5 on the density grid, added in corner
// order); the same body is rule 17 at a vertex
__host__ __device__ inline double pn_density_at(const double* p, const PnGrid& gd, const long long* sums) {
    int i0[3];
    double w[8], v = 0.0;
    pn_corners_weights(p, gd, i0, w);
    for (int c = 0; c < 8; ++c) v = v + w[c] * pn_dequant(sums[pn_corner_node(gd.G, i0, c)]);
    return v;
}

// rule 15: a point density in units of 2^-16 for the order-free sum behind rho_mean, and the mean of N of them
__host__ __device__ inline long long pn_rho_quant(double rho) { return llrint(rho * 65536.0); }
__host__ __device__ inline double pn_rho_mean(long long sum, long long N) { return (double)sum * (1.0 / 65536.0) / (double)N; }

// rule 16: the gain of a point of density rho (rho = 0 gives max_gain)
__host__ __device__ inline double pn_gain(double rho_mean, double rho, double max_gain) {
    const double s = rho_mean / rho;
    return s > max_gain ? max_gain : s;
}

// rule 19: the screening weight of every used point: alpha over the mean number of used points per occupied cell, at least 1
__host__ __device__ inline double pn_screen_lambda(double alpha, long long N, long long occ) {
    const double r = (double)N / (double)occ;
    return alpha / (r > 1.0 ? r : 1.0);
}

// rule 20: the 27 offsets {-1, 0, 1}^3 of a stencil in the order (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
__host__ __device__ inline int pn_screen_offset(int dx, int dy, int dz) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }

// rule 20: the contribution of the corner pair c1 <= c2 (corner order bx + 2 by + 4 bz) of a point with the weights w of rule 5, in
// units of 2^-30: it goes to the entry (node of c1, offset *o12 = c2 - c1) and, when c1 != c2, to (node of c2, offset *o21 = c1 - c2)
__host__ __device__ inline long long pn_screen_pair(double lambda, const double w[8], int c1, int c2, int* o12, int* o21) {
    const int dx = (c2 & 1) - (c1 & 1), dy = (c2 >> 1 & 1) - (c1 >> 1 & 1), dz = (c2 >> 2 & 1) - (c1 >> 2 & 1);
    *o12 = pn_screen_offset(dx, dy, dz);
    *o21 = pn_screen_offset(-dx, -dy, -dz);
    return llrint(((lambda * w[c1]) * w[c2]) * 1073741824.0);
}
__host__ __device__ inline double pn_screen_dequant(long long s) { return (double)s * (1.0 / 1073741824.0); }

// rule 18: does a value pass the threshold?  NaN does not
__host__ __device__ inline bool pn_trim_pass(double value, double threshold) { return value >= threshold; }

// rule 10: an edge type's offset as a bit mask (x = 1, y = 2, z = 4), types 0..6 = +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z; and back
__host__ __device__ inline int pn_type_mask(int type) { return (0x7653421 >> (4 * type)) & 15; }
__host__ __device__ inline int pn_mask_type(int mask) { return (0x65423100 >> (4 * mask)) & 15; }

// rule 10: corner i (0..3) of Kuhn tetrahedron k (0..5 = xyz, xzy, yxz, yzx, zxy, zyx) as an offset mask from the cube origin
__host__ __device__ inline int pn_tet_corner(int k, int i) {
    const int a = k >> 1, b = (0x489 >> (2 * k)) & 3;
    return i == 0 ? 0 : i == 1 ? 1 << a : i == 2 ? (1 << a) | (1 << b) : 7;
}

// the edge between corners i and j of tetrahedron k: the offset mask of its lower node from the cube origin, and its type
__host__ __device__ inline void pn_tet_edge(int k, int i, int j, int* node_mask, int* type) {
    const int lo = pn_tet_corner(k, i < j ? i : j), hi = pn_tet_corner(k, i < j ? j : i);
    *node_mask = lo;
    *type = pn_mask_type(hi ^ lo);
}

// rule 12: the I-O edges of a tetrahedron whose corner i is inside when bit i of `in` is set, as the listed cycle of (inside corner,
// outside corner) pairs: three edges for |I| = 1 or 3 (the O resp. I corners ascending), AC AD BD BC for I = {A < B}, O = {C < D}.
// -> the cycle's length: 0, 3 or 4
__host__ __device__ inline int pn_tet_cycle(int in, int ci[4], int co[4]) {
    int I[4], O[4], ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) { if (in >> i & 1) I[ni++] = i; else O[no++] = i; }
    if (ni == 0 || no == 0) return 0;
    if (ni == 1) { for (int q = 0; q < 3; ++q) { ci[q] = I[0]; co[q] = O[q]; } return 3; }
    if (ni == 3) { for (int q = 0; q < 3; ++q) { ci[q] = I[q]; co[q] = O[0]; } return 3; }
    ci[0] = I[0]; co[0] = O[0]; ci[1] = I[0]; co[1] = O[1]; ci[2] = I[1]; co[2] = O[1]; ci[3] = I[1]; co[3] = O[0];
    return 4;
}

// rule 12: d = mean(O corners) - mean(I corners) of tetrahedron k, in cells (both sets non-empty)
__host__ __device__ inline void pn_tet_dir(int k, int in, double d[3]) {
    int si[3] = {0, 0, 0}, so[3] = {0, 0, 0}, ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
        const int m = pn_tet_corner(k, i);
        if (in >> i & 1) { ++ni; for (int a = 0; a < 3; ++a) si[a] += m >> a & 1; }
        else { ++no; for (int a = 0; a < 3; ++a) so[a] += m >> a & 1; }
    }
    for (int a = 0; a < 3; ++a) d[a] = (double)so[a] / (double)no - (double)si[a] / (double)ni;
}

// rule 12: orient the cycle idx[n] (n = 3 or 4, positions pos) so that its normal — (p1 - p0) x (p2 - p0), for the quad plus
// (p2 - p0) x (p3 - p0) — has a positive dot product with d (reversed when the product is negative; a zero or NaN product keeps the
// listed cycle), then rotate it so that its smallest index comes first
__host__ __device__ inline void pn_polygon(int n, int32_t* idx, const double (*pos)[3], const double* d) {
    double e1[3], e2[3], e3[3], nr[3];
    for (int a = 0; a < 3; ++a) { e1[a] = pos[1][a] - pos[0][a]; e2[a] = pos[2][a] - pos[0][a]; e3[a] = n == 4 ? pos[3][a] - pos[0][a] : 0.0; }
    nr[0] = e1[1] * e2[2] - e1[2] * e2[1]; nr[1] = e1[2] * e2[0] - e1[0] * e2[2]; nr[2] = e1[0] * e2[1] - e1[1] * e2[0];
    if (n == 4) {
        nr[0] = nr[0] + (e2[1] * e3[2] - e2[2] * e3[1]); nr[1] = nr[1] + (e2[2] * e3[0] - e2[0] * e3[2]); nr[2] = nr[2] + (e2[0] * e3[1] - e2[1] * e3[0]);
    }
    int32_t c[4];
    const bool rev = (nr[0] * d[0] + nr[1] * d[1]) + nr[2] * d[2] < 0.0;
    for (int q = 0; q < n; ++q) c[q] = idx[rev ? n - 1 - q : q];
    int first = 0;
    for (int q = 1; q < n; ++q) if (c[q] < c[first]) first = q;
    for (int q = 0; q < n; ++q) idx[q] = c[(first + q) % n];
}

// rule 11: the vertex of a crossed edge, a / pa at the inside end, b / pb at the outside end
__host__ __device__ inline void pn_vertex(double a, double b, const double* pa, const double* pb, double iso, double* out) {
    const double t = (iso - a) / (b - a);
    for (int q = 0; q < 3; ++q) out[q] = pa[q] + t * (pb[q] - pa[q]);
}

// rule 11: does the edge (node (ix, iy, iz), type) exist in the grid?
__host__ __device__ inline bool pn_edge_in_grid(int32_t G, int ix, int iy, int iz, int type) {
    const int m = pn_type_mask(type);
    return ix + (m & 1) <= G && iy + (m >> 1 & 1) <= G && iz + (m >> 2 & 1) <= G;
}

#endif
