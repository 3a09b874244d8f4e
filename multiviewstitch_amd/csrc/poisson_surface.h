// poisson_surface.h — the extraction of rules 10-12 (and 30-31 on the band's finest level), stated once over a surface view S:
//   k_pn_cubemask<S>       rule 10: the inside bits of a cube's eight corners, one byte per cube item; 0 for a cube that takes no part
//   k_pn_edge_count<S> / k_pn_vertex_scatter<S>, k_pn_face_count (poisson.hip) / k_pn_face_scatter<S>
//                          rules 11-12: two ordered compactions (wg_rank per workgroup of 256 items, PnScan between count and scatter).
//                          The edge flags stay behind as a bitmap, 64 flags per word: a face finds the number of a vertex as
//                          base[workgroup] + popcounts, no edge map is stored.
// Edge item r = node item * 7 + type, face item r = (cube item * 6 + tetrahedron) * 2 + slot.  A view holds g, chi and iso and answers
// what differs between the dense grid (PnDenseSurf, here) and the stored blocks of a band level (BdSurf, poisson_band.hip):
//   node_items(), cube_items()    how many items of each kind there are
//   node(item, i) -> place        the node of a node item and where its value lies in chi
//   cube(item, i)                 the lower corner of a cube item
//   takes_part(i)                 does the cube at i have faces at all?
//   slot(ix, iy, iz), has(place)  where the value of a node lies; has: the node is stored (a missing node compares as outside)
//   place(ix, iy, iz)             the node item of a node
//   edge(i, type, &open)          does the edge exist?  open: rule 31, counted into n_open when S::counts_open (a compile-time
//                                 property: a view without it pays neither the ballot nor the atomic)
#ifndef MVS_POISSON_SURFACE_H_
#define MVS_POISSON_SURFACE_H_
#ifdef __HIPCC__
#include "frontend_dev.h"
#include "poisson_dev.h"

struct PnDenseSurf {                     // every node of a grid of g.G cells in node order; cube item = (cz * G + cy) * G + cx
    static constexpr bool counts_open = false;
    PnGrid g;
    const double* chi;
    double iso;
    __host__ __device__ int64_t node_items() const { return (int64_t)(g.G + 1) * (g.G + 1) * (g.G + 1); }
    __host__ __device__ int64_t cube_items() const { return (int64_t)g.G * g.G * g.G; }
    __device__ int64_t node(int64_t item, int i[3]) const {
        const int n1 = g.G + 1;
        i[0] = (int)(item % n1); i[1] = (int)(item / n1 % n1); i[2] = (int)(item / ((int64_t)n1 * n1));
        return item;
    }
    __device__ void cube(int64_t item, int i[3]) const {
        i[0] = (int)(item % g.G); i[1] = (int)(item / g.G % g.G); i[2] = (int)(item / ((int64_t)g.G * g.G));
    }
    __device__ bool takes_part(const int*) const { return true; }
    __device__ int64_t slot(int ix, int iy, int iz) const { return pn_node(g.G, ix, iy, iz); }
    __device__ bool has(int64_t) const { return true; }
    __device__ int64_t place(int ix, int iy, int iz) const { return pn_node(g.G, ix, iy, iz); }
    __device__ bool edge(const int i[3], int type, bool* open) const {
        *open = false;
        return pn_edge_in_grid(g.G, i[0], i[1], i[2], type);
    }
};

template <class S>
__global__ __launch_bounds__(PN_TPB) void k_pn_cubemask(S q, uint8_t* __restrict__ mask) {
    const int64_t cube = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    if (cube >= q.cube_items()) return;
    int i0[3], m = 0;
    q.cube(cube, i0);
    if (q.takes_part(i0))
        for (int c = 0; c < 8; ++c) {
            const int64_t at = q.slot(i0[0] + (c & 1), i0[1] + (c >> 1 & 1), i0[2] + (c >> 2 & 1));
            m |= (q.has(at) && q.chi[at] < q.iso ? 1 : 0) << c;
        }
    mask[cube] = (uint8_t)m;
}

// edge item r: a crossed edge that exists?
template <class S>
__device__ inline bool pn_edge_crossed(const S& q, int64_t r, int64_t items, bool* open) {
    *open = false;
    if (r >= items) return false;
    const int type = (int)(r % 7);
    int i[3];
    const int64_t at = q.node(r / 7, i);
    if (!q.edge(i, type, open)) { *open = false; return false; }
    const int m = pn_type_mask(type);
    const int64_t hi = q.slot(i[0] + (m & 1), i[1] + (m >> 1 & 1), i[2] + (m >> 2 & 1));
    const bool f = q.has(hi) && (q.chi[at] < q.iso) != (q.chi[hi] < q.iso);
    *open = *open && f;
    return f;
}

template <class S>
__global__ __launch_bounds__(PN_TPB) void k_pn_edge_count(S q, int64_t items, unsigned long long* __restrict__ words, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t r = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    bool open;
    const bool f = pn_edge_crossed(q, r, items, &open);
    const unsigned long long bal = __ballot(f);
    if ((threadIdx.x & 63) == 0) words[r >> 6] = bal;
    if constexpr (S::counts_open) {
        const unsigned long long obal = __ballot(open);
        if ((threadIdx.x & 63) == 0 && obal) atomicAdd(q.n_open, (unsigned long long)__popcll(obal));     // integers: any order
    }
    const WgRank k = wg_rank<PN_WAVES>(f, s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

template <class S>
__global__ __launch_bounds__(PN_TPB) void k_pn_vertex_scatter(S q, int64_t items, const unsigned long long* __restrict__ words,
                                                              const int32_t* __restrict__ base, double* __restrict__ vertices) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t r = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const bool f = (words[r >> 6] >> (r & 63)) & 1ull;                       // the bitmap covers whole workgroups
    const int64_t pos = (int64_t)base[blockIdx.x] + wg_rank<PN_WAVES>(f, s_wsum).rank;
    if (!f) return;
    const int m = pn_type_mask((int)(r % 7));
    int i[3];
    const int64_t at = q.node(r / 7, i);
    const int jx = i[0] + (m & 1), jy = i[1] + (m >> 1 & 1), jz = i[2] + (m >> 2 & 1);
    const double vl = q.chi[at], vh = q.chi[q.slot(jx, jy, jz)];
    double pl[3], ph[3], out[3];
    pn_node_pos(q.g, i[0], i[1], i[2], pl);
    pn_node_pos(q.g, jx, jy, jz, ph);
    if (vl < q.iso) pn_vertex(vl, vh, pl, ph, q.iso, out); else pn_vertex(vh, vl, ph, pl, q.iso, out);
    for (int a = 0; a < 3; ++a) vertices[3 * pos + a] = out[a];
}

template <class S>
__global__ __launch_bounds__(PN_TPB) void k_pn_face_scatter(S q, const uint8_t* __restrict__ mask, int64_t items,
                                                            const unsigned long long* __restrict__ words, const int32_t* __restrict__ vbase,
                                                            const double* __restrict__ vertices, const int32_t* __restrict__ fbase,
                                                            int32_t* __restrict__ faces) {
    __shared__ int s_wsum[PN_WAVES];
    const int64_t r = (int64_t)blockIdx.x * PN_TPB + threadIdx.x;
    const int in = pn_face_item(mask, r, items);
    const int64_t pos = (int64_t)fbase[blockIdx.x] + wg_rank<PN_WAVES>(in >= 0, s_wsum).rank;
    if (in < 0) return;
    const int k = (int)(r % 12) >> 1, slot = (int)(r & 1);
    int i0[3];
    q.cube(r / 12, i0);
    int ci[4], co[4];
    const int n = pn_tet_cycle(in, ci, co);
    int32_t idx[4];
    double pos3[4][3], d[3];
    for (int e = 0; e < n; ++e) {
        int nm, type;
        pn_tet_edge(k, ci[e], co[e], &nm, &type);
        idx[e] = pn_vertex_index(words, vbase, q.place(i0[0] + (nm & 1), i0[1] + (nm >> 1 & 1), i0[2] + (nm >> 2 & 1)) * 7 + type);
        for (int a = 0; a < 3; ++a) pos3[e][a] = vertices[3 * (int64_t)idx[e] + a];
    }
    pn_tet_dir(k, in, d);
    pn_polygon(n, idx, pos3, d);
    faces[3 * pos] = idx[0];
    faces[3 * pos + 1] = idx[slot ? 2 : 1];
    faces[3 * pos + 2] = idx[slot ? 3 : 2];
}

#endif
#endif
