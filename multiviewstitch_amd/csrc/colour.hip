// colour.hip — mvs_colour_vertices (include/mvs.h): the colour of every vertex of the stitched model from the base images of all
// cameras of all sequences.  The reference has no such stage; the rules C1-C8 are this library's definition, stated in include/mvs.h.
// Their per-(vertex, view) part is colour_rules.h, one body for this kernel and for host code.
//
//   k_colour<LANES>   ONE launch for all vertices and all views.  The camera and SRT tables are staged once per workgroup in LDS.
//                     LANES == 1: a thread per vertex walks every view (col_vertex).  LANES == 16: a row of 16 lanes per vertex, lane j
//                     takes the views j, j + 16, ...; the int64 sums, the count and — under MVS_COLOUR_BEST — the key (Wq, -view) are
//                     reduced over the row with xor shuffles of 8, 4, 2, 1, which never leave a row.  Every sum is an integer, so the
//                     order of the reduction cannot change a byte.  Lane 0 of the row writes the vertex: no atomic anywhere.
// Which mapping a call takes: colour_mapping().
#include "engine.h"
#include "trace.h"
#include "stitch.h"
#include "colour_rules.h"
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

constexpr int TPB = 256;
constexpr int COL_ROW = 16;                       // lanes per vertex of the row mapping: one DPP row
constexpr size_t COL_LDS_MAX = 64 * 1024;         // the tables of a call must fit the LDS one workgroup may ask for
// Below this many vertices (four waves per SIMD for a thread per vertex: 256 CUs x 4 SIMDs x 4 x 64 lanes) the row mapping is taken: it
// has 16 times the threads.  Measured at V = 54 762 (rows win) and V = 2 000 000 (threads win), nowhere between (profiles/r32/colour.md).
constexpr int64_t COL_ROW_BELOW = 262144;

template <int LANES>
__global__ __launch_bounds__(TPB) void k_colour(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t V,
                                                const ColView* __restrict__ gviews, int N, const ColSeq* __restrict__ gseqs, int n_seq,
                                                const uint8_t* __restrict__ imgs, const float* __restrict__ ras, int w, int h, ColRules q,
                                                uint8_t* __restrict__ colours, int32_t* __restrict__ n_views) {
    extern __shared__ double lds[];                                      // ColView[N], then ColSeq[n_seq]: both are whole doubles
    {
        const int nv = N * (int)(sizeof(ColView) / 8), ns = gseqs ? n_seq * (int)(sizeof(ColSeq) / 8) : 0;
        const double* gv = (const double*)gviews;
        const double* gs = (const double*)gseqs;
        for (int k = threadIdx.x; k < nv; k += TPB) lds[k] = gv[k];
        for (int k = threadIdx.x; k < ns; k += TPB) lds[nv + k] = gs[k];
    }
    __syncthreads();
    const ColView* views = (const ColView*)lds;
    const ColSeq* seqs = gseqs ? (const ColSeq*)(lds + N * (sizeof(ColView) / 8)) : nullptr;
    const int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) / LANES;
    const bool live = i < V;                                             // uniform over a row: the shuffles below see whole rows
    if (LANES == 1) {
        if (!live) return;
        uint8_t c[3];
        const int32_t n = col_vertex(ld3(pts + 3 * i), ld3(nrm + 3 * i), views, N, seqs, w, h, imgs, ras, q, c);
        colours[3 * i] = c[0]; colours[3 * i + 1] = c[1]; colours[3 * i + 2] = c[2];
        if (n_views) n_views[i] = n;
        return;
    }
    const int j = threadIdx.x % LANES;
    ColAcc acc = col_acc_zero();
    if (live) {
        const d3 p = ld3(pts + 3 * i), n = ld3(nrm + 3 * i);
        const int64_t npx = (int64_t)w * h;
        d3 pm = p, nm = n;
        int last = -1;
        for (int v = j; v < N; v += LANES) {
            const ColView& cv = views[v];
            if (seqs && cv.seq != last) { col_map(seqs[cv.seq], p, n, &pm, &nm); last = cv.seq; }
            int32_t wq, S[3];
            if (col_view(pm, nm, cv.c, w, h, imgs + 3 * npx * v, ras ? ras + npx * v : nullptr, q, &wq, S)) col_add(acc, q.best, v, wq, S);
        }
    }
    if (q.best) {                                                        // the row's greatest key; its one owner keeps its sums
        long long kmax = acc.key;
#pragma unroll
        for (int o = LANES / 2; o > 0; o >>= 1) {
            const long long other = __shfl_xor(kmax, o, 64);
            kmax = other > kmax ? other : kmax;
        }
        if (acc.key != kmax) { acc.a[0] = acc.a[1] = acc.a[2] = 0; acc.b = 0; }
    }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) {
        acc.a[0] += __shfl_xor((long long)acc.a[0], o, 64);
        acc.a[1] += __shfl_xor((long long)acc.a[1], o, 64);
        acc.a[2] += __shfl_xor((long long)acc.a[2], o, 64);
        acc.b += __shfl_xor((long long)acc.b, o, 64);
        acc.n += __shfl_xor(acc.n, o, 64);
    }
    if (live && j == 0) {
        uint8_t c[3];
        col_result(acc, q, c);
        colours[3 * i] = c[0]; colours[3 * i + 1] = c[1]; colours[3 * i + 2] = c[2];
        if (n_views) n_views[i] = acc.n;
    }
}

// MVS_COLOUR_MAPPING = 1 (a thread per vertex) or 16 (a row per vertex) fixes the mapping of every call, for measurements and tests;
// anything else: by the vertex count
int colour_mapping(int64_t V) {
    const char* e = std::getenv("MVS_COLOUR_MAPPING");
    if (e) {
        const int m = std::atoi(e);
        if (m == 1 || m == COL_ROW) return m;
    }
    return V < COL_ROW_BELOW ? COL_ROW : 1;
}

// what a call is made of, built by the argument checks on the host
struct ColPlan {
    ColRules q;
    int N, w, h;
    std::vector<ColView> views;
    std::vector<ColSeq> seqs;          // empty: the world frame
    size_t lds;
};

int check_colour(const char* fn, const void* points, const void* normals, int64_t V, int32_t n_seq, const double* scales, const double* R,
                 const double* t, const int32_t* cam_off, const mvs_camera* cams, const void* imgs, const mvs_colour_params* prm,
                 const void* colours, ColPlan* pl) {
    int rc;
    mvs_colour_params p;
    if (prm) p = *prm; else mvs_colour_default_params(&p);
    if ((rc = colour_check_params(fn, &p))) return rc;
    if (V < 0 || V >= 0x7fffffffLL) return bad(fn, "need 0 <= V < 2^31 - 1");
    if (!points || !imgs || !colours) return bad(fn, "points, imgs or colours is NULL");
    if (!normals) return bad(fn, "normals is NULL (mvs_mesh_vertex_normals computes them)");
    if ((rc = colour_check_views(fn, n_seq, scales, R, t, cam_off, cams))) return rc;
    pl->q = ColRules{p.min_cos, p.occ_tol, (p.flags & MVS_COLOUR_BEST) ? 1 : 0, {p.fill[0], p.fill[1], p.fill[2]}};
    pl->N = cam_off[n_seq]; pl->w = cams[0].w; pl->h = cams[0].h;
    pl->views.resize((size_t)pl->N);
    for (int k = 0; k < n_seq; ++k)
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) { pl->views[(size_t)c].c = make_camdev(cams + c); pl->views[(size_t)c].seq = k; pl->views[(size_t)c].pad = 0; }
    pl->seqs.clear();
    if (scales)
        for (int k = 0; k < n_seq; ++k) pl->seqs.push_back(col_make_seq(scales[k], R + 9 * k, t + 3 * k));
    pl->lds = sizeof(ColView) * pl->views.size() + sizeof(ColSeq) * pl->seqs.size();
    if (pl->lds > COL_LDS_MAX) return bad(fn, "the camera and SRT tables of the call exceed 64 KiB (chunking the views is not built)");
    return MVS_OK;
}

}  // namespace

int colour_check_params(const char* fn, const mvs_colour_params* p) {
    if (!(p->min_cos > 0.0 && p->min_cos <= 1.0)) return bad(fn, "min_cos must lie in (0, 1]");
    if (!std::isfinite(p->occ_tol) || p->occ_tol <= 0.0) return bad(fn, "occ_tol must be finite and > 0");
    if (p->flags & ~(int32_t)MVS_COLOUR_BEST) return bad(fn, "unknown flag bits");
    if (p->reserved != 0) return bad(fn, "reserved must be 0");
    return MVS_OK;
}

int colour_check_views(const char* fn, int32_t n_seq, const double* scales, const double* R, const double* t, const int32_t* cam_off,
                       const mvs_camera* cams) {
    if (n_seq < 1) return bad(fn, "n_seq must be >= 1");
    if (!cam_off) return bad(fn, "cam_off is NULL");
    if (int rc = check_offsets(fn, "cam_off", cam_off, n_seq)) return rc;
    if (cam_off[n_seq] < 1) return bad(fn, "no cameras");
    if (!cams) return bad(fn, "cams is NULL");
    if (!((scales && R && t) || (!scales && !R && !t))) return bad(fn, "scales, R and t must all be given or all be NULL");
    if (cams[0].w < 2 || cams[0].h < 2) return bad(fn, "every camera needs w, h >= 2");
    if ((int64_t)cams[0].w * cams[0].h > 0x7fffffffLL) return bad(fn, "w * h must not exceed 2^31 - 1");
    for (int c = 1; c < cam_off[n_seq]; ++c)
        if (cams[c].w != cams[0].w || cams[c].h != cams[0].h) return bad(fn, "every camera must have the size of cams[0] (one viewport, as mvs_render_depth_views)");
    return MVS_OK;
}

// checked arguments -> the launch on device arrays, enqueued on s; complete on return
static int colour_launch(const ColPlan& pl, const double* pts, const double* nrm, int64_t V, const uint8_t* imgs, const float* depths,
                         uint8_t* colours, int32_t* n_views, hipStream_t s) {
    Scratch dv, ds;
    int rc;
    if ((rc = up_async(dv, pl.views.data(), pl.views.size(), s)) || (rc = up_async(ds, pl.seqs.data(), pl.seqs.size(), s))) return rc;
    const ColSeq* seqs = pl.seqs.empty() ? nullptr : ds.as<ColSeq>();
    const int n_seq = (int)pl.seqs.size();
    if (colour_mapping(V) == 1) {
        const unsigned nb = (unsigned)((V + TPB - 1) / TPB);
        k_colour<1><<<dim3(nb), dim3(TPB), pl.lds, s>>>(pts, nrm, V, dv.as<ColView>(), pl.N, seqs, n_seq, imgs, depths, pl.w, pl.h, pl.q, colours, n_views);
    } else {
        const unsigned nb = (unsigned)((V * COL_ROW + TPB - 1) / TPB);
        k_colour<COL_ROW><<<dim3(nb), dim3(TPB), pl.lds, s>>>(pts, nrm, V, dv.as<ColView>(), pl.N, seqs, n_seq, imgs, depths, pl.w, pl.h, pl.q, colours,
                                                           n_views);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

int colour_vertices_dev(const char* fn, const double* pts, const double* nrm, int64_t V, int32_t n_seq, const double* scales, const double* R,
                        const double* t, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                        const mvs_colour_params* prm, uint8_t* colours, int32_t* n_views, hipStream_t s) {
    ColPlan pl;
    int rc = check_colour(fn, pts, nrm, V, n_seq, scales, R, t, cam_off, cams, imgs, prm, colours, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (V == 0) return MVS_OK;
    return colour_launch(pl, pts, nrm, V, imgs, depths, colours, n_views, s);
}

extern "C" {

void mvs_colour_default_params(mvs_colour_params* p) {
    if (!p) return;
    p->min_cos = 0.2; p->occ_tol = 0.01; p->flags = 0;
    p->fill[0] = p->fill[1] = p->fill[2] = 128; p->reserved = 0;
}

int mvs_colour_vertices(const double* points, const double* normals, int64_t V, int32_t n_seq, const double* scales, const double* R,
                        const double* t, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                        const mvs_colour_params* prm, uint8_t* colours, int32_t* n_views) {
    MVS_TRACE();
    ColPlan pl;
    int rc = check_colour(__func__, points, normals, V, n_seq, scales, R, t, cam_off, cams, imgs, prm, colours, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (V == 0) return MVS_OK;
    const size_t npx = (size_t)pl.N * (size_t)pl.w * (size_t)pl.h;
    Scratch dp, dn, di, dd, dc, dk;
    if ((rc = up(dp, points, 3 * (size_t)V)) || (rc = up(dn, normals, 3 * (size_t)V)) || (rc = up(di, imgs, 3 * npx)) ||
        (depths && (rc = up(dd, depths, npx))) || (rc = dc.alloc(3 * (size_t)V)) || (n_views && (rc = dk.alloc(sizeof(int32_t) * (size_t)V)))) return rc;
    if ((rc = colour_launch(pl, dp.as<double>(), dn.as<double>(), V, di.as<uint8_t>(), depths ? dd.as<float>() : nullptr, dc.as<uint8_t>(),
                            n_views ? dk.as<int32_t>() : nullptr, nullptr))) return rc;
    if ((rc = down(colours, dc, 3 * (size_t)V))) return rc;
    return n_views ? down(n_views, dk, (size_t)V) : MVS_OK;
}

int mvs_colour_vertices_dev(const double* points_dev, const double* normals_dev, int64_t V, int32_t n_seq, const double* scales, const double* R,
                            const double* t, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev, const float* depths_dev,
                            const mvs_colour_params* prm, uint8_t* colours_dev, int32_t* n_views_dev, void* hip_stream) {
    MVS_TRACE();
    return colour_vertices_dev(__func__, points_dev, normals_dev, V, n_seq, scales, R, t, cam_off, cams, imgs_dev, depths_dev, prm, colours_dev,
                               n_views_dev, (hipStream_t)hip_stream);
}

}  // extern "C"
