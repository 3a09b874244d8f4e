// stitch.hip — the tail of Processor::AlignmentSeq (R/Processor/Processor.cpp:952-1105) and Mesh::CalculateVertexNormals for a
// general mesh (R/PlyObj/PlyObj.cpp:3-16,139-185).
//
//   k_vis_cull      : the visibility cull of :966-1004 (each sequence's points, before Poisson) and of :1064-1105 (AllSeqProj, the
//                     Poisson model): a point stays iff, for every sequence k0 and every camera c of k0, the point mapped into k0's
//                     frame projects inside c's image (GetImgCoordFromWorld + CheckRange, R/Common/Utils.h:20-22).  One thread per
//                     point, one launch for every segment of a call (blockIdx.y = segment); the map of (segment, k0) and the
//                     cameras are read with wave-uniform indices (scalar loads).  The result is an AND of pure tests, so a wave
//                     stops at the first camera that none of its lanes passes; the mask equals the reference's loop, not its order.
//   k_stitch_compact: the in-place compaction of :969-1003 written out of place with the reference's layout (the kept points in
//                     order, then the untouched originals at [n_keep, P_k): the vectors are never resized, :1022) or truncated.
//   k_vn_*          : vertex normals of a triangle list: unit facet normals (tri_normal_plyobj), the vertex -> facet incidence
//                     built with integer atomics, each vertex's slice sorted to ascending facet order, then summed in that order.
#include "engine.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include "stitch.h"
#include <algorithm>

namespace {

constexpr int TPB = 256;

// the map of (segment, k0): identity (a sequence's own points before Poisson, p3d_ = p3d at :973-983), else the similarity map
struct CullMap { Map34 m; int32_t identity; int32_t pad; };

// a wave-uniform read of a table the kernel never writes, through the constant address space: the backend then always selects
// scalar loads (through the generic pointer it chose vector loads inside the camera loop)
template <class T>
__device__ inline T load_uniform(const T* p) {
    typedef const __attribute__((address_space(4))) T* cptr;
    const cptr q = (cptr)p;
    T r;
    const __attribute__((address_space(4))) uint32_t* src = (const __attribute__((address_space(4))) uint32_t*)q;
    uint32_t* dst = (uint32_t*)&r;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); ++i) dst[i] = src[i];
    return r;
}

template <class T>
__global__ __launch_bounds__(TPB) void k_vis_cull(const double* __restrict__ pts, const int64_t* __restrict__ seg_off, int n_seq,
                                                  const CullMap* __restrict__ maps, const int32_t* __restrict__ cam_off,
                                                  const CamDev* __restrict__ cams, T* __restrict__ keep,
                                                  unsigned long long* __restrict__ n_keep) {
    const int seg = blockIdx.y;
    const int64_t b = seg_off[seg], e = seg_off[seg + 1];
    const int lane = threadIdx.x & 63;
    const CullMap* __restrict__ row = maps + (int64_t)seg * n_seq;
    // wave-uniform trip count: every lane of a wave runs the loop (the ballot below needs all of them)
    for (int64_t i0 = b + (int64_t)blockIdx.x * TPB + (threadIdx.x & ~63); i0 < e; i0 += (int64_t)gridDim.x * TPB) {
        const int64_t i = i0 + lane;
        const bool active = i < e;
        bool in = active;
        const d3 p = active ? ld3(pts + 3 * i) : mk3(0, 0, 0);
        for (int k0 = 0; k0 < n_seq && __any(in); ++k0) {
            const d3 q = row[k0].identity ? p : map34_point(row[k0].m, p);
            const int c1 = cam_off[k0 + 1];
            for (int c = cam_off[k0]; c < c1 && __any(in); ++c) {
                // (a lane already out computes along unmasked)
                const CamDev cam = load_uniform(cams + c);
                int32_t u, v;
                img_from_world(cam, q, &u, &v);                           // GetImgCoordFromWorld, Camera.cpp:45-48,68-72
                in = in && in_range(u, v, cam.w, cam.h);
            }
        }
        if (active) keep[i] = (T)(in ? 1 : 0);
        const unsigned long long kept = __ballot(in);
        if (lane == 0 && kept) atomicAdd(n_keep + seg, (unsigned long long)__popcll(kept));
    }
}

// one sequence's compaction (:969-1003) from the exclusive scan of the keep mask over all segments: kept point i goes to
// out_base + (pos[i] - pos[b]); with `tail`, every i whose offset in the segment is >= n_keep also lands on its own offset (the
// originals the in-place loop never overwrote)
__global__ void k_stitch_compact(const double* __restrict__ pts, const double* __restrict__ nrm, const int32_t* __restrict__ keep,
                                 const int32_t* __restrict__ pos, int64_t b, int64_t n, int64_t n_keep, int tail, int64_t out_base,
                                 double* __restrict__ out_pts, double* __restrict__ out_nrm) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t i = b + j;
    const d3 p = ld3(pts + 3 * i), q = ld3(nrm + 3 * i);
    if (keep[i]) {
        const int64_t o = out_base + (pos[i] - pos[b]);
        st3(out_pts + 3 * o, p);
        st3(out_nrm + 3 * o, q);
    }
    if (tail && j >= n_keep) {
        st3(out_pts + 3 * (out_base + j), p);
        st3(out_nrm + 3 * (out_base + j), q);
    }
}

// ------------------------------------------------------------ vertex normals ----
// CalculateFacetNormals (:157-170) + the sizes of AdjacentFacetsPerVertex; a facet with an index outside [0, V) raises *bad and
// takes no part (the count and the fill skip the same facets)
__global__ void k_vn_facets(const double* __restrict__ pts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                            double* __restrict__ fn, int32_t* __restrict__ cnt, int32_t* __restrict__ bad) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) { atomicOr(bad, 1); return; }
    st3(fn + 3 * f, tri_normal_plyobj(ld3(pts + 3 * (int64_t)a), ld3(pts + 3 * (int64_t)b), ld3(pts + 3 * (int64_t)c)));
    atomicAdd(cnt + a, 1);
    atomicAdd(cnt + b, 1);
    atomicAdd(cnt + c, 1);
}

// the incidence lists in arbitrary order (a facet that lists a vertex twice appears twice in its list)
__global__ void k_vn_fill(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ start,
                          int32_t* __restrict__ fill, int32_t* __restrict__ list) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) return;
    for (int j = 0; j < 3; ++j) {
        const int32_t v = faces[3 * f + j];
        list[start[v] + atomicAdd(fill + v, 1)] = (int32_t)f;
    }
}

__device__ inline void sift_down(int32_t* a, int root, int n) {
    while (true) {
        int c = 2 * root + 1;
        if (c >= n) return;
        if (c + 1 < n && a[c + 1] > a[c]) ++c;
        if (a[root] >= a[c]) return;
        const int32_t t = a[root]; a[root] = a[c]; a[c] = t;
        root = c;
    }
}
// ascending facet order within one slice: insertion sort for the usual few entries, heap sort (n log n) for a hub
__device__ inline void sort_slice(int32_t* a, int n) {
    if (n <= 32) {
        for (int i = 1; i < n; ++i) {
            const int32_t x = a[i];
            int j = i - 1;
            while (j >= 0 && a[j] > x) { a[j + 1] = a[j]; --j; }
            a[j + 1] = x;
        }
        return;
    }
    for (int r = n / 2 - 1; r >= 0; --r) sift_down(a, r, n);
    for (int end = n - 1; end > 0; --end) {
        const int32_t t = a[0]; a[0] = a[end]; a[end] = t;
        sift_down(a, 0, end);
    }
}

// CalculateVertexNormals (:139-156): meanNormal summed over the adjacent facets in facet order, / size, normalize()
__global__ void k_vn_vertex(const int32_t* __restrict__ start, int32_t* __restrict__ list, const double* __restrict__ fn, int64_t V,
                            double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int32_t s0 = start[v], n = start[v + 1] - s0;
    sort_slice(list + s0, n);
    d3 sum = mk3(0, 0, 0);
    for (int j = 0; j < n; ++j) sum = sum + ld3(fn + 3 * (int64_t)list[s0 + j]);
    const d3 m = sum / (double)n;                                         // (no facet: 0/0 -> NaN, as the reference)
    st3(out + 3 * v, m / norm3(m));
}

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + TPB - 1) / TPB)); }

}  // namespace

// ------------------------------------------------------------------ launchers ----
int vis_cull_dev(const double* pts_dev, const int64_t* seg_off, int n_seg, int n_seq, const double* scales, const double* R,
                 const double* t, const int32_t* cam_off, const mvs_camera* cams, int mode, uint8_t* keep_u8, int32_t* keep_i32,
                 int64_t* n_keep, hipStream_t s) {
    const int64_t P = seg_off[n_seg] - seg_off[0];
    const int n_cams = cam_off[n_seq];
    std::vector<CullMap> maps((size_t)n_seg * n_seq);
    for (int g = 0; g < n_seg; ++g)
        for (int k0 = 0; k0 < n_seq; ++k0) {
            CullMap& m = maps[(size_t)g * n_seq + k0];
            m.identity = 0; m.pad = 0;
            if (mode == MVS_CULL_SEQUENCES) {
                if (k0 == g) { m.identity = 1; m.m = Map34(); continue; }                                     // :973-974: no map at all
                double sr, Rr[9], tr[3];                                                                   // :979-982
                mvs_srt_relative(scales[k0], R + 9 * k0, t + 3 * k0, scales[g], R + 9 * g, t + 3 * g, &sr, Rr, tr);
                m.m = make_map34(sr, Rr, tr, 0);
            } else {
                m.m = make_map34(scales[k0], R + 9 * k0, t + 3 * k0, 1);                                   // :1069
            }
        }
    std::vector<CamDev> cd;
    Scratch dseg, dmaps, doff, dcams, dcnt;
    int rc;
    if ((rc = up_async(dseg, seg_off, (size_t)n_seg + 1, s)) || (rc = up_async(dmaps, maps.data(), maps.size(), s)) ||
        (rc = up_async(doff, cam_off, (size_t)n_seq + 1, s)) || (rc = up_cams(dcams, cd, cams, (size_t)n_cams, s)) ||
        (rc = dcnt.alloc(sizeof(unsigned long long) * n_seg, s))) return rc;
    HIPCHK(hipMemsetAsync(dcnt.p, 0, sizeof(unsigned long long) * n_seg, s));
    int64_t maxn = 0;
    for (int g = 0; g < n_seg; ++g) maxn = std::max(maxn, seg_off[g + 1] - seg_off[g]);
    if (P > 0) {
        // enough waves to fill the device (256 CUs x 8 blocks) spread over the segments; each block strides over its segment
        const int64_t per_seg = std::max<int64_t>(1, std::min<int64_t>((maxn + TPB - 1) / TPB, std::max<int64_t>(1, 2048 / n_seg)));
        const dim3 grid((unsigned)per_seg, (unsigned)n_seg);
        if (keep_i32) k_vis_cull<int32_t><<<grid, dim3(TPB), 0, s>>>(pts_dev, dseg.as<int64_t>(), n_seq, dmaps.as<CullMap>(), doff.as<int32_t>(),
                                                                      dcams.as<CamDev>(), keep_i32, dcnt.as<unsigned long long>());
        else k_vis_cull<uint8_t><<<grid, dim3(TPB), 0, s>>>(pts_dev, dseg.as<int64_t>(), n_seq, dmaps.as<CullMap>(), doff.as<int32_t>(),
                                                             dcams.as<CamDev>(), keep_u8, dcnt.as<unsigned long long>());
        HIPCHK(hipGetLastError());
    }
    std::vector<unsigned long long> cnt(n_seg);
    HIPCHK(hipMemcpyAsync(cnt.data(), dcnt.p, sizeof(unsigned long long) * n_seg, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int g = 0; g < n_seg; ++g) n_keep[g] = (int64_t)cnt[g];
    return MVS_OK;
}

int stitch_compact_dev(const double* pts, const double* nrm, const int32_t* keep, const int64_t* seg_off, int n_seg, const int64_t* n_keep,
                       int truncate, const double* scales, const double* R, const double* t, double* out_pts, double* out_nrm,
                       int64_t* out_off, hipStream_t s) {
    const int64_t P = seg_off[n_seg];
    Scratch pos, tp, tn;
    int rc;
    if ((rc = pos.alloc(sizeof(int32_t) * (P + 1), s))) return rc;
    if ((rc = scan_exclusive_i32(keep, P, pos.as<int32_t>(), s))) return rc;
    out_off[0] = 0;
    for (int g = 0; g < n_seg; ++g) out_off[g + 1] = out_off[g] + (truncate ? n_keep[g] : seg_off[g + 1] - seg_off[g]);
    const int64_t Q = out_off[n_seg];
    if ((rc = tp.alloc(sizeof(double) * 3 * Q, s)) || (rc = tn.alloc(sizeof(double) * 3 * Q, s))) return rc;
    for (int g = 0; g < n_seg; ++g) {
        const int64_t n = seg_off[g + 1] - seg_off[g];
        if (n > 0)
            k_stitch_compact<<<blocks_of(n), dim3(TPB), 0, s>>>(pts, nrm, keep, pos.as<int32_t>(), seg_off[g], n, n_keep[g], !truncate,
                                                                 out_off[g], tp.as<double>(), tn.as<double>());
    }
    for (int g = 0; g < n_seg; ++g) {                                     // vpts / vnorm, :1021-1027
        const int64_t o = out_off[g], m = out_off[g + 1] - o;
        launch_srt_apply(tp.as<double>() + 3 * o, tn.as<double>() + 3 * o, m, scales[g], R + 9 * g, t + 3 * g, 0, out_pts + 3 * o,
                         out_nrm + 3 * o, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

int mesh_vertex_normals_dev(const double* pts, int64_t V, const int32_t* faces, int64_t F, double* out, hipStream_t s) {
    if (V <= 0) return MVS_OK;
    Scratch cnt, start, fill, list, fn, bad;
    int rc;
    const int64_t F1 = std::max<int64_t>(F, 1);
    if ((rc = cnt.alloc(sizeof(int32_t) * V, s)) || (rc = start.alloc(sizeof(int32_t) * (V + 1), s)) ||
        (rc = fill.alloc(sizeof(int32_t) * V, s)) || (rc = list.alloc(sizeof(int32_t) * 3 * F1, s)) ||
        (rc = fn.alloc(sizeof(double) * 3 * F1, s)) || (rc = bad.alloc(sizeof(int32_t), s))) return rc;
    HIPCHK(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * V, s));
    HIPCHK(hipMemsetAsync(fill.p, 0, sizeof(int32_t) * V, s));
    HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(int32_t), s));
    if (F > 0) k_vn_facets<<<blocks_of(F), dim3(TPB), 0, s>>>(pts, V, faces, F, fn.as<double>(), cnt.as<int32_t>(), bad.as<int32_t>());
    if ((rc = scan_exclusive_i32(cnt.as<int32_t>(), V, start.as<int32_t>(), s))) return rc;
    int32_t hbad = 0;
    HIPCHK(hipMemcpyAsync(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hbad) { mvs_set_error("mvs_mesh_vertex_normals: a facet index is outside [0, %lld)", (long long)V); return MVS_E_BAD_MESH; }
    if (F > 0) k_vn_fill<<<blocks_of(F), dim3(TPB), 0, s>>>(faces, F, V, start.as<int32_t>(), fill.as<int32_t>(), list.as<int32_t>());
    k_vn_vertex<<<blocks_of(V), dim3(TPB), 0, s>>>(start.as<int32_t>(), list.as<int32_t>(), fn.as<double>(), V, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_stitch() { return (const void*)k_vis_cull<uint8_t>; }
