// mesh_trim.hip — mvs_mesh_trim_by_value (include/mvs.h, rule 18): the faces of any triangle mesh whose three vertices pass the test of
// poisson_rules.h against a per-vertex value, and the vertices those faces use, both in their order, the faces renumbered.  The density
// calls of poisson.hip supply such a value (rule 17); nothing else is shared with them.
//   k_tr_face_mark     flags the kept faces, counts them per workgroup and marks their vertices as referenced with plain byte stores of 1
//                      (ref was cleared; every store writes the same value)
//   k_tr_vertex_count  counts the referenced vertices per workgroup; compact.hip's tail (CompactTail) scans the two count arrays
//   k_tr_vertex_scatter / k_tr_face_scatter
//                      write the survivors in their order, the faces through the new numbers of their vertices
#include "engine.h"
#include "trace.h"
#include "frontend_dev.h"
#include "poisson_rules.h"
#include "stitch.h"
#include <cmath>

namespace {

__device__ inline bool tr_face_kept(int64_t V, const int32_t* __restrict__ faces, const double* __restrict__ values, double thr, int64_t f, int64_t F,
                                    uint8_t* bad) {
    if (f >= F) return false;
    bool keep = true;
    for (int q = 0; q < 3; ++q) {
        const int32_t v = faces[3 * f + q];
        if (v < 0 || v >= V) { *bad = 1; return false; }
        keep = keep && pn_trim_pass(values[v], thr);
    }
    return keep;
}

__global__ __launch_bounds__(COMPACT_TPB) void k_tr_face_mark(int64_t V, int64_t F, const int32_t* __restrict__ faces, const double* __restrict__ values,
                                                              double thr, uint8_t* __restrict__ keepf, uint8_t* __restrict__ ref, uint8_t* __restrict__ bad,
                                                              int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[COMPACT_TPB / 64];
    const int64_t f = (int64_t)blockIdx.x * COMPACT_TPB + threadIdx.x;
    const bool keep = tr_face_kept(V, faces, values, thr, f, F, bad);
    if (f < F) keepf[f] = keep ? 1 : 0;
    if (keep)
        for (int q = 0; q < 3; ++q) ref[faces[3 * f + q]] = 1;
    const WgRank k = wg_rank<COMPACT_TPB / 64>(keep, s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

__global__ __launch_bounds__(COMPACT_TPB) void k_tr_vertex_count(int64_t V, const uint8_t* __restrict__ ref, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[COMPACT_TPB / 64];
    const int64_t v = (int64_t)blockIdx.x * COMPACT_TPB + threadIdx.x;
    const WgRank k = wg_rank<COMPACT_TPB / 64>(v < V && ref[v], s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

__global__ __launch_bounds__(COMPACT_TPB) void k_tr_vertex_scatter(int64_t V, const uint8_t* __restrict__ ref, const int32_t* __restrict__ base,
                                                                   const double* __restrict__ vertices, const double* __restrict__ normals,
                                                                   double* __restrict__ vertices_out, double* __restrict__ normals_out,
                                                                   int32_t* __restrict__ renum) {
    __shared__ int s_wsum[COMPACT_TPB / 64];
    const int64_t v = (int64_t)blockIdx.x * COMPACT_TPB + threadIdx.x;
    const bool keep = v < V && ref[v];
    const int64_t pos = (int64_t)base[blockIdx.x] + wg_rank<COMPACT_TPB / 64>(keep, s_wsum).rank;
    if (!keep) return;
    renum[v] = (int32_t)pos;
    for (int a = 0; a < 3; ++a) vertices_out[3 * pos + a] = vertices[3 * v + a];
    if (normals)
        for (int a = 0; a < 3; ++a) normals_out[3 * pos + a] = normals[3 * v + a];
}

__global__ __launch_bounds__(COMPACT_TPB) void k_tr_face_scatter(int64_t F, const uint8_t* __restrict__ keepf, const int32_t* __restrict__ base,
                                                                 const int32_t* __restrict__ faces, const int32_t* __restrict__ renum,
                                                                 int32_t* __restrict__ faces_out) {
    __shared__ int s_wsum[COMPACT_TPB / 64];
    const int64_t f = (int64_t)blockIdx.x * COMPACT_TPB + threadIdx.x;
    const bool keep = f < F && keepf[f];
    const int64_t pos = (int64_t)base[blockIdx.x] + wg_rank<COMPACT_TPB / 64>(keep, s_wsum).rank;
    if (!keep) return;
    for (int q = 0; q < 3; ++q) faces_out[3 * pos + q] = renum[faces[3 * f + q]];       // a kept face: its vertices are referenced, renum is set
}

int check_trim(const char* fn, int64_t V, const void* vertices, const void* normals, int64_t F, const void* faces, const void* values, double thr,
               const void* vertices_out, const void* normals_out, const void* faces_out, const void* V_out, const void* F_out) {
    if (!vertices || !faces || !values || !vertices_out || !faces_out || !V_out || !F_out) return bad(fn, "an argument other than normals / normals_out is NULL");
    if (normals && !normals_out) return bad(fn, "normals without normals_out");
    if (V < 0 || F < 0) return bad(fn, "V or F is negative");
    if (V > 0x7fffffffLL || F > 0x7fffffffLL) return bad(fn, "V or F exceeds 2^31 - 1");
    if (std::isnan(thr)) return bad(fn, "threshold is NaN");
    return MVS_OK;
}

}  // namespace

// rule 18 on device arrays, arguments validated by the caller.  Synchronises s.
int mesh_trim_dev(int64_t V, const double* vertices, const double* normals, int64_t F, const int32_t* faces, const double* values, double thr,
                  double* vertices_out, double* normals_out, int32_t* faces_out, int64_t* V_out, int64_t* F_out, hipStream_t s) {
    *V_out = *F_out = 0;
    if (V == 0 || F == 0) return MVS_OK;
    int rc;
    const int64_t nbv = (V + COMPACT_TPB - 1) / COMPACT_TPB, nbf = (F + COMPACT_TPB - 1) / COMPACT_TPB;
    Scratch keepf, ref, renum;                                               // ref: V bytes and the bad-mesh byte behind them
    CompactTail tv, tf;
    if ((rc = keepf.alloc((size_t)F, s)) || (rc = ref.alloc((size_t)V + 1, s)) || (rc = renum.alloc(4 * (size_t)V, s)) ||
        (rc = tv.alloc((size_t)nbv, 1, s)) || (rc = tf.alloc((size_t)nbf, 1, s))) return rc;
    HIPCHK(hipMemsetAsync(ref.p, 0, (size_t)V + 1, s));
    k_tr_face_mark<<<dim3((unsigned)nbf), dim3(COMPACT_TPB), 0, s>>>(V, F, faces, values, thr, keepf.as<uint8_t>(), ref.as<uint8_t>(), ref.as<uint8_t>() + V,
                                                                    tf.cnt.as<int32_t>());
    k_tr_vertex_count<<<dim3((unsigned)nbv), dim3(COMPACT_TPB), 0, s>>>(V, ref.as<uint8_t>(), tv.cnt.as<int32_t>());
    tf.strided((int)nbf, nullptr, 1, (int)nbf, s);                            // off = {0, all survivors}
    tv.strided((int)nbv, nullptr, 1, (int)nbv, s);
    HIPCHK(hipGetLastError());
    uint8_t badmesh = 0;
    int64_t offv[2] = {0, 0}, offf[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&badmesh, ref.as<uint8_t>() + V, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(offv, tv.off.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(offf, tf.off.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (badmesh) { mvs_set_error("mesh trim: a face index is outside [0, V)"); return MVS_E_BAD_MESH; }
    if (offf[1] > 0) {
        k_tr_vertex_scatter<<<dim3((unsigned)nbv), dim3(COMPACT_TPB), 0, s>>>(V, ref.as<uint8_t>(), tv.base.as<int32_t>(), vertices, normals, vertices_out,
                                                                             normals_out, renum.as<int32_t>());
        k_tr_face_scatter<<<dim3((unsigned)nbf), dim3(COMPACT_TPB), 0, s>>>(F, keepf.as<uint8_t>(), tf.base.as<int32_t>(), faces, renum.as<int32_t>(),
                                                                           faces_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
    }
    *V_out = offv[1];
    *F_out = offf[1];
    return MVS_OK;
}

extern "C" {

int mvs_mesh_trim_by_value_dev(int64_t V, const double* vertices_dev, const double* normals_dev, int64_t F, const int32_t* faces_dev,
                               const double* values_dev, double threshold, double* vertices_out_dev, double* normals_out_dev,
                               int32_t* faces_out_dev, int64_t* V_out, int64_t* F_out, void* hip_stream) {
    MVS_TRACE();
    int rc = check_trim(__func__, V, vertices_dev, normals_dev, F, faces_dev, values_dev, threshold, vertices_out_dev, normals_out_dev, faces_out_dev,
                        V_out, F_out);
    if (rc || (rc = need_device())) return rc;
    return mesh_trim_dev(V, vertices_dev, normals_dev, F, faces_dev, values_dev, threshold, vertices_out_dev, normals_out_dev, faces_out_dev, V_out,
                         F_out, (hipStream_t)hip_stream);
}

int mvs_mesh_trim_by_value(int64_t V, const double* vertices, const double* normals, int64_t F, const int32_t* faces, const double* values,
                           double threshold, double* vertices_out, double* normals_out, int32_t* faces_out, int64_t* V_out, int64_t* F_out) {
    MVS_TRACE();
    int rc = check_trim(__func__, V, vertices, normals, F, faces, values, threshold, vertices_out, normals_out, faces_out, V_out, F_out);
    if (rc || (rc = need_device())) return rc;
    Scratch dv, dn, df, dval, ov, on, of;
    if ((rc = up(dv, vertices, 3 * (size_t)V)) || (rc = up(df, faces, 3 * (size_t)F)) || (rc = up(dval, values, (size_t)V)) ||
        (normals && (rc = up(dn, normals, 3 * (size_t)V))) || (rc = ov.alloc(24 * (size_t)V)) || (rc = of.alloc(12 * (size_t)F)) ||
        (normals && (rc = on.alloc(24 * (size_t)V)))) return rc;
    if ((rc = mesh_trim_dev(V, dv.as<double>(), normals ? dn.as<double>() : nullptr, F, df.as<int32_t>(), dval.as<double>(), threshold, ov.as<double>(),
                            normals ? on.as<double>() : nullptr, of.as<int32_t>(), V_out, F_out, nullptr))) return rc;
    if ((rc = down(vertices_out, ov, 3 * (size_t)*V_out)) || (normals && (rc = down(normals_out, on, 3 * (size_t)*V_out)))) return rc;
    return down(faces_out, of, 3 * (size_t)*F_out);
}

}  // extern "C"
