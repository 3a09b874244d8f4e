// srt_refine_rules.h — the per-match rules of mvs_srt_refine (include/mvs.h, I1-I6) in one host/device body: the maps of a sequence
// (I1), the relative map a query takes into its target's frame (I3), the acceptance of a match (I4), its residual and 14-vector (I5)
// and the 121 quantised terms (I6).  srt_refine.hip runs it on the device; tests/srt_refine_rules.cpp compiles it with the host
// compiler alone, under the sanitizers.  Every expression is the literal sequence of IEEE operations (the library is built with
// -ffp-contract=off), so that tests/ref_srt_refine.py can restate them operation for operation.
#ifndef MVS_SRT_REFINE_RULES_H_
#define MVS_SRT_REFINE_RULES_H_
#include "dev_common.h"

#define SRR_TERMS 121        /* count | J_i J_j, i <= j, row by row (105) | J_i r (14) | r r */
#define SRR_JJ 1
#define SRR_JR 106
#define SRR_RR 120

struct SrrMap { double M[9], R[9], t[3]; };        // y = M p + t with M = s * R element by element; normals turn by R

__host__ __device__ inline SrrMap srr_map(double s, const double* R, const double* t) {
    SrrMap m;
    for (int i = 0; i < 9; ++i) { m.M[i] = s * R[i]; m.R[i] = R[i]; }
    m.t[0] = t[0]; m.t[1] = t[1]; m.t[2] = t[2];
    return m;
}
__host__ __device__ inline d3 srr_apply(const SrrMap& m, d3 p) { return mulMv(m.M, p) + mk3(m.t[0], m.t[1], m.t[2]); }

// the map of sequence a's points into sequence b's OWN frame: mvs_srt_relative(b, a), operation for operation (api_geom.cpp)
__host__ __device__ inline SrrMap srr_relative(double sb, const double* Rb, const double* tb, double sa, const double* Ra, const double* ta) {
    const double Rt[9] = {Rb[0], Rb[3], Rb[6], Rb[1], Rb[4], Rb[7], Rb[2], Rb[5], Rb[8]};
    const double s = 1.0 / sb * sa;
    double R[9], M[9], t[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (Rt[3 * i] * Ra[j] + Rt[3 * i + 1] * Ra[3 + j]) + Rt[3 * i + 2] * Ra[6 + j];
    const double inv = 1.0 / sb;
    for (int i = 0; i < 9; ++i) M[i] = inv * Rt[i];
    const d3 tt = mulMv(M, mk3(ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]));
    t[0] = tt.x; t[1] = tt.y; t[2] = tt.z;
    return srr_map(s, R, t);
}

// I1: a point takes part iff its coordinates are finite and stay finite as float32
__host__ __device__ inline bool srr_coord_ok(double v) { return v - v == 0.0 && fabs(v) <= 3.4028234663852886e38; }
__host__ __device__ inline bool srr_usable(d3 p) { return srr_coord_ok(p.x) && srr_coord_ok(p.y) && srr_coord_ok(p.z); }
// I1: n / |n|; false for a normal that is not finite or has no length (|n|^2 zero or not finite)
__host__ __device__ inline bool srr_unit(d3 n, d3* u) {
    const double l2 = sqn3(n);
    if (!(l2 > 0.0) || !(l2 - l2 == 0.0)) return false;
    *u = n / sqrt(l2);
    return true;
}

struct SrrFrame { double c[3], D, cap2, min_cos; };     // I2 and the two thresholds of I4 (cap2 = (2 rel_dist)^2)

__host__ __device__ inline d3 srr_normalised(const SrrMap& m, d3 p, const SrrFrame& f) {
    return (srr_apply(m, p) - mk3(f.c[0], f.c[1], f.c[2])) / f.D;
}
__host__ __device__ inline long long srr_quant(double v) { return llrint(v * 68719476736.0); }            // q of I6: 2^36
__host__ __device__ inline double srr_dequant(long long s) { return (double)s * (1.0 / 68719476736.0); }

// I4 and I5 for the query (pa, na) of sequence a and its nearest point (pb, nb) of sequence b, both in their own frames: false when
// the match is rejected, else r and J
__host__ __device__ inline bool srr_match(const SrrMap& A, const SrrMap& B, const SrrFrame& f, d3 pa, d3 na, d3 pb, d3 nb, double* r, double* J) {
    d3 ua, ub;
    if (!srr_unit(na, &ua) || !srr_unit(nb, &ub)) return false;
    const d3 xa = srr_normalised(A, pa, f), xb = srr_normalised(B, pb, f);
    const d3 d = xa - xb;
    if (!(sqn3(d) <= f.cap2)) return false;
    const d3 n = mulMv(B.R, ub);
    if (!(dot3(mulMv(A.R, ua), n) >= f.min_cos)) return false;
    *r = dot3(n, d);
    const d3 ca = cross3(xa, n), cb = cross3(xb, n);
    J[0] = ca.x; J[1] = ca.y; J[2] = ca.z; J[3] = n.x; J[4] = n.y; J[5] = n.z; J[6] = dot3(n, xa);
    J[7] = -cb.x; J[8] = -cb.y; J[9] = -cb.z; J[10] = -n.x; J[11] = -n.y; J[12] = -n.z; J[13] = -dot3(n, xb);
    return true;
}

// I6: the 121 terms of an accepted match in slot order, emit(slot, term); fully unrolled, so J stays in registers on the device
template <class F>
__host__ __device__ inline void srr_terms(double r, const double* J, F&& emit) {
    emit(0, 1LL);
    int k = SRR_JJ;
#pragma unroll
    for (int i = 0; i < 14; ++i)
#pragma unroll
        for (int j = i; j < 14; ++j) emit(k++, srr_quant(J[i] * J[j]));
#pragma unroll
    for (int i = 0; i < 14; ++i) emit(SRR_JR + i, srr_quant(J[i] * r));
    emit(SRR_RR, srr_quant(r * r));
}

#endif
