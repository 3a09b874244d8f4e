// colour_rules.h — the per-(vertex, view) rules of mvs_colour_vertices (include/mvs.h): the map into the sequence's frame (C1), the
// projection (C2), the facing test (C3), the occlusion test against the view's raster (C4), the bilinear sample in integers (C5), the
// weight (C6), the accumulation (C7) and the result (C8).  One body for the kernels of colour.hip and for host code:
// tests/colour_rules.cpp runs it as a program of its own, tests/ref_colour.py restates it operation for operation.  Every
// floating-point operation is an fp64 + - * / sqrt in the order written; the library is built with -ffp-contract=off.
#ifndef MVS_COLOUR_RULES_H_
#define MVS_COLOUR_RULES_H_
#include "camera_dev.h"

struct ColRules {                      // mvs_colour_params as the body reads it
    double min_cos, occ_tol;
    int32_t best;                      // MVS_COLOUR_BEST
    uint8_t fill[3];
};

// the inverse similarity map of one sequence as mvs_srt_apply(inverse = 1) builds it: M = (1 / s) * R^T element by element, Rn = R^T
struct ColSeq { double M[9], Rn[9], t[3]; };
struct ColView { CamDev c; int32_t seq, pad; };

__host__ __device__ inline ColSeq col_make_seq(double sc, const double* R, const double* t) {
    ColSeq m;
    const double Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
    const double inv = 1.0 / sc;
    for (int i = 0; i < 9; ++i) { m.M[i] = inv * Rt[i]; m.Rn[i] = Rt[i]; }
    for (int i = 0; i < 3; ++i) m.t[i] = t[i];
    return m;
}

// C1: the vertex and its normal in the sequence's frame
__host__ __device__ inline void col_map(const ColSeq& m, d3 p, d3 n, d3* pm, d3* nm) {
    *pm = mulMv(m.M, p - mk3(m.t[0], m.t[1], m.t[2]));
    *nm = mulMv(m.Rn, n);
}

// What the views of a vertex (or of one lane's share of them) add up to.  Blend: a, b are the sums of C7.  BEST: a, b hold the one
// view of greatest key = (Wq, lowest view index).  n counts the accepted views either way.
struct ColAcc {
    int64_t a[3], b, key;
    int32_t n;
};
__host__ __device__ inline ColAcc col_acc_zero() {
    ColAcc r;
    r.a[0] = r.a[1] = r.a[2] = 0; r.b = 0; r.key = -1; r.n = 0;
    return r;
}
__host__ __device__ inline int64_t col_key(int32_t wq, int32_t view) { return ((int64_t)wq << 32) | (int64_t)(0x7fffffff - view); }

// C2-C6 for a mapped vertex and one view: false when a rule rejects the view; else Wq and the three channel sums S.  img is the
// view's image (h x w x 3), ras its raster (h x w) or NULL.
__host__ __device__ inline bool col_view(d3 pm, d3 nm, const CamDev& c, int w, int h, const uint8_t* __restrict__ img,
                                         const float* __restrict__ ras, const ColRules& q, int32_t* wq, int32_t* S) {
    const d3 pc = cam_from_world(c, pm);                                                       // C2
    if (!(pc.z > 0.0)) return false;
    const double x = c.fx * pc.x / pc.z + c.cx, y = c.fy * pc.y / pc.z + c.cy;
    if (!(x >= 0.0 && x <= (double)(w - 1) && y >= 0.0 && y <= (double)(h - 1))) return false;
    const d3 m = mulMv(c.R, nm);                                                               // C3
    const double dot = -((m.x * pc.x + m.y * pc.y) + m.z * pc.z);
    const double cs = dot / sqrt(((m.x * m.x + m.y * m.y) + m.z * m.z) * ((pc.x * pc.x + pc.y * pc.y) + pc.z * pc.z));
    if (!(cs >= q.min_cos)) return false;
    if (ras) {                                                                                 // C4
        const int32_t u = cvt_i32(x + 0.5), v = cvt_i32(y + 0.5);
        const double d = (double)ras[(int64_t)v * w + u];
        if (!(d > 0.0 && fabs(pc.z * d - 1.0) <= q.occ_tol)) return false;
    }
    int32_t x0 = cvt_i32(x), y0 = cvt_i32(y);                                                  // C5
    if (x0 > w - 2) x0 = w - 2;
    if (y0 > h - 2) y0 = h - 2;
    const int32_t ax = cvt_i32((x - (double)x0) * 256.0 + 0.5), ay = cvt_i32((y - (double)y0) * 256.0 + 0.5);
    const uint8_t* r0 = img + ((int64_t)y0 * w + x0) * 3;
    const uint8_t* r1 = r0 + (int64_t)w * 3;
    const int32_t w00 = (256 - ax) * (256 - ay), w10 = ax * (256 - ay), w01 = (256 - ax) * ay, w11 = ax * ay;
    for (int ch = 0; ch < 3; ++ch) S[ch] = w00 * r0[ch] + w10 * r0[3 + ch] + w01 * r1[ch] + w11 * r1[3 + ch];
    const int32_t k = cvt_i32(cs * cs * 4096.0 + 0.5);                                         // C6
    *wq = k < 1 ? 1 : k;
    return true;
}

// C7 for one accepted view
__host__ __device__ inline void col_add(ColAcc& acc, int best, int32_t view, int32_t wq, const int32_t* S) {
    ++acc.n;
    if (!best) {
        for (int ch = 0; ch < 3; ++ch) acc.a[ch] += (int64_t)wq * S[ch];
        acc.b += wq;
        return;
    }
    const int64_t key = col_key(wq, view);
    if (key > acc.key) {
        acc.key = key;
        for (int ch = 0; ch < 3; ++ch) acc.a[ch] = (int64_t)wq * S[ch];
        acc.b = wq;
    }
}

// C8
__host__ __device__ inline void col_result(const ColAcc& acc, const ColRules& q, uint8_t* colour) {
    for (int ch = 0; ch < 3; ++ch) colour[ch] = acc.n ? (uint8_t)((acc.a[ch] + 32768 * acc.b) / (65536 * acc.b)) : q.fill[ch];
}

// C1-C8 for one vertex over all views in camera order: the body of the thread-per-vertex mapping and of host code.  seqs == NULL:
// the world frame.  imgs / ras: all views back to back
__host__ __device__ inline int32_t col_vertex(d3 p, d3 n, const ColView* __restrict__ views, int N, const ColSeq* __restrict__ seqs, int w, int h,
                                              const uint8_t* __restrict__ imgs, const float* __restrict__ ras, const ColRules& q, uint8_t* colour) {
    ColAcc acc = col_acc_zero();
    const int64_t npx = (int64_t)w * h;
    d3 pm = p, nm = n;
    int last = -1;
    for (int v = 0; v < N; ++v) {
        const ColView& cv = views[v];
        if (seqs && cv.seq != last) { col_map(seqs[cv.seq], p, n, &pm, &nm); last = cv.seq; }
        int32_t wq, S[3];
        if (col_view(pm, nm, cv.c, w, h, imgs + 3 * npx * v, ras ? ras + npx * v : nullptr, q, &wq, S)) col_add(acc, q.best, v, wq, S);
    }
    col_result(acc, q, colour);
    return acc.n;
}

#endif
