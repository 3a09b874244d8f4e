// depth_refine_rules.h — the per-pixel rules of mvs_refine_depth_maps (include/mvs.h): the reference frames (2), the candidate test
// (3), the hypotheses (4), the cost of one hypothesis (5), the choice (6), the acceptance (7) and the substep (8).  One body for the
// kernel of depth_refine.hip and for host code: tests/depth_refine_rules.cpp runs it as a program of its own,
// tests/ref_depth_refine.py restates it operation for operation.  Every floating-point operation is an fp64 + - * / sqrt in the order
// written (the library is built with -ffp-contract=off); every sum of squared grey differences is an exact integer.
#ifndef MVS_DEPTH_REFINE_RULES_H_
#define MVS_DEPTH_REFINE_RULES_H_
#include "camera_dev.h"
#include "frontend_dev.h"

constexpr int DR_MAX_REFS = 8;         // ref_frm_count <= 9, and the current frame is not a reference
constexpr int DR_NONE = -128;          // k_out of a pixel that keeps its input

struct DrRules {                       // mvs_depth_refine_params as the body reads it
    double mn, mx, rel, err;
    int32_t N, refs, K, flags;
};

struct DrPixel {                       // what rules 3-8 decide for one pixel
    bool accepted;                     // out = (float)d; otherwise the input float, bit for bit
    double d;
    int32_t k, sum, cnt;               // k_out (DR_NONE unless accepted), sum_out and cnt_out (-1 and 0 without an eligible hypothesis)
};

__host__ __device__ inline bool dr_in_bounds(double d, double mn, double mx) { return d >= mn && d <= mx; }   // a NaN is not
__host__ __device__ inline bool dr_interior(int u, int v, int w, int h, int N) { return u >= N && u < w - N && v >= N && v < h - N; }
// rule 4
__host__ __device__ inline double dr_hypothesis(double d0, int k, double step) { return d0 * (1.0 + (double)k * step); }

// rule 5 for one reference in its plain form: the exact sum over the window of (cur(a, b) - G_g[v' + a][u' + b])^2; cur(a, b) =
// G_f[v + a][u + b].  ssd(g, u', v') of dr_pixel for host code: the grey rasters of a sequence (n of w x h bytes, back to back)
template <class Cur>
struct DrPlainSsd {
    Cur cur;
    const uint8_t* grey;
    int w, h, N;
    __host__ __device__ int32_t operator()(int g, int u2, int v2) const {
        const uint8_t* gg = grey + (int64_t)g * w * h;
        int32_t s = 0;
        for (int a = -N; a <= N; ++a) {
            const uint8_t* row = gg + (int64_t)(v2 + a) * w + u2;
            for (int b = -N; b <= N; ++b) {
                const int df = cur(a, b) - (int)row[b];
                s += df * df;
            }
        }
        return s;
    }
};

// rule 6: does (sum, cnt) of k beat (bsum, bcnt) of j?  k runs upwards, so k > j: on equality k wins only when |k| < |j|
__host__ __device__ inline bool dr_beats(int32_t sum, int32_t cnt, int k, int32_t bsum, int32_t bcnt, int j) {
    const int64_t l = (int64_t)sum * bcnt, r = (int64_t)bsum * cnt;
    if (l != r) return l < r;
    return (k < 0 ? -k : k) < (j < 0 ? -j : j);
}

// Rules 3-8 for pixel (u, v) of frame f of a sequence of n frames: cameras cams[n], d0f the pixel's input float; ssd(g, u', v') is
// rule 5's sum for the window of frame g at (u', v'), an interior pixel, against the window of frame f at (u, v) — any exact evaluation.
// The hypotheses are walked once in ascending k: the best so far, the one before it and the one after it are all the substep needs.
// A reference remembers the pixel its last hypothesis landed on: the next hypothesis that lands there has the same sum.
template <class Ssd>
__host__ __device__ inline DrPixel dr_pixel(const CamDev* __restrict__ cams, int n, int f, int u, int v, float d0f, const DrRules& q, const Ssd& ssd) {
    DrPixel r = {false, 0.0, DR_NONE, -1, 0};
    const CamDev& c = cams[f];
    const int w = c.w, h = c.h, N = q.N, K = q.K;
    const double d0 = (double)d0f;
    if (!dr_in_bounds(d0, q.mn, q.mx) || !dr_interior(u, v, w, h, N)) return r;              // rule 3
    const double step = q.rel / (double)K;
    const int g0 = f - q.refs / 2;                                                            // rule 2
    int32_t lu[DR_MAX_REFS + 1], lv[DR_MAX_REFS + 1], ls[DR_MAX_REFS + 1];
#pragma unroll
    for (int i = 0; i <= DR_MAX_REFS; ++i) { lu[i] = lv[i] = -1; ls[i] = 0; }                 // no interior pixel has a negative coordinate
    bool have = false, pending = false;
    int bk = 0;
    int32_t bsum = 0, bcnt = 0, msum = 0, mcnt = 0, psum = 0, pcnt = 0, prev_sum = 0, prev_cnt = 0;
    for (int k = -K; k <= K; ++k) {
        const double dk = dr_hypothesis(d0, k, step);
        int32_t sum = 0, cnt = 0;
        if (dr_in_bounds(dk, q.mn, q.mx)) {                                                   // live
            const d3 P = world_from_img_hd(c, u, v, 1.0 / dk);
#pragma unroll
            for (int i = 0; i <= DR_MAX_REFS; ++i) {
                const int g = g0 + i;
                if (i < q.refs && g >= 0 && g < n && g != f) {
                    const d3 xc = cam_from_world(cams[g], P);
                    int32_t u2, v2;
                    if (xc.z > 0.0) {
                        img_from_cam(cams[g], xc, &u2, &v2);
                        if (dr_interior(u2, v2, w, h, N)) {
                            if (u2 != lu[i] || v2 != lv[i]) {
                                ls[i] = ssd(g, u2, v2);
                                lu[i] = u2; lv[i] = v2;
                            }
                            sum += ls[i];
                            ++cnt;
                        }
                    }
                }
            }
        }
        if (pending) { psum = sum; pcnt = cnt; pending = false; }                             // k - 1 is the best so far: this is its k + 1
        if (cnt > 0 && (!have || dr_beats(sum, cnt, k, bsum, bcnt, bk))) {                    // rule 6
            have = true; bk = k; bsum = sum; bcnt = cnt;
            msum = prev_sum; mcnt = prev_cnt;                                                 // cnt 0: k - 1 is below -K or not eligible
            psum = 0; pcnt = 0; pending = true;
        }
        prev_sum = sum; prev_cnt = cnt;
    }
    if (!have) return r;
    r.sum = bsum; r.cnt = bcnt;
    const int len = 2 * N + 1;
    const double m = (double)bsum / (double)bcnt;
    if (!(sqrt(m / (double)(len * len)) <= q.err)) return r;                                  // rule 7
    r.accepted = true;
    r.k = bk;
    r.d = dr_hypothesis(d0, bk, step);
    if ((q.flags & 1) && mcnt > 0 && pcnt > 0) {                                              // rule 8
        const double cm = (double)msum / (double)mcnt, cp = (double)psum / (double)pcnt;
        const double den = (cm - 2.0 * m) + cp;
        if (den > 0.0) {
            const double o = 0.5 * ((cm - cp) / den);
            const double d = d0 * (1.0 + ((double)bk + o) * step);
            if (dr_in_bounds(d, q.mn, q.mx)) r.d = d;
        }
    }
    return r;
}

#endif
