// depth_recover_rules.h — the per-pixel rules of mvs_recover_depth_maps (include/mvs.h): the candidate test (R3), the levels (R4), the
// cost of one level (R5), the choice of the best and the worst level (R6), the acceptance (R7), the substep (R8) and the value (R9).
// One body for the kernel of depth_recover.hip and for host code: tests/depth_recover_rules.cpp runs it as a program of its own,
// tests/ref_depth_recover.py restates it operation for operation.  Every floating-point operation is an fp64 + - * / sqrt in the order
// written (the library is built with -ffp-contract=off); every sum of squared grey differences is an exact integer.
#ifndef MVS_DEPTH_RECOVER_RULES_H_
#define MVS_DEPTH_RECOVER_RULES_H_
#include "depth_refine_rules.h"
#include <cstring>

constexpr int RC_NONE = -1;            // level_out of a pixel without an accepted level

struct RcRules {                       // mvs_depth_recover_params as the body reads it
    double mn, mx, err, peak;
    int32_t N, refs, L, min_refs, flags;
};

struct RcPixel {                       // what R3-R9 decide for one pixel
    float out;                         // +0.0f unless accepted
    int32_t level, sum, cnt;           // level_out (RC_NONE unless accepted), sum_out and cnt_out (-1 and 0 without an eligible level)
};

// R4
__host__ __device__ inline double rc_level(double mn, double mx, int l, int L, double step) { return l < L - 1 ? mn + (double)l * step : mx; }

// R6: does (sum, cnt) have a smaller mean than (bsum, bcnt)?  The levels are walked upwards, so on equality the earlier one stays, as
// the best and as the worst
__host__ __device__ inline bool rc_less(int32_t sum, int32_t cnt, int32_t bsum, int32_t bcnt) { return (int64_t)sum * bcnt < (int64_t)bsum * cnt; }

// R9: (float)d, moved by one float32 into [mn, mx] when the rounding left it.  d > 0, so the neighbours are the neighbouring bit patterns.
__host__ __device__ inline float rc_value(double d, double mn, double mx) {
    float out = (float)d;
    uint32_t bits;
    memcpy(&bits, &out, sizeof bits);
    if ((double)out < mn) ++bits;
    else if ((double)out > mx) --bits;
    memcpy(&out, &bits, sizeof bits);
    return out;
}

// R3-R9 for pixel (u, v) of frame f of a sequence of n frames: cameras cams[n]; ssd(g, u', v') is R5's sum for the window of frame g at
// (u', v'), an interior pixel, against the window of frame f at (u, v) — any exact evaluation.  The levels are walked once in ascending
// l: the best so far, the one before it, the one after it and the worst so far are all R6-R8 need.  A reference remembers the pixel its
// last level landed on: with many levels several consecutive ones land there, and the sum is the same.
template <class Ssd>
__host__ __device__ inline RcPixel rc_pixel(const CamDev* __restrict__ cams, int n, int f, int u, int v, const RcRules& q, const Ssd& ssd) {
    RcPixel r = {0.0f, RC_NONE, -1, 0};
    const CamDev& c = cams[f];
    const int w = c.w, h = c.h, N = q.N, L = q.L;
    if (!dr_interior(u, v, w, h, N)) return r;                                                // R3
    const double step = (q.mx - q.mn) / (double)(L - 1);                                      // R4
    const int g0 = f - q.refs / 2;                                                            // R2
    int32_t lu[DR_MAX_REFS + 1], lv[DR_MAX_REFS + 1], ls[DR_MAX_REFS + 1];
#pragma unroll
    for (int i = 0; i <= DR_MAX_REFS; ++i) { lu[i] = lv[i] = -1; ls[i] = 0; }                 // no interior pixel has a negative coordinate
    bool have = false, pending = false;
    int bl = 0;
    int32_t bsum = 0, bcnt = 0, wsum = 0, wcnt = 0, msum = 0, mcnt = 0, psum = 0, pcnt = 0, prev_sum = 0, prev_cnt = 0;
    for (int l = 0; l < L; ++l) {
        const double dl = rc_level(q.mn, q.mx, l, L, step);
        const d3 P = world_from_img_hd(c, u, v, 1.0 / dl);
        int32_t sum = 0, cnt = 0;
#pragma unroll
        for (int i = 0; i <= DR_MAX_REFS; ++i) {                                              // R5
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
        if (cnt < q.min_refs) cnt = 0;                                                        // R6: not eligible
        if (pending) { psum = sum; pcnt = cnt; pending = false; }                             // l - 1 is the best so far: this is its l + 1
        if (cnt > 0) {
            if (!have || rc_less(sum, cnt, bsum, bcnt)) {
                bl = l; bsum = sum; bcnt = cnt;
                msum = prev_sum; mcnt = prev_cnt;                                             // cnt 0: l - 1 is below 0 or not eligible
                psum = 0; pcnt = 0; pending = true;
            }
            if (!have || rc_less(wsum, wcnt, sum, cnt)) { wsum = sum; wcnt = cnt; }
            have = true;
        }
        prev_sum = sum; prev_cnt = cnt;
    }
    if (!have) return r;
    r.sum = bsum; r.cnt = bcnt;
    const int len = 2 * N + 1;
    const double m = (double)bsum / (double)bcnt, mw = (double)wsum / (double)wcnt;
    if (!(sqrt(m / (double)(len * len)) <= q.err) || !(m < q.peak * mw)) return r;            // R7
    r.level = bl;
    double d = rc_level(q.mn, q.mx, bl, L, step);
    if ((q.flags & 1) && mcnt > 0 && pcnt > 0) {                                              // R8
        const double cm = (double)msum / (double)mcnt, cp = (double)psum / (double)pcnt;
        const double den = (cm - 2.0 * m) + cp;
        if (den > 0.0) {
            const double o = 0.5 * ((cm - cp) / den);
            const double ds = q.mn + ((double)bl + o) * step;
            if (dr_in_bounds(ds, q.mn, q.mx)) d = ds;
        }
    }
    r.out = rc_value(d, q.mn, q.mx);                                                          // R9
    return r;
}

#endif
