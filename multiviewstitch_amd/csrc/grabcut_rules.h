// grabcut_rules.h — the per-pixel and per-component rules of mvs_grabcut_masks (include/mvs.h): the half pixel (1), the rectangle (2),
// the luma component (4), the fit of a component from its integer sums (5), the score of a pixel under a component (6), beta (7), an
// n-link (8), the t-link (9) and the footprint of a full-size pixel (12).  One body for the kernels of grabcut.hip and for host code:
// tests/grabcut_rules.cpp runs it as a program of its own, tests/ref_grabcut.py restates it operation for operation.  Apart from exp
// and log every operation is an integer one or an fp64 + - * / in the order written; the library is built with -ffp-contract=off.
#ifndef MVS_GRABCUT_RULES_H_
#define MVS_GRABCUT_RULES_H_
#include <stdint.h>
#include <float.h>
#include <math.h>

constexpr int GC_K = 5;               // components per model
constexpr int GC_SUMS = 10;           // int64 per component: c | s0 s1 s2 | p00 p01 p02 p11 p12 p22
constexpr int GC_LUMA = 766;          // bins of the luma histogram

struct GcRect { int32_t x0, y0, x1, y1; };                    // [x0, x1) x [y0, y1) of the half image
struct GcComp {                                               // a fitted component; used == 0: empty, skipped everywhere
    double lw, mean[3], inv[9];                               // lw = log(weight) - 0.5 log(det); inv row-major, inv[3 * r + c] = i_rc
    double det, weight;
    int32_t used, pad;
};

// a colour as one word: c0 | c1 << 8 | c2 << 16
__host__ __device__ inline int gc_ch(uint32_t px, int a) { return (int)((px >> (8 * a)) & 255u); }

// rule 1: half pixel (x, y) of a w-wide image
__host__ __device__ inline uint32_t gc_half_px(const uint8_t* __restrict__ img, int w, int x, int y) {
    const uint8_t* a = img + ((int64_t)(2 * y) * w + 2 * x) * 3;
    const uint8_t* c = a + (int64_t)w * 3;
    uint32_t px = 0;
    for (int k = 0; k < 3; ++k) px |= (uint32_t)((a[k] + a[3 + k] + c[k] + c[3 + k] + 2) >> 2) << (8 * k);
    return px;
}

// rule 2
__host__ __device__ inline GcRect gc_rect(int hw, int hh, double hl, double hr, double vl, double vr) {
    const int rowL = (int)((double)hh * vl), colL = (int)((double)hw * hl), rowR = (int)((double)hh * vr), colR = (int)((double)hw * hr);
    return GcRect{colL, rowL, hw - colR, hh - rowR};
}
__host__ __device__ inline bool gc_inside(const GcRect& r, int x, int y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }

__host__ __device__ inline int gc_luma(uint32_t px) { return gc_ch(px, 0) + gc_ch(px, 1) + gc_ch(px, 2); }

// rule 4: the thresholds of a model from its histogram (m pixels), and the component of a luma
__host__ __device__ inline void gc_thresholds(const int32_t* __restrict__ hist, int64_t m, int32_t t[4]) {
    int64_t cum = 0;
    int k = 1;
    for (int l = 0; l < GC_LUMA && k <= 4; ++l) {
        cum += hist[l];
        while (k <= 4 && cum >= (k * m + 4) / 5) t[k++ - 1] = l;
    }
    while (k <= 4) t[k++ - 1] = GC_LUMA - 1;                  // m == 0
}
__host__ __device__ inline int gc_luma_component(int luma, const int32_t t[4]) {
    return (t[0] < luma) + (t[1] < luma) + (t[2] < luma) + (t[3] < luma);
}

// rule 5: a component from its sums; m = the pixels of its model
__host__ __device__ inline void gc_fit(const int64_t* __restrict__ s, int64_t m, GcComp* o) {
    *o = GcComp{};
    const int64_t cnt = s[0];
    if (cnt <= 0) return;
    const double n = (double)cnt;
    double c[3][3];
    for (int a = 0; a < 3; ++a) o->mean[a] = (double)s[1 + a] / n;
    const int at[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) c[a][b] = (double)s[at[a][b]] / n - o->mean[a] * o->mean[b];
    double det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) +
                 c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]);
    if (det <= DBL_EPSILON) {
        c[0][0] += 0.01; c[1][1] += 0.01; c[2][2] += 0.01;
        det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) +
              c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]);
    }
    o->inv[0] =  (c[1][1] * c[2][2] - c[1][2] * c[2][1]) / det;
    o->inv[3] = -(c[1][0] * c[2][2] - c[1][2] * c[2][0]) / det;
    o->inv[6] =  (c[1][0] * c[2][1] - c[1][1] * c[2][0]) / det;
    o->inv[1] = -(c[0][1] * c[2][2] - c[0][2] * c[2][1]) / det;
    o->inv[4] =  (c[0][0] * c[2][2] - c[0][2] * c[2][0]) / det;
    o->inv[7] = -(c[0][0] * c[2][1] - c[0][1] * c[2][0]) / det;
    o->inv[2] =  (c[0][1] * c[1][2] - c[0][2] * c[1][1]) / det;
    o->inv[5] = -(c[0][0] * c[1][2] - c[0][2] * c[1][0]) / det;
    o->inv[8] =  (c[0][0] * c[1][1] - c[0][1] * c[1][0]) / det;
    o->det = det;
    o->weight = n / (double)m;
    o->lw = log(o->weight) - 0.5 * log(det);
    o->used = 1;
}

// rule 6: a_k of a pixel under a (non-empty) component
__host__ __device__ inline double gc_score(const GcComp& g, uint32_t px) {
    const double d0 = (double)gc_ch(px, 0) - g.mean[0], d1 = (double)gc_ch(px, 1) - g.mean[1], d2 = (double)gc_ch(px, 2) - g.mean[2];
    const double q = d0 * (d0 * g.inv[0] + d1 * g.inv[3] + d2 * g.inv[6]) + d1 * (d0 * g.inv[1] + d1 * g.inv[4] + d2 * g.inv[7]) +
                     d2 * (d0 * g.inv[2] + d1 * g.inv[5] + d2 * g.inv[8]);
    return g.lw - 0.5 * q;
}
// the component of a pixel in its model (0 for a model without a component)
__host__ __device__ inline int gc_assign(const GcComp* __restrict__ m, uint32_t px) {
    int best = 0;
    double ab = 0.0;
    bool have = false;
    for (int k = 0; k < GC_K; ++k) {
        if (!m[k].used) continue;
        const double a = gc_score(m[k], px);
        if (!have || a > ab) { ab = a; best = k; have = true; }
    }
    return best;
}

// rule 9: L of a pixel under a model
__host__ __device__ inline double gc_L(const GcComp* __restrict__ m, uint32_t px, double gamma) {
    double a[GC_K], mx = 0.0;
    int n = 0;
    for (int k = 0; k < GC_K; ++k) {
        if (!m[k].used) continue;
        a[n] = gc_score(m[k], px);
        if (n == 0 || a[n] > mx) mx = a[n];
        ++n;
    }
    if (n == 0) return 9.0 * gamma;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) sum += exp(a[k] - mx);
    return -(mx + log(sum));
}
__host__ __device__ inline int32_t gc_tlink_max(double gamma) { return (int32_t)llrint(1024.0 * 9.0 * gamma); }
__host__ __device__ inline int32_t gc_excess(const GcComp* __restrict__ fg, const GcComp* __restrict__ bg, uint32_t px, double gamma, bool inside) {
    const int32_t K = gc_tlink_max(gamma);
    if (!inside) return -K;
    const double v = 1024.0 * (gc_L(bg, px, gamma) - gc_L(fg, px, gamma));
    if (!(v < (double)K)) return K;                                              // a NaN cannot arise: both L are finite
    if (v <= -(double)K) return -K;
    return (int32_t)llrint(v);
}

// rules 7 and 8
__host__ __device__ inline int gc_d2(uint32_t p, uint32_t q) {
    const int a = gc_ch(p, 0) - gc_ch(q, 0), b = gc_ch(p, 1) - gc_ch(q, 1), c = gc_ch(p, 2) - gc_ch(q, 2);
    return a * a + b * b + c * c;
}
__host__ __device__ inline int64_t gc_pairs(int hw, int hh) { return 4 * (int64_t)hw * hh - 3 * (int64_t)hw - 3 * (int64_t)hh + 2; }
__host__ __device__ inline double gc_beta(int64_t S, int hw, int hh) {
    if (S == 0) return 0.0;
    return 1.0 / (2.0 * ((double)S / (double)gc_pairs(hw, hh)));
}
__host__ __device__ inline int32_t gc_ncap(double beta, double gamma, int d2, bool diagonal) {
    const double g = diagonal ? gamma / sqrt(2.0) : gamma;
    return (int32_t)llrint(1024.0 * g * exp(-beta * (double)d2));
}

// rule 12: the full-size pixel (x, y) from the half mask (non-zero = foreground)
__host__ __device__ inline int gc_foot0(int x) { return (x & 1) ? (x - 1) / 2 : x / 2 - 1; }
__host__ __device__ inline int gc_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__host__ __device__ inline uint8_t gc_full_px(const uint8_t* __restrict__ half, int hw, int hh, int x, int y) {
    const int x0 = gc_foot0(x), y0 = gc_foot0(y);
    const int xa = gc_clampi(x0, hw - 1), xb = gc_clampi(x0 + 1, hw - 1), ya = gc_clampi(y0, hh - 1), yb = gc_clampi(y0 + 1, hh - 1);
    const bool f = half[(int64_t)ya * hw + xa] | half[(int64_t)ya * hw + xb] | half[(int64_t)yb * hw + xa] | half[(int64_t)yb * hw + xb];
    return f ? 255 : 0;
}

#endif
