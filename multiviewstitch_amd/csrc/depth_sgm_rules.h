// depth_sgm_rules.h — the per-pixel rules of mvs_recover_depth_maps_aggregated (include/mvs.h, S1-S6): the raw (sum, cnt) of one level
// (R5, stated a second time so that rc_pixel of depth_recover_rules.h stays as it is), the quantised capped cost (S1), one level of the
// path recurrence (S2), the winner (S3) and the acceptance, substep and value (S4-S6).  One body for the kernels of depth_sgm.hip and for
// host code: tests/depth_sgm_rules.cpp runs it as a program of its own (sg_frame), tests/ref_depth_sgm.py restates the rules on whole
// arrays.  The costs and every path value are integers; the only fp64 operations are those of R4, R5, R7, R8 and R9, in the order written.
#ifndef MVS_DEPTH_SGM_RULES_H_
#define MVS_DEPTH_SGM_RULES_H_
#include "depth_recover_rules.h"

constexpr int32_t SG_FAR = 1 << 20;    // a level that does not take part: above every L_r + p1 (<= 8190 + 4095)

struct SgRules {                       // mvs_depth_aggregate_params as the body reads it
    int32_t p1, p2, cap, paths;
};

struct SgPixel {                       // what S3-S6 decide for one pixel of the rectangle
    RcPixel r;
    int32_t agg;
};

// R5 and the eligibility of R6 for level l: the landing pixels of the level walked before are remembered per reference, as rc_pixel does
struct SgLand {
    int32_t lu[DR_MAX_REFS + 1], lv[DR_MAX_REFS + 1], ls[DR_MAX_REFS + 1];
    __host__ __device__ SgLand() {
#pragma unroll
        for (int i = 0; i <= DR_MAX_REFS; ++i) { lu[i] = lv[i] = -1; ls[i] = 0; }
    }
};

// -> the raw sum and cnt of level l; cnt is 0 when fewer than min_refs references count (not eligible)
template <class Ssd>
__host__ __device__ inline void sg_level(const CamDev* __restrict__ cams, int n, int f, int u, int v, const RcRules& q, double step, int l, const Ssd& ssd,
                                         SgLand& a, int32_t* sum_out, int32_t* cnt_out) {
    const CamDev& c = cams[f];
    const int w = c.w, h = c.h, N = q.N;
    const int g0 = f - q.refs / 2;                                                            // R2
    const double dl = rc_level(q.mn, q.mx, l, q.L, step);
    const d3 P = world_from_img_hd(c, u, v, 1.0 / dl);
    int32_t sum = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i <= DR_MAX_REFS; ++i) {                                                  // R5
        const int g = g0 + i;
        if (i < q.refs && g >= 0 && g < n && g != f) {
            const d3 xc = cam_from_world(cams[g], P);
            int32_t u2, v2;
            if (xc.z > 0.0) {
                img_from_cam(cams[g], xc, &u2, &v2);
                if (dr_interior(u2, v2, w, h, N)) {
                    if (u2 != a.lu[i] || v2 != a.lv[i]) {
                        a.ls[i] = ssd(g, u2, v2);
                        a.lu[i] = u2; a.lv[i] = v2;
                    }
                    sum += a.ls[i];
                    ++cnt;
                }
            }
        }
    }
    if (cnt < q.min_refs) cnt = 0;
    *sum_out = sum; *cnt_out = cnt;
}

// S1
__host__ __device__ inline int32_t sg_cost(int32_t sum, int32_t cnt, int len, int32_t cap) {
    if (cnt <= 0) return cap;
    const int64_t c = (int64_t)sum / ((int64_t)cnt * len * len);
    return c < cap ? (int32_t)c : cap;
}

// S1 for every level of pixel (u, v) of the rectangle, in ascending l: emit(l, C); -> the worst eligible raw pair as R6 finds it (cnt 0:
// no level is eligible)
template <class Ssd, class Emit>
__host__ __device__ inline void sg_column(const CamDev* __restrict__ cams, int n, int f, int u, int v, const RcRules& q, const SgRules& g, const Ssd& ssd,
                                          const Emit& emit, int32_t* wsum_out, int32_t* wcnt_out) {
    const double step = (q.mx - q.mn) / (double)(q.L - 1);                                    // R4
    const int len = 2 * q.N + 1;
    SgLand land;
    int32_t wsum = 0, wcnt = 0;
    for (int l = 0; l < q.L; ++l) {
        int32_t sum, cnt;
        sg_level(cams, n, f, u, v, q, step, l, ssd, land, &sum, &cnt);
        if (cnt > 0 && (wcnt == 0 || rc_less(wsum, wcnt, sum, cnt))) { wsum = sum; wcnt = cnt; }
        emit(l, sg_cost(sum, cnt, len, g.cap));
    }
    *wsum_out = wsum; *wcnt_out = wcnt;
}

// S2 for one level: c = C(p, l); here, below, above = L_r(q, l), L_r(q, l - 1), L_r(q, l + 1), SG_FAR for a level outside [0, L - 1];
// m = M_r(q)
__host__ __device__ inline int32_t sg_step(int32_t c, int32_t here, int32_t below, int32_t above, int32_t m, int32_t p1, int32_t p2) {
    int32_t best = here;
    if (below + p1 < best) best = below + p1;
    if (above + p1 < best) best = above + p1;
    if (m + p2 < best) best = m + p2;
    return c + best - m;
}

// S4-S6: the winner l* with S(p, l* - 1), S(p, l*), S(p, l* + 1) (a neighbour outside [0, L - 1]: any value, not read), its raw pair
// (cnt 0: not eligible) and the worst eligible raw pair
__host__ __device__ inline SgPixel sg_finish(const RcRules& q, int ls, int32_t s_below, int32_t s_here, int32_t s_above, int32_t sum, int32_t cnt,
                                             int32_t wsum, int32_t wcnt) {
    SgPixel x = {{0.0f, RC_NONE, -1, 0}, s_here};
    if (cnt <= 0) return x;                                                                   // S4: l* is not eligible
    x.r.sum = sum; x.r.cnt = cnt;
    const int len = 2 * q.N + 1;
    const double m = (double)sum / (double)cnt, mw = (double)wsum / (double)wcnt;
    if (!(sqrt(m / (double)(len * len)) <= q.err) || !(m < q.peak * mw)) return x;            // R7
    x.r.level = ls;
    const double step = (q.mx - q.mn) / (double)(q.L - 1);
    double d = rc_level(q.mn, q.mx, ls, q.L, step);
    if ((q.flags & 1) && ls - 1 >= 0 && ls + 1 <= q.L - 1) {                                  // S5
        const double cm = (double)s_below, c0 = (double)s_here, cp = (double)s_above;
        const double den = (cm - 2.0 * c0) + cp;
        if (den > 0.0) {
            const double o = 0.5 * ((cm - cp) / den);
            const double ds = q.mn + ((double)ls + o) * step;
            if (dr_in_bounds(ds, q.mn, q.mx)) d = ds;
        }
    }
    x.r.out = rc_value(d, q.mn, q.mx);                                                        // S6
    return x;
}

// S3-S6 for pixel (u, v) of the rectangle whose column of S is s(l)
template <class Ssd, class Col>
__host__ __device__ inline SgPixel sg_select(const CamDev* __restrict__ cams, int n, int f, int u, int v, const RcRules& q, const Ssd& ssd, const Col& s,
                                             int32_t wsum, int32_t wcnt) {
    int ls = 0;
    int32_t best = s(0);
    for (int l = 1; l < q.L; ++l) {                                                           // S3: the lowest l of the smallest S
        const int32_t x = s(l);
        if (x < best) { ls = l; best = x; }
    }
    const int32_t s_below = ls > 0 ? s(ls - 1) : 0, s_above = ls < q.L - 1 ? s(ls + 1) : 0;
    SgLand land;
    int32_t sum, cnt;
    sg_level(cams, n, f, u, v, q, (q.mx - q.mn) / (double)(q.L - 1), ls, ssd, land, &sum, &cnt);
    return sg_finish(q, ls, s_below, best, s_above, sum, cnt, wsum, wcnt);
}

#ifndef __HIP_DEVICE_COMPILE__
// The whole of S1-S6 for frame f on the host, a plain loop per rule: vol and agg hold rw * rh * L uint16 each (level fastest), line holds
// 2 * L int32.  out, level, sum, cnt and agg_out are rasters of w * h.
template <class MakeSsd>
inline void sg_frame(const CamDev* cams, int n, int f, const RcRules& q, const SgRules& g, const MakeSsd& make_ssd, uint16_t* vol, uint16_t* agg,
                     int32_t* wpair, int32_t* line, float* out, int16_t* level, int32_t* sum, uint8_t* cnt, int32_t* agg_out) {
    const int w = cams[f].w, h = cams[f].h, N = q.N, L = q.L;
    const int rw = w - 2 * N, rh = h - 2 * N;
    for (int i = 0; i < w * h; ++i) { out[i] = 0.0f; level[i] = RC_NONE; sum[i] = -1; cnt[i] = 0; agg_out[i] = -1; }
    if (rw <= 0 || rh <= 0) return;
    for (int y = 0; y < rh; ++y)
        for (int x = 0; x < rw; ++x) {
            uint16_t* col = vol + ((size_t)y * rw + x) * L;
            uint16_t* acc = agg + ((size_t)y * rw + x) * L;
            sg_column(cams, n, f, x + N, y + N, q, g, make_ssd(x + N, y + N), [&](int l, int32_t c) { col[l] = (uint16_t)c; acc[l] = 0; },
                      wpair + 2 * ((size_t)y * rw + x), wpair + 2 * ((size_t)y * rw + x) + 1);
        }
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
    int32_t *prev = line, *cur = line + L;
    for (int r = 0; r < g.paths; ++r) {
        const int dx = dirs[r][0], dy = dirs[r][1];
        for (int y0 = 0; y0 < rh; ++y0)
            for (int x0 = 0; x0 < rw; ++x0) {
                const int bx = x0 - dx, by = y0 - dy;
                if (bx >= 0 && bx < rw && by >= 0 && by < rh) continue;                       // (x0, y0) starts a line: q lies outside
                int32_t m = 0;
                for (int x = x0, y = y0, k = 0; x >= 0 && x < rw && y >= 0 && y < rh; x += dx, y += dy, ++k) {
                    const uint16_t* col = vol + ((size_t)y * rw + x) * L;
                    uint16_t* acc = agg + ((size_t)y * rw + x) * L;
                    int32_t least = SG_FAR;
                    for (int l = 0; l < L; ++l) {
                        cur[l] = k == 0 ? (int32_t)col[l]
                                        : sg_step(col[l], prev[l], l > 0 ? prev[l - 1] : SG_FAR, l < L - 1 ? prev[l + 1] : SG_FAR, m, g.p1, g.p2);
                        if (cur[l] < least) least = cur[l];
                        acc[l] = (uint16_t)(acc[l] + cur[l]);
                    }
                    m = least;
                    int32_t* t = prev; prev = cur; cur = t;
                }
            }
    }
    for (int y = 0; y < rh; ++y)
        for (int x = 0; x < rw; ++x) {
            const uint16_t* acc = agg + ((size_t)y * rw + x) * L;
            const int32_t* wp = wpair + 2 * ((size_t)y * rw + x);
            const SgPixel p = sg_select(cams, n, f, x + N, y + N, q, make_ssd(x + N, y + N), [&](int l) { return (int32_t)acc[l]; }, wp[0], wp[1]);
            const size_t i = (size_t)(y + N) * w + x + N;
            out[i] = p.r.out; level[i] = (int16_t)p.r.level; sum[i] = p.r.sum; cnt[i] = (uint8_t)p.r.cnt; agg_out[i] = p.agg;
        }
}
#endif

#endif
