// srt_refine.hip — mvs_srt_refine (include/mvs.h): joint similarity ICP of the SRT chain on the sequences' oriented points.  The
// reference has no such stage; the rules I1-I9 are this library's definition, stated in include/mvs.h.  Their per-match part is
// srt_refine_rules.h, one body for the kernel below and for host code.
//
//   k_srr_prepare   once per call: the copy of the points a target grid is built from (a point I1 excludes becomes NaN, which the
//                   grid build and d2f both ignore) and the partial bounding boxes of the mapped points (I2; min and max are order-free)
//   knn_grid_build  (knn.hip) once per sequence, in the sequence's OWN frame: the frame never moves, only the map into it does
//   k_srr_search    ONE launch per iteration over all ordered pairs (a, b): a host-built prefix table maps workgroups to pairs, so a
//                   workgroup's pair is uniform.  A thread per query maps its point into b's frame (I3), walks the shells of b's grid
//                   as k_label_nn does — bounded by the cap, so no far list — gathers the winner's fp64 point and normal and forms the
//                   121 terms of I6.  They are int64, so the order of the adds cannot change a bit: each wave reduces them, the
//                   workgroup folds its waves in LDS and issues one global atomic per non-zero sum.  No floating-point atomic.
// The 121 sums of every pair are all that leaves the device per iteration; the host solves (I7), steps the chain (I8) and uploads its
// 13 doubles per sequence.  The next search needs that chain, so every iteration waits for the stream once.
//
// How the 121 sums are reduced (SRR_FORM_*, both are built; mvs_test_srt_refine_timed runs either, profiles/r34/srt_refine.md holds
// the figures): BUTTERFLY sums each term over the wave with six xor shuffles of its two halves, lane 0 stores the result;
// LDS_ATOMIC lets every accepted lane add its term to the workgroup's slot with an LDS atomic (64 lanes on one address serialise).
// A third form was weighed and not built: the transposing butterfly (each step halves the terms a lane keeps: 126 exchanges in
// place of 726) needs all 128 int64 of a lane live at once, 256 VGPRs before the walk's own.  A wave without an accepted match skips
// the reduction altogether, which is most waves of most pairs: sequences overlap their neighbours only.
#include "engine.h"
#include "trace.h"
#include "knn_dev.h"
#include "srt_refine_rules.h"
#include "../../include/mvs_io.h"
#include "../../include/mvs_test.h"
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int TPB = 256;
constexpr int SRR_FORM_BUTTERFLY = 0, SRR_FORM_LDS_ATOMIC = 1;
constexpr int SRR_MAX_SEQ = 128;                       // n_seq^2 slots of 121 sums, a 7 n_seq square matrix on the host
constexpr int64_t SRR_MAX_QUERIES = 1 << 24;           // I6: 2^24 terms of at most 2^36 stay inside int64
constexpr int SRR_PREP_BLOCKS = 256;

struct SrrGrid { const NgGeom* geo; const int* cs; const float4* sorted; };
struct SrrArgs {
    const double* pts; const double* nrm; const int64_t* seg; const double* chain;      // chain: 13 doubles per sequence: s, R, t
    const SrrGrid* grids; const int32_t* pair_first; const int32_t* pair_ab;
    int npairs, n_seq, stride;
    SrrFrame f; double cap;
    unsigned long long* sums;
};

__device__ inline int srr_seq_of(const int64_t* seg, int n_seq, int64_t i) {      // the segment of point i: the last k with seg[k] <= i
    int lo = 0, hi = n_seq - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg[mid] <= i) lo = mid; else hi = mid - 1; }
    return lo;
}

__global__ __launch_bounds__(TPB) void k_srr_prepare(const double* __restrict__ pts, const int64_t* __restrict__ seg, int n_seq,
                                                     const double* __restrict__ chain, double* __restrict__ tpts, double* __restrict__ part) {
    const int64_t P = seg[n_seq];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < P; i += (int64_t)gridDim.x * TPB) {
        const d3 p = ld3(pts + 3 * i);
        if (!srr_usable(p)) { st3(tpts + 3 * i, mk3(NAN, NAN, NAN)); continue; }
        st3(tpts + 3 * i, p);
        const double* c = chain + 13 * srr_seq_of(seg, n_seq, i);
        const d3 y = srr_apply(srr_map(c[0], c + 1, c + 10), p);
        lo[0] = fmin(lo[0], y.x); lo[1] = fmin(lo[1], y.y); lo[2] = fmin(lo[2], y.z);
        hi[0] = fmax(hi[0], y.x); hi[1] = fmax(hi[1], y.y); hi[2] = fmax(hi[2], y.z);
    }
    __shared__ double sm[6][TPB / 64];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = lo[c], b = hi[c];
        for (int o = 32; o > 0; o >>= 1) { a = fmin(a, __shfl_xor(a, o, 64)); b = fmax(b, __shfl_xor(b, o, 64)); }
        if ((threadIdx.x & 63) == 0) { sm[c][threadIdx.x >> 6] = a; sm[3 + c][threadIdx.x >> 6] = b; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = sm[threadIdx.x][0];
        for (int w = 1; w < TPB / 64; ++w) v = threadIdx.x < 3 ? fmin(v, sm[threadIdx.x][w]) : fmax(v, sm[threadIdx.x][w]);
        part[6 * blockIdx.x + threadIdx.x] = v;
    }
}

// I3 + the early stop of I4: the index of the point of the grid nearest to q (float32, d2f, ties to the lower index), or -1 when no
// point lies within `stop` of q — then none can be accepted.  The shells and the closing bound are k_label_nn's (knn.hip).
__device__ inline int srr_nearest(const SrrGrid& G, float qx, float qy, float qz, double stop) {
    if (!((qx - qx == 0.0f) && (qy - qy == 0.0f) && (qz - qz == 0.0f))) return -1;
    const NgGeom g = *G.geo;
    {   // farther from the grid's box than the stop: nothing to walk
        const float ux = g.minx + (float)g.nx * g.h, uy = g.miny + (float)g.ny * g.h, uz = g.minz + (float)g.nz * g.h;
        const double dx = fmax(fmax((double)g.minx - qx, (double)qx - ux), 0.0), dy = fmax(fmax((double)g.miny - qy, (double)qy - uy), 0.0),
                     dz = fmax(fmax((double)g.minz - qz, (double)qz - uz), 0.0);
        if ((dx * dx + dy * dy) + dz * dz > stop * stop) return -1;
    }
    const float fx = (qx - g.minx) * g.inv_h, fy = (qy - g.miny) * g.inv_h, fz = (qz - g.minz) * g.inv_h;
    const int cx = ng_axis(qx, g.minx, g.inv_h, g.nx), cy = ng_axis(qy, g.miny, g.inv_h, g.ny), cz = ng_axis(qz, g.minz, g.inv_h, g.nz);
    float m = fminf(fminf(fminf(fx - cx, cx + 1 - fx), fminf(fy - cy, cy + 1 - fy)), fminf(fz - cz, cz + 1 - fz));
    m = fmaxf(m, 0.0f);
    float best = INFINITY;
    int arg = -1;
    auto take = [&](const float4& p) {
        const float d = d2f(qx, qy, qz, p.x, p.y, p.z);
        const int j = __float_as_int(p.w);
        if (d < best || (d == best && j < arg)) { best = d; arg = j; }
    };
    auto scan = [&](int A, int B) {
        int k = A;
        for (; k + 4 <= B; k += 4) {
            const float4 p0 = G.sorted[k], p1 = G.sorted[k + 1], p2 = G.sorted[k + 2], p3 = G.sorted[k + 3];
            take(p0); take(p1); take(p2); take(p3);
        }
        for (; k < B; ++k) take(G.sorted[k]);
    };
    const int nmax = max(g.nx, max(g.ny, g.nz));
    for (int s = 0; s <= nmax; ++s) {
        for (int dz = -s; dz <= s; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.nz) continue;
            for (int dy = -s; dy <= s; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.ny) continue;
                const int rb = (z * g.ny + y) * g.nx;
                if (abs(dy) == s || abs(dz) == s) {
                    const int x0 = max(cx - s, 0), x1 = min(cx + s, g.nx - 1);
                    if (x0 <= x1) scan(G.cs[rb + x0], G.cs[rb + x1 + 1]);
                } else {
                    if (cx - s >= 0) scan(G.cs[rb + cx - s], G.cs[rb + cx - s + 1]);
                    if (cx + s < g.nx) scan(G.cs[rb + cx + s], G.cs[rb + cx + s + 1]);
                }
            }
        }
        const float bound = ((float)s + m - 0.01f) * g.h;            // every point nearer than this has been seen
        if (bound > 0.0f && best <= bound * bound) return arg;       // the nearest point, proven
        if ((double)bound >= stop) return -1;                        // the nearest point is beyond the stop
    }
    return arg;                                                       // every cell visited
}

template <int FORM>
__global__ __launch_bounds__(TPB) void k_srr_search(SrrArgs a) {
    __shared__ long long wsum[TPB / 64][SRR_TERMS];
    for (int k = threadIdx.x; k < (TPB / 64) * SRR_TERMS; k += TPB) (&wsum[0][0])[k] = 0;
    int pair;
    {   // the last pair whose first workgroup is not behind this one (workgroup-uniform)
        int lo = 0, hi = a.npairs - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.pair_first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
        pair = lo;
    }
    const int sa = a.pair_ab[2 * pair], sb = a.pair_ab[2 * pair + 1];
    const int64_t off_a = a.seg[sa], n_a = a.seg[sa + 1] - off_a, off_b = a.seg[sb];
    const int64_t i = ((int64_t)((int)blockIdx.x - a.pair_first[pair]) * TPB + threadIdx.x) * a.stride;
    bool acc = false;
    double r = 0.0, J[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) J[k] = 0.0;
    if (i < n_a) {
        const d3 pa = ld3(a.pts + 3 * (off_a + i));
        if (srr_usable(pa)) {
            const double* ca = a.chain + 13 * sa;
            const double* cb = a.chain + 13 * sb;
            const d3 yb = srr_apply(srr_relative(cb[0], cb + 1, cb + 10, ca[0], ca + 1, ca + 10), pa);
            const SrrGrid G = a.grids[sb];
            // I4's stopping bound in b's frame: the cap there, cap D / s_b, with a slack of 1/64 of itself for the float32 distance
            // and for an R that is a rotation only to a few digits, and of 2^-18 of the largest coordinate for the float32 rounding
            // of the two points
            const NgGeom g = *G.geo;
            const double capb = a.cap * a.f.D / cb[0];
            const double ext = fmax(fmax(fmax(fabs((double)g.minx), fabs((double)g.minx + (double)g.nx * g.h)),
                                         fmax(fabs((double)g.miny), fabs((double)g.miny + (double)g.ny * g.h))),
                                    fmax(fabs((double)g.minz), fabs((double)g.minz + (double)g.nz * g.h)));
            const double stop = capb * (1.0 + 1.0 / 64.0) + (ext + capb) * (1.0 / 262144.0);
            const int j = srr_nearest(G, (float)yb.x, (float)yb.y, (float)yb.z, stop);
            if (j >= 0) {
                const d3 pb = ld3(a.pts + 3 * (off_b + j)), nb = ld3(a.nrm + 3 * (off_b + j)), na = ld3(a.nrm + 3 * (off_a + i));
                acc = srr_match(srr_map(ca[0], ca + 1, ca + 10), srr_map(cb[0], cb + 1, cb + 10), a.f, pa, na, pb, nb, &r, J);
            }
        }
    }
    __syncthreads();                                                  // the zeroes of wsum
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (__ballot(acc)) {                                              // (wave-uniform)
        if (!acc) {
            r = 0.0;
#pragma unroll
            for (int k = 0; k < 14; ++k) J[k] = 0.0;
        }
        if (FORM == SRR_FORM_BUTTERFLY) {
            srr_terms(r, J, [&](int k, long long v) {
                if (k == 0 && !acc) v = 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) wsum[w][k] = v;
            });
        } else if (acc) {
            srr_terms(r, J, [&](int k, long long v) { atomicAdd((unsigned long long*)&wsum[0][k], (unsigned long long)v); });
        }
    }
    __syncthreads();
    if (threadIdx.x < SRR_TERMS) {
        long long tot = 0;
#pragma unroll
        for (int ww = 0; ww < TPB / 64; ++ww) tot += wsum[ww][threadIdx.x];
        if (tot != 0) atomicAdd(a.sums + ((size_t)sa * a.n_seq + sb) * SRR_TERMS + threadIdx.x, (unsigned long long)tot);
    }
}

// ------------------------------------------------------------------ host: checks, solve, step ----
struct SrrPlan {
    mvs_srt_refine_params p;
    int n_seq = 0, fixed = 0;
    int64_t P = 0;
    std::vector<int64_t> seg;
    std::vector<int32_t> pair_first, pair_ab;      // the ordered pairs that have work: first workgroup of each (+ the total), (a, b)
};

int check_refine(const char* fn, const void* points, const void* normals, const int64_t* seg_off, int32_t n_seq, const double* scales,
                 const double* R, const double* t, const mvs_srt_refine_params* prm, const void* iters_done, SrrPlan* pl) {
    if (!points || !normals || !seg_off || !scales || !R || !t || !iters_done) return bad(fn, "points, normals, seg_off, scales, R, t or iters_done is NULL");
    if (n_seq < 2) return bad(fn, "need n_seq >= 2");
    if (n_seq > SRR_MAX_SEQ) return bad(fn, "more than 128 sequences");
    if (int rc = check_offsets(fn, "seg_off", seg_off, n_seq, 0x7fffffffLL)) return rc;
    if (prm) pl->p = *prm; else mvs_srt_refine_default_params(&pl->p);
    const mvs_srt_refine_params& p = pl->p;
    if (!(p.rel_dist > 0.0 && p.rel_dist <= 1.0)) return bad(fn, "rel_dist must lie in (0, 1]");
    if (!(p.min_cos >= -1.0 && p.min_cos <= 1.0)) return bad(fn, "min_cos must lie in [-1, 1]");
    if (!std::isfinite(p.damping) || p.damping < 0.0) return bad(fn, "damping must be finite and >= 0");
    if (!std::isfinite(p.tol) || p.tol < 0.0) return bad(fn, "tol must be finite and >= 0");
    if (p.iters < 1 || p.iters > 64) return bad(fn, "iters must lie in 1..64");
    if (p.stride < 1) return bad(fn, "stride must be >= 1");
    if (p.fixed_seq < -1 || p.fixed_seq >= n_seq) return bad(fn, "fixed_seq must be -1 or a sequence");
    if (p.min_pairs < 0) return bad(fn, "min_pairs must be >= 0");
    if (p.flags & ~(int32_t)MVS_SRT_REFINE_FIX_SCALE) return bad(fn, "unknown flag bits");
    if (p.reserved != 0) return bad(fn, "reserved must be 0");
    for (int k = 0; k < n_seq; ++k) {
        if (!(scales[k] > 0.0) || !std::isfinite(scales[k])) return bad(fn, "every scale must be finite and > 0");
        for (int i = 0; i < 9; ++i) if (!std::isfinite(R[9 * k + i])) return bad(fn, "R holds a value that is not finite");
        for (int i = 0; i < 3; ++i) if (!std::isfinite(t[3 * k + i])) return bad(fn, "t holds a value that is not finite");
        if ((seg_off[k + 1] - seg_off[k] + p.stride - 1) / p.stride > SRR_MAX_QUERIES) return bad(fn, "more than 2^24 queries in one sequence");
    }
    pl->n_seq = n_seq;
    pl->fixed = p.fixed_seq < 0 ? n_seq - 1 : p.fixed_seq;
    pl->P = seg_off[n_seq];
    pl->seg.assign(seg_off, seg_off + n_seq + 1);
    pl->pair_first.clear(); pl->pair_ab.clear();
    int64_t blocks = 0;
    for (int a = 0; a < n_seq; ++a)
        for (int b = 0; b < n_seq; ++b) {
            const int64_t na = seg_off[a + 1] - seg_off[a], nb = seg_off[b + 1] - seg_off[b];
            if (a == b || na == 0 || nb == 0) continue;
            pl->pair_first.push_back((int32_t)blocks);
            pl->pair_ab.push_back(a); pl->pair_ab.push_back(b);
            blocks += ((na + p.stride - 1) / p.stride + TPB - 1) / TPB;
            if (blocks > 0x3fffffffLL) return bad(fn, "too many queries over all pairs for one launch");
        }
    pl->pair_first.push_back((int32_t)blocks);
    return MVS_OK;
}

// I7.  sums: n * n slots of 121; free[k]: sequence k moves.  step: 7 n, zero where nothing moves.  MVS_E_SOLVER on a pivot <= 0.
int srr_solve(const char* fn, int n, const long long* sums, const std::vector<char>& free_seq, bool fix_scale, double damping, std::vector<double>& step) {
    const int N = 7 * n;
    std::vector<double> H((size_t)N * N, 0.0), g((size_t)N, 0.0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            if (a == b) continue;
            const long long* S = sums + ((size_t)a * n + b) * SRR_TERMS;
            if (S[0] == 0) continue;
            int k = SRR_JJ;
            for (int i = 0; i < 14; ++i)
                for (int j = i; j < 14; ++j) {
                    const double v = srr_dequant(S[k++]);
                    const int gi = i < 7 ? 7 * a + i : 7 * b + i - 7, gj = j < 7 ? 7 * a + j : 7 * b + j - 7;
                    H[(size_t)gi * N + gj] += v;
                    if (gi != gj) H[(size_t)gj * N + gi] += v;
                }
            for (int i = 0; i < 14; ++i) g[i < 7 ? 7 * a + i : 7 * b + i - 7] += srr_dequant(S[SRR_JR + i]);
        }
    std::vector<int> idx;
    for (int k = 0; k < n; ++k)
        if (free_seq[k])
            for (int i = 0; i < (fix_scale ? 6 : 7); ++i) idx.push_back(7 * k + i);
    const int m = (int)idx.size();
    std::vector<double> A((size_t)m * m), L((size_t)m * m, 0.0), y((size_t)m), x((size_t)m);
    double max_diag = 0.0;
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) A[(size_t)i * m + j] = H[(size_t)idx[i] * N + idx[j]];
        if (A[(size_t)i * m + i] > max_diag) max_diag = A[(size_t)i * m + i];
    }
    for (int i = 0; i < m; ++i) A[(size_t)i * m + i] += damping * max_diag;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[(size_t)i * m + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * m + k] * L[(size_t)j * m + k];
            if (i == j) {
                if (!(s > 0.0)) { mvs_set_error("%s: the normal matrix is not positive definite (pivot %d)", fn, i); return MVS_E_SOLVER; }
                L[(size_t)i * m + i] = sqrt(s);
            } else L[(size_t)i * m + j] = s / L[(size_t)j * m + j];
        }
    for (int i = 0; i < m; ++i) {
        double s = -g[idx[i]];
        for (int k = 0; k < i; ++k) s -= L[(size_t)i * m + k] * y[k];
        y[i] = s / L[(size_t)i * m + i];
    }
    for (int i = m - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < m; ++k) s -= L[(size_t)k * m + i] * x[k];
        x[i] = s / L[(size_t)i * m + i];
    }
    step.assign((size_t)N, 0.0);
    for (int i = 0; i < m; ++i) step[idx[i]] = x[i];
    return MVS_OK;
}

// I8: the step (w, tau, sigma) on one entry of the chain
void srr_step(const double* st, const double* c, double D, double* s, double* R, double* t) {
    const double wx = st[0], wy = st[1], wz = st[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
    double dR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0.0) {
        const double ka = sin(th) / th, kb = (1.0 - cos(th)) / th2;
        const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
                dR[3 * i + j] = (dR[3 * i + j] + ka * K[3 * i + j]) + kb * k2;
            }
    }
    const double gg = exp(st[6]);
    double Rn[9], gdR[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j];
    for (int i = 0; i < 9; ++i) gdR[i] = gg * dR[i];
    const d3 cc = mk3(c[0], c[1], c[2]);
    const d3 tn = mulMv(gdR, ld3(t)) + ((cc - mulMv(gdR, cc)) + D * mk3(st[3], st[4], st[5]));
    *s = gg * *s;
    std::memcpy(R, Rn, sizeof Rn);
    st3(t, tn);
}

struct SrrHook { long long* sums; double* c_D; int form, reps; double* ms; };      // mvs_test_srt_refine_*: one search, nothing else

// the call on device arrays, everything ordered on s; the chain and the reports are host arrays
int srr_run(const char* fn, const SrrPlan& pl, const double* dpts, const double* dnrm, double* scales, double* R, double* t,
            int32_t* iters_done, double* history, int64_t* pair_count, hipStream_t s, const SrrHook* hook) {
    const int n = pl.n_seq;
    const double t_begin = now_ms();
    const mvs_srt_refine_params& p = pl.p;
    const int npairs = (int)pl.pair_ab.size() / 2, nblocks = pl.pair_first.back();
    const size_t nsum = (size_t)n * n * SRR_TERMS;
    std::vector<double> chain((size_t)13 * n), part((size_t)6 * SRR_PREP_BLOCKS);
    std::vector<long long> sums(nsum, 0);
    std::vector<SrrGrid> grids((size_t)n, SrrGrid{nullptr, nullptr, nullptr});
    auto pack = [&]() {
        for (int k = 0; k < n; ++k) {
            chain[13 * k] = scales[k];
            std::memcpy(&chain[13 * k + 1], R + 9 * k, 72);
            std::memcpy(&chain[13 * k + 10], t + 3 * k, 24);
        }
    };
    pack();
    if (iters_done) *iters_done = 0;
    if (pair_count) std::memset(pair_count, 0, sizeof(int64_t) * n * n);
    int rc;
    Scratch dseg, dchain, dtp, dpart, dgrids, dws, dfirst, dab, dsums;
    std::vector<size_t> ws_off((size_t)n + 1, 0);
    for (int k = 0; k < n; ++k) {
        const int64_t nk = pl.seg[k + 1] - pl.seg[k];
        ws_off[k + 1] = ws_off[k] + (nk > 0 ? (knn_grid_ws_bytes((int)nk) + 255) / 256 * 256 : 0);
    }
    if ((rc = up_async(dseg, pl.seg.data(), pl.seg.size(), s)) || (rc = up_async(dchain, chain.data(), chain.size(), s)) ||
        (rc = dtp.alloc(sizeof(double) * 3 * (size_t)pl.P, s)) || (rc = dpart.alloc(sizeof(double) * part.size(), s)) ||
        (rc = dws.alloc(ws_off[n], s)) || (rc = dsums.alloc(sizeof(long long) * nsum, s))) return rc;
    // I2
    k_srr_prepare<<<dim3(SRR_PREP_BLOCKS), dim3(TPB), 0, s>>>(dpts, dseg.as<int64_t>(), n, dchain.as<double>(), dtp.as<double>(), dpart.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(part.data(), dpart.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = 0; b < SRR_PREP_BLOCKS; ++b)
        for (int c = 0; c < 3; ++c) { lo[c] = fmin(lo[c], part[6 * b + c]); hi[c] = fmax(hi[c], part[6 * b + 3 + c]); }
    SrrFrame f;
    const d3 ext = mk3(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);
    for (int c = 0; c < 3; ++c) f.c[c] = (lo[c] + hi[c]) / 2.0;
    f.D = norm3(ext) / 2.0;
    if (!(lo[0] <= hi[0]) || !(f.D > 0.0) || !std::isfinite(f.D)) { mvs_set_error("%s: the mapped points span no finite box", fn); return MVS_E_DEGENERATE; }
    const double cap = 2.0 * p.rel_dist;
    f.cap2 = cap * cap; f.min_cos = p.min_cos;
    if (hook && hook->c_D) { hook->c_D[0] = f.c[0]; hook->c_D[1] = f.c[1]; hook->c_D[2] = f.c[2]; hook->c_D[3] = f.D; }
    // the target grids, once: each in its sequence's own frame
    for (int k = 0; k < n; ++k) {
        const int64_t nk = pl.seg[k + 1] - pl.seg[k];
        if (nk == 0) continue;
        void* ws = (char*)dws.p + ws_off[k];
        knn_grid_build(dtp.as<double>() + 3 * pl.seg[k], (int)nk, ws, s);
        const void *geo, *sorted; const int* cs;
        knn_grid_views(ws, (int)nk, &geo, &cs, &sorted);
        grids[k] = SrrGrid{(const NgGeom*)geo, cs, (const float4*)sorted};
    }
    HIPCHK(hipGetLastError());
    if ((rc = up_async(dgrids, grids.data(), grids.size(), s)) || (rc = up_async(dfirst, pl.pair_first.data(), pl.pair_first.size(), s)) ||
        (rc = up_async(dab, pl.pair_ab.data(), pl.pair_ab.size(), s))) return rc;
    double t_setup = 0.0;
    if (hook && hook->ms) {                                                             // the timed hook alone waits here
        HIPCHK(hipStreamSynchronize(s));
        t_setup = now_ms() - t_begin;
    }
    SrrArgs a{dpts, dnrm, dseg.as<int64_t>(), dchain.as<double>(), dgrids.as<SrrGrid>(), dfirst.as<int32_t>(), dab.as<int32_t>(),
              npairs, n, p.stride, f, cap, dsums.as<unsigned long long>()};
    auto search = [&](int form) -> int {              // chain up, sums down, one wait
        HIPCHK(hipMemcpyAsync(dchain.p, chain.data(), sizeof(double) * chain.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(dsums.p, 0, sizeof(long long) * nsum, s));
        if (nblocks > 0) {
            if (form == SRR_FORM_LDS_ATOMIC) k_srr_search<SRR_FORM_LDS_ATOMIC><<<dim3((unsigned)nblocks), dim3(TPB), 0, s>>>(a);
            else k_srr_search<SRR_FORM_BUTTERFLY><<<dim3((unsigned)nblocks), dim3(TPB), 0, s>>>(a);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(sums.data(), dsums.p, sizeof(long long) * nsum, hipMemcpyDeviceToHost, s));
        return mvs_check_hip(hipStreamSynchronize(s), "srt_refine search");
    };
    if (hook) {
        StageClock clk(hook->ms != nullptr);
        if ((rc = search(hook->form))) return rc;                                      // (also the warm-up of the timed launches)
        if (hook->ms) {
            if ((rc = clk.mark(s))) return rc;
            for (int i = 0; i < hook->reps; ++i) {
                if (hook->form == SRR_FORM_LDS_ATOMIC) k_srr_search<SRR_FORM_LDS_ATOMIC><<<dim3((unsigned)nblocks), dim3(TPB), 0, s>>>(a);
                else k_srr_search<SRR_FORM_BUTTERFLY><<<dim3((unsigned)nblocks), dim3(TPB), 0, s>>>(a);
            }
            if ((rc = clk.mark(s))) return rc;
            HIPCHK(hipStreamSynchronize(s));
            if ((rc = clk.read(hook->ms))) return rc;
            hook->ms[0] /= hook->reps;
            // the host solve of I7 on these sums, every sequence but the fixed one free
            std::vector<char> fr((size_t)n, 1);
            std::vector<double> st;
            fr[pl.fixed] = 0;
            const double t0 = now_ms();
            const int src = srr_solve(fn, n, sums.data(), fr, (p.flags & MVS_SRT_REFINE_FIX_SCALE) != 0, p.damping, st);
            hook->ms[1] = src ? -1.0 : now_ms() - t0;
            hook->ms[2] = t_setup;
        }
        std::memcpy(hook->sums, sums.data(), sizeof(long long) * nsum);
        return MVS_OK;
    }
    std::vector<char> free_seq((size_t)n);
    std::vector<double> step;
    for (int it = 0; it < p.iters; ++it) {
        if ((rc = search(SRR_FORM_BUTTERFLY))) return rc;
        long long total = 0;
        double rr = 0.0;
        std::vector<long long> per((size_t)n, 0);
        for (int x = 0; x < n; ++x)
            for (int y = 0; y < n; ++y) {
                const long long* S = &sums[((size_t)x * n + y) * SRR_TERMS];
                if (pair_count) pair_count[(size_t)x * n + y] = S[0];
                total += S[0]; per[x] += S[0]; per[y] += S[0];
                rr += srr_dequant(S[SRR_RR]);
            }
        bool any = false;
        for (int k = 0; k < n; ++k) { free_seq[k] = k != pl.fixed && per[k] >= p.min_pairs && per[k] > 0; any = any || free_seq[k]; }
        if (!any) break;                                                                // I7.6: nothing moves, nothing is written
        if ((rc = srr_solve(fn, n, sums.data(), free_seq, (p.flags & MVS_SRT_REFINE_FIX_SCALE) != 0, p.damping, step))) return rc;
        if (history) { history[2 * it] = (double)total; history[2 * it + 1] = f.D * sqrt(rr / (double)total); }
        double big = 0.0;
        for (int k = 0; k < n; ++k) {
            if (!free_seq[k]) continue;
            srr_step(&step[7 * k], f.c, f.D, scales + k, R + 9 * k, t + 3 * k);
            for (int i = 0; i < 7; ++i) big = fmax(big, fabs(step[7 * k + i]));
        }
        pack();
        *iters_done = it + 1;
        if (big < p.tol) break;                                                         // I9
    }
    return MVS_OK;
}

int refine_host(const char* fn, const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq, double* scales, double* R,
                double* t, const mvs_srt_refine_params* prm, int32_t* iters_done, double* history, int64_t* pair_count, const SrrHook* hook) {
    SrrPlan pl;
    int rc = check_refine(fn, points, normals, seg_off, n_seq, scales, R, t, prm, hook ? (const void*)hook->sums : (const void*)iters_done, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    Scratch dp, dn;
    if ((rc = up(dp, points, 3 * (size_t)pl.P)) || (rc = up(dn, normals, 3 * (size_t)pl.P))) return rc;
    return srr_run(fn, pl, dp.as<double>(), dn.as<double>(), scales, R, t, iters_done, history, pair_count, nullptr, hook);
}

}  // namespace

extern "C" {

void mvs_srt_refine_default_params(mvs_srt_refine_params* p) {
    if (!p) return;
    p->rel_dist = 0.02; p->min_cos = 0.7; p->damping = 1e-9; p->tol = 1e-9;
    p->iters = 20; p->stride = 1; p->fixed_seq = -1; p->min_pairs = 64; p->flags = 0; p->reserved = 0;
}

int mvs_srt_refine(const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq, double* scales, double* R, double* t,
                   const mvs_srt_refine_params* p, int32_t* iters_done, double* history, int64_t* pair_count) {
    MVS_TRACE();
    return refine_host(__func__, points, normals, seg_off, n_seq, scales, R, t, p, iters_done, history, pair_count, nullptr);
}

int mvs_srt_refine_dev(const double* points_dev, const double* normals_dev, const int64_t* seg_off, int32_t n_seq, double* scales, double* R,
                       double* t, const mvs_srt_refine_params* p, int32_t* iters_done, double* history, int64_t* pair_count, void* hip_stream) {
    MVS_TRACE();
    SrrPlan pl;
    int rc = check_refine(__func__, points_dev, normals_dev, seg_off, n_seq, scales, R, t, p, iters_done, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return srr_run(__func__, pl, points_dev, normals_dev, scales, R, t, iters_done, history, pair_count, (hipStream_t)hip_stream, nullptr);
}

int mvs_processor_refine_srt(int32_t n_seq, const char* const* npts_paths, const char* srt_in, const mvs_srt_refine_params* p, const char* srt_out,
                             int32_t* iters_done, double* history) {
    MVS_TRACE();
    if (!npts_paths || !srt_in || !srt_out || !iters_done) return bad(__func__, "npts_paths, srt_in, srt_out or iters_done is NULL");
    if (n_seq < 2) return bad(__func__, "need n_seq >= 2");
    for (int k = 0; k < n_seq; ++k)
        if (!npts_paths[k]) return bad(__func__, "a path of npts_paths is NULL");
    int rc;
    std::vector<int64_t> off((size_t)n_seq + 1, 0);
    for (int k = 0; k < n_seq; ++k) {
        int64_t n = 0;
        if ((rc = mvs_npts_read(npts_paths[k], &n, nullptr, nullptr))) return rc;
        off[k + 1] = off[k] + n;
    }
    const int64_t P = off[n_seq];
    std::vector<double> hp((size_t)P * 3 + 1), hn((size_t)P * 3 + 1), s((size_t)n_seq), R((size_t)n_seq * 9), t((size_t)n_seq * 3);
    for (int k = 0; k < n_seq; ++k) {
        int64_t n = off[k + 1] - off[k];
        if ((rc = mvs_npts_read(npts_paths[k], &n, hp.data() + 3 * off[k], hn.data() + 3 * off[k]))) return rc;
        if (n != off[k + 1] - off[k]) { mvs_set_error("%s changed while it was read", npts_paths[k]); return MVS_E_IO; }
    }
    if ((rc = mvs_srt_txt_read(srt_in, n_seq, s.data(), R.data(), t.data()))) return rc;
    if ((rc = refine_host(__func__, hp.data(), hn.data(), off.data(), n_seq, s.data(), R.data(), t.data(), p, iters_done, history, nullptr, nullptr))) return rc;
    return mvs_srt_txt_write(srt_out, n_seq, s.data(), R.data(), t.data());
}

int mvs_test_srt_refine_timed(const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq, const double* scales,
                              const double* R, const double* t, const mvs_srt_refine_params* p, int64_t* sums, double* c_D, int32_t form,
                              int32_t reps, double* ms) {
    if (form != SRR_FORM_BUTTERFLY && form != SRR_FORM_LDS_ATOMIC) return bad(__func__, "form must be 0 or 1");
    if (ms && reps < 1) return bad(__func__, "need reps >= 1");
    SrrHook hook{(long long*)sums, c_D, form, reps, ms};
    return refine_host(__func__, points, normals, seg_off, n_seq, const_cast<double*>(scales), const_cast<double*>(R), const_cast<double*>(t), p,
                       nullptr, nullptr, nullptr, &hook);
}

int mvs_test_srt_refine_sums(const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq, const double* scales,
                             const double* R, const double* t, const mvs_srt_refine_params* p, int64_t* sums, double* c_D) {
    if (!sums) return bad(__func__, "sums is NULL");
    SrrHook hook{(long long*)sums, c_D, SRR_FORM_BUTTERFLY, 1, nullptr};
    return refine_host(__func__, points, normals, seg_off, n_seq, const_cast<double*>(scales), const_cast<double*>(R), const_cast<double*>(t), p,
                       nullptr, nullptr, nullptr, &hook);
}

}  // extern "C"
