// depth_sgm.hip — mvs_recover_depth_maps_aggregated (include/mvs.h): the plane sweep of depth_recover.hip with semi-global path
// aggregation of its cost volume before the winner is taken, rules S1-S6 (this library's definition).  The per-pixel rules are
// depth_sgm_rules.h, one body for these kernels and for host code; the window cost of R5 on the device is depth_cost_dev.h.
//
// Two uint16 volumes per group of frames, C and S, in the layout [frame][pixel of the rectangle, row-major][level], level fastest: the
// column of one pixel is one run of 2 L bytes, so a wave that walks a row, a column or a diagonal loads and stores whole columns
// coalesced whatever the direction.
//
//   k_sg_volume  the sweep's mapping (a workgroup per DR_TILE x DR_TILE tile, a thread per pixel walking every level): writes C (S1) and
//                the worst eligible raw pair of every pixel of the rectangle (S4).
//   k_sg_paths   one wave64 per line of one family (rows, columns, the two diagonals), the lines of every frame of the group in one
//                launch.  A lane holds K consecutive levels in registers; the wave walks the line forwards and then backwards (the two
//                directions of the family), takes l - 1 and l + 1 across lanes, M_r by a wave reduction, and adds L_r into S.  Within a
//                launch a pixel lies on exactly one line, so S has one owner per entry; the first pass of the row family stores S, every
//                other pass adds to it.  The families are launches on one stream.  No atomic: two runs give the same bytes.
//   k_sg_select  the sweep's mapping again: argmin of S (S3), the raw pair of the winner by one more DotSsd level, S4-S6, the outputs.
#include "engine.h"
#include "trace.h"
#include "stitch.h"
#include "knobs.h"
#include "depth_recover_plan.h"
#include "depth_sgm_rules.h"

namespace {

constexpr int SG_WAVES = 4;            // lines per workgroup of k_sg_paths

__global__ __launch_bounds__(DR_TPB) void k_sg_volume(const uint8_t* __restrict__ grey, const uint32_t* __restrict__ sq, const CamDev* __restrict__ cams,
                                                      const DrSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int maxblk, int cam0, RcRules q,
                                                      SgRules g, const int64_t* __restrict__ roff, uint16_t* __restrict__ vol, int2* __restrict__ wpair) {
    __shared__ DrTile lds;
    const int cam = cam0 + blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const DrSeq s = seqs[seq_of[cam]];
    if (b >= s.tw * s.th) return;                                        // the whole workgroup: no barrier is skipped by a part of it
    const int f = cam - s.cam0, N = q.N;
    const int u0 = (b % s.tw) * DR_TILE, v0 = (b / s.tw) * DR_TILE;
    const int64_t npx = (int64_t)s.w * s.h;
    lds.load(grey + s.px_off + f * npx, s.w, s.h, u0, v0, N);
    const int tx = threadIdx.x % DR_TILE, ty = threadIdx.x / DR_TILE, u = u0 + tx, v = v0 + ty;
    if (!dr_interior(u, v, s.w, s.h, N)) return;                         // S1: the rectangle
    const int64_t at = s.px_off + f * npx + (int64_t)v * s.w + u;
    const int64_t rp = roff[cam] + (int64_t)(v - N) * (s.w - 2 * N) + (u - N);
    uint16_t* col = vol + rp * q.L;
    const DotSsd ssd = lds.ssd(grey, sq, s, at, tx, ty, N);
    int32_t wsum, wcnt;
    sg_column(cams + s.cam0, s.n, f, u, v, q, g, ssd, [col](int l, int32_t c) { col[l] = (uint16_t)c; }, &wsum, &wcnt);
    wpair[rp] = make_int2(wsum, wcnt);
}

// line `line` of family `fam` in a rectangle of rw x rh: its first pixel, its step and its length (0: the family has no such line)
__device__ inline int sg_line(int fam, int line, int rw, int rh, int* x0, int* y0, int* dx, int* dy) {
    switch (fam) {
    case 0: *x0 = 0; *y0 = line; *dx = 1; *dy = 0; return line < rh ? rw : 0;
    case 1: *x0 = line; *y0 = 0; *dx = 0; *dy = 1; return line < rw ? rh : 0;
    case 2:                                                              // (1, 1): from the left edge upwards, then along the top edge
        *dx = 1; *dy = 1;
        if (line >= rw + rh - 1) return 0;
        if (line < rh) { *x0 = 0; *y0 = rh - 1 - line; } else { *x0 = line - rh + 1; *y0 = 0; }
        return min(rw - *x0, rh - *y0);
    default:                                                             // (1, -1): from the left edge downwards, then along the bottom edge
        *dx = 1; *dy = -1;
        if (line >= rw + rh - 1) return 0;
        if (line < rh) { *x0 = 0; *y0 = line; } else { *x0 = line - rh + 1; *y0 = rh - 1; }
        return min(rw - *x0, *y0 + 1);
    }
}

template <int K>
__global__ __launch_bounds__(64 * SG_WAVES) void k_sg_paths(const DrSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int cam0, int ncam,
                                                            int maxlines, int fam, int N, int L, SgRules g, const int64_t* __restrict__ roff,
                                                            const uint16_t* __restrict__ vol, uint16_t* __restrict__ agg) {
    const int64_t wave = (int64_t)blockIdx.x * SG_WAVES + threadIdx.x / 64;
    if (wave >= (int64_t)ncam * maxlines) return;                        // a whole wave; the kernel has no barrier
    const int cam = cam0 + (int)(wave / maxlines), line = (int)(wave % maxlines);
    const DrSeq s = seqs[seq_of[cam]];
    const int rw = s.w - 2 * N, rh = s.h - 2 * N;
    if (rw <= 0 || rh <= 0) return;
    int x0, y0, dx, dy;
    const int n = sg_line(fam, line, rw, rh, &x0, &y0, &dx, &dy);
    if (n <= 0) return;
    const int lane = threadIdx.x & 63, l0 = lane * K;
    const int64_t base = roff[cam];
    int32_t prev[K], cur[K], c[K], a[K], cn[K], an[K];
    for (int pass = 0; pass < 2; ++pass) {
        const bool add = fam != 0 || pass != 0;                          // the first pass of the rows stores S
        auto column = [&](int k) {                                       // the k-th pixel of this pass -> the offset of its column
            const int i = pass == 0 ? k : n - 1 - k;
            return (base + (int64_t)(y0 + i * dy) * rw + (x0 + i * dx)) * L + l0;
        };
        auto fetch = [&](int64_t off, int32_t (&cc)[K], int32_t (&aa)[K]) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const bool live = l0 + j < L;
                cc[j] = live ? (int32_t)vol[off + j] : 0;
                aa[j] = live && add ? (int32_t)agg[off + j] : 0;
            }
        };
        int32_t m = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) prev[j] = SG_FAR;                    // the first pixel of a line reads no neighbour
        int64_t off = column(0);
        fetch(off, c, a);
        for (int k = 0; k < n; ++k) {
            const int64_t next = k + 1 < n ? column(k + 1) : off;
            if (k + 1 < n) fetch(next, cn, an);                          // the next column is on its way while this one is worked on
            int32_t below = __shfl_up(prev[K - 1], 1), above = __shfl_down(prev[0], 1);
            if (lane == 0) below = SG_FAR;
            if (lane == 63) above = SG_FAR;
            int32_t least = SG_FAR;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (l0 + j >= L) cur[j] = SG_FAR;                        // no such level: it never wins a minimum
                else if (k == 0) cur[j] = c[j];
                else cur[j] = sg_step(c[j], prev[j], j > 0 ? prev[j - 1] : below, j < K - 1 ? prev[j + 1] : above, m, g.p1, g.p2);
                least = min(least, cur[j]);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) least = min(least, __shfl_xor(least, d));
            m = least;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (l0 + j < L) agg[off + j] = (uint16_t)(a[j] + cur[j]);
                prev[j] = cur[j]; c[j] = cn[j]; a[j] = an[j];
            }
            off = next;
        }
    }
}

__global__ __launch_bounds__(DR_TPB) void k_sg_select(const uint8_t* __restrict__ grey, const uint32_t* __restrict__ sq, const CamDev* __restrict__ cams,
                                                      const DrSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int maxblk, int cam0, RcRules q,
                                                      const int64_t* __restrict__ roff, const uint16_t* __restrict__ agg, const int2* __restrict__ wpair,
                                                      float* __restrict__ out, int16_t* __restrict__ level_out, int32_t* __restrict__ sum_out,
                                                      uint8_t* __restrict__ cnt_out, int32_t* __restrict__ agg_out) {
    __shared__ DrTile lds;
    const int cam = cam0 + blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const DrSeq s = seqs[seq_of[cam]];
    if (b >= s.tw * s.th) return;
    const int f = cam - s.cam0, N = q.N;
    const int u0 = (b % s.tw) * DR_TILE, v0 = (b / s.tw) * DR_TILE;
    const int64_t npx = (int64_t)s.w * s.h;
    lds.load(grey + s.px_off + f * npx, s.w, s.h, u0, v0, N);
    const int tx = threadIdx.x % DR_TILE, ty = threadIdx.x / DR_TILE, u = u0 + tx, v = v0 + ty;
    if (u >= s.w || v >= s.h) return;
    const int64_t at = s.px_off + f * npx + (int64_t)v * s.w + u;
    SgPixel r = {{0.0f, RC_NONE, -1, 0}, -1};                            // outside the rectangle
    if (dr_interior(u, v, s.w, s.h, N)) {
        const int64_t rp = roff[cam] + (int64_t)(v - N) * (s.w - 2 * N) + (u - N);
        const uint16_t* col = agg + rp * q.L;
        const int2 wp = wpair[rp];
        const DotSsd ssd = lds.ssd(grey, sq, s, at, tx, ty, N);
        r = sg_select(cams + s.cam0, s.n, f, u, v, q, ssd, [col](int l) { return (int32_t)col[l]; }, wp.x, wp.y);
    }
    out[at] = r.r.out;
    if (level_out) level_out[at] = (int16_t)r.r.level;
    if (sum_out) sum_out[at] = r.r.sum;
    if (cnt_out) cnt_out[at] = (uint8_t)r.r.cnt;
    if (agg_out) agg_out[at] = r.agg;
}

// what a call is made of, built by the argument checks on the host: the plain sweep's plan, the penalties, and the frames cut into
// groups whose volumes fit the budget
struct SgPlan : RcPlan {
    SgRules g;
    std::vector<int64_t> roff;         // per camera: pixels of the rectangles in front of it in its group
    std::vector<int32_t> group;        // cameras [group[i], group[i + 1]) form group i
    int64_t most = 0;                  // rectangle pixels of the largest group
    int maxlines[4] = {0, 0, 0, 0};    // lines per frame and family, the most any sequence has
};

int check_sg(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const void* imgs, const mvs_depth_recover_params* p,
             const mvs_depth_aggregate_params* ap, const void* out, SgPlan* pl) {
    int rc = check_rc(fn, n_seq, cam_off, cams, imgs, p, out, pl);
    if (rc) return rc;
    mvs_depth_aggregate_params dflt;
    if (!ap) { mvs_depth_aggregate_default_params(&dflt); ap = &dflt; }
    if (ap->p1 < 0 || ap->p1 > ap->p2 || ap->p2 > 4095) return bad(fn, "need 0 <= p1 <= p2 <= 4095");
    if (ap->cost_cap < 1 || ap->cost_cap > 4095) return bad(fn, "cost_cap must lie in [1, 4095]");
    if (ap->paths != 4 && ap->paths != 8) return bad(fn, "paths must be 4 or 8");
    if (ap->max_volume_mb < 0) return bad(fn, "max_volume_mb is negative");
    if (ap->reserved != 0) return bad(fn, "reserved (aggregation) must be 0");
    pl->g = SgRules{ap->p1, ap->p2, ap->cost_cap, ap->paths};
    const int64_t budget = (int64_t)(ap->max_volume_mb > 0 ? ap->max_volume_mb : MVS_SGM_VOLUME_MB) << 20;
    const int N = pl->q.N, L = pl->q.L;
    pl->roff.assign((size_t)pl->ncam, 0);
    pl->group.assign(1, 0);
    int64_t held = 0;
    for (const DrSeq& s : pl->seqs) {
        const int64_t rw = s.w - 2 * N, rh = s.h - 2 * N;
        const int64_t rect = rw > 0 && rh > 0 ? rw * rh : 0, bytes = 4 * rect * L;          // C and S, uint16 each
        if (s.n && bytes > budget) {
            mvs_set_error("%s: the volumes of one frame of %d x %d at %d levels need %lld MB, the budget is %lld MB (max_volume_mb)", fn, s.w, s.h, L,
                          (long long)((bytes + (1 << 20) - 1) >> 20), (long long)(budget >> 20));
            return MVS_E_INVALID_ARG;
        }
        if (rect) {
            pl->maxlines[0] = std::max<int>(pl->maxlines[0], (int)rh);
            pl->maxlines[1] = std::max<int>(pl->maxlines[1], (int)rw);
            if (rw + rh - 1 > 0x7fffffffLL) return bad(fn, "too many diagonals in a frame");
            pl->maxlines[2] = pl->maxlines[3] = std::max<int>(pl->maxlines[2], (int)(rw + rh - 1));
        }
        for (int f = 0; f < s.n; ++f) {
            if (4 * (held + rect) * L > budget) {                                           // this frame opens the next group
                pl->group.push_back(s.cam0 + f);
                held = 0;
            }
            pl->roff[(size_t)(s.cam0 + f)] = held;
            held += rect;
            pl->most = std::max(pl->most, held);
        }
    }
    pl->group.push_back(pl->ncam);
    for (int fam = 0; fam < 4; ++fam)
        if (((int64_t)pl->ncam * pl->maxlines[fam] + SG_WAVES - 1) / SG_WAVES > 0x7fffffffLL) return bad(fn, "cameras * lines is too large for one launch");
    return MVS_OK;
}

template <int K>
void launch_paths(const SgPlan& pl, int fam, int c0, int nc, const DrSeq* seqs, const int32_t* sof, const int64_t* roff, const uint16_t* vol, uint16_t* agg,
                  hipStream_t s) {
    const int64_t waves = (int64_t)nc * pl.maxlines[fam];
    k_sg_paths<K><<<dim3((unsigned)((waves + SG_WAVES - 1) / SG_WAVES)), dim3(64 * SG_WAVES), 0, s>>>(seqs, sof, c0, nc, pl.maxlines[fam], fam, pl.q.N, pl.q.L,
                                                                                                      pl.g, roff, vol, agg);
}

// the grey pass, the squares, and per group the volume, the path families and the selection, on device arrays, enqueued on s; the tables
// stay alive in the object until the caller has synchronised
struct SgRun {
    DrCost cost;
    Scratch droff, dvol, dagg, dwp;
    int launch(const SgPlan& pl, const mvs_camera* cams, const uint8_t* imgs, float* out, int16_t* level_out, int32_t* sum_out, uint8_t* cnt_out,
               int32_t* agg_out, hipStream_t s) {
        int rc;
        const size_t entries = (size_t)pl.most * (size_t)pl.q.L;
        if ((rc = cost.launch(pl, pl.q.N, cams, imgs, s)) || (rc = up_async(droff, pl.roff.data(), pl.roff.size(), s)) ||
            (rc = dvol.alloc(sizeof(uint16_t) * entries, s)) || (rc = dagg.alloc(sizeof(uint16_t) * entries, s)) ||
            (rc = dwp.alloc(sizeof(int2) * (size_t)pl.most, s))) return rc;
        const DrSeq* seqs = cost.dseq.as<DrSeq>();
        const int32_t* sof = cost.dsof.as<int32_t>();
        const int64_t* roff = droff.as<int64_t>();
        const int per = (pl.q.L + 63) / 64;                                                 // levels per lane, rounded up to a power of two
        for (size_t i = 0; i + 1 < pl.group.size(); ++i) {
            const int c0 = pl.group[i], nc = pl.group[i + 1] - c0;
            if (!nc) continue;
            const dim3 tiles((unsigned)(nc * pl.maxblk));
            k_sg_volume<<<tiles, dim3(DR_TPB), 0, s>>>(cost.dgrey.as<uint8_t>(), cost.dsq.as<uint32_t>(), cost.dcam.as<CamDev>(), seqs, sof, pl.maxblk, c0, pl.q,
                                                       pl.g, roff, dvol.as<uint16_t>(), dwp.as<int2>());
            for (int fam = 0; fam < pl.g.paths / 2; ++fam) {
                if (!pl.maxlines[fam]) continue;
                if (per <= 1) launch_paths<1>(pl, fam, c0, nc, seqs, sof, roff, dvol.as<uint16_t>(), dagg.as<uint16_t>(), s);
                else if (per <= 2) launch_paths<2>(pl, fam, c0, nc, seqs, sof, roff, dvol.as<uint16_t>(), dagg.as<uint16_t>(), s);
                else if (per <= 4) launch_paths<4>(pl, fam, c0, nc, seqs, sof, roff, dvol.as<uint16_t>(), dagg.as<uint16_t>(), s);
                else if (per <= 8) launch_paths<8>(pl, fam, c0, nc, seqs, sof, roff, dvol.as<uint16_t>(), dagg.as<uint16_t>(), s);
                else launch_paths<16>(pl, fam, c0, nc, seqs, sof, roff, dvol.as<uint16_t>(), dagg.as<uint16_t>(), s);
            }
            k_sg_select<<<tiles, dim3(DR_TPB), 0, s>>>(cost.dgrey.as<uint8_t>(), cost.dsq.as<uint32_t>(), cost.dcam.as<CamDev>(), seqs, sof, pl.maxblk, c0, pl.q,
                                                       roff, dagg.as<uint16_t>(), dwp.as<int2>(), out, level_out, sum_out, cnt_out, agg_out);
            HIPCHK(hipGetLastError());
        }
        return MVS_OK;
    }
};

}  // namespace

// the host form under the name fn (mvs_recover_depth_maps_aggregated, mvs_processor_recover_depths_aggregated)
int recover_depth_maps_aggregated_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                                       const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* ap, float* out, int16_t* level_out,
                                       int32_t* sum_out, uint8_t* cnt_out, int32_t* agg_out) {
    SgPlan pl;
    int rc = check_sg(fn, n_seq, cam_off, cams, imgs, p, ap, out, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    const size_t n = (size_t)pl.px;
    Scratch di, dout, dl, dsum, dcnt, dagg;
    if ((rc = up(di, imgs, 3 * n)) || (rc = dout.alloc(sizeof(float) * n)) || (level_out && (rc = dl.alloc(sizeof(int16_t) * n))) ||
        (sum_out && (rc = dsum.alloc(sizeof(int32_t) * n))) || (cnt_out && (rc = dcnt.alloc(n))) || (agg_out && (rc = dagg.alloc(sizeof(int32_t) * n))))
        return rc;
    SgRun run;
    if ((rc = run.launch(pl, cams, di.as<uint8_t>(), dout.as<float>(), level_out ? dl.as<int16_t>() : nullptr, sum_out ? dsum.as<int32_t>() : nullptr,
                         cnt_out ? dcnt.as<uint8_t>() : nullptr, agg_out ? dagg.as<int32_t>() : nullptr, nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(out, dout, n))) return rc;
    if (level_out && (rc = down(level_out, dl, n))) return rc;
    if (sum_out && (rc = down(sum_out, dsum, n))) return rc;
    if (cnt_out && (rc = down(cnt_out, dcnt, n))) return rc;
    return agg_out ? down(agg_out, dagg, n) : MVS_OK;
}

// every argument check of the call that needs neither the images nor the outputs, under the name fn: what a file form asks before it
// reads a frame.  ap may be NULL (defaults)
int recover_depth_maps_aggregated_check(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams,
                                        const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* ap) {
    SgPlan pl;
    return check_sg(fn, n_seq, cam_off, cams, /*imgs: not looked at*/ cams, p, ap, /*out: not looked at*/ cams, &pl);
}

// every kernel of this translation unit, for the cold-start preload of runtime.cpp
const void* const* mvs_tu_kernels_depth_sgm(int* n) {
    static const void* const ks[] = {
        (const void*)k_dr_grey,
        (const void*)k_dr_squares,
        (const void*)k_sg_volume,
        (const void*)k_sg_paths<1>,
        (const void*)k_sg_paths<2>,
        (const void*)k_sg_paths<4>,
        (const void*)k_sg_paths<8>,
        (const void*)k_sg_paths<16>,
        (const void*)k_sg_select};
    *n = (int)(sizeof ks / sizeof ks[0]);
    return ks;
}

extern "C" {

void mvs_depth_aggregate_default_params(mvs_depth_aggregate_params* p) {
    if (!p) return;
    p->p1 = 8; p->p2 = 128; p->cost_cap = 255; p->paths = 8; p->max_volume_mb = 0; p->reserved = 0;
}

int mvs_recover_depth_maps_aggregated(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                                      const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* ap, float* out, int16_t* level_out,
                                      int32_t* sum_out, uint8_t* cnt_out, int32_t* agg_out) {
    MVS_TRACE();
    return recover_depth_maps_aggregated_host(__func__, n_seq, cam_off, cams, imgs, p, ap, out, level_out, sum_out, cnt_out, agg_out);
}

int mvs_recover_depth_maps_aggregated_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev,
                                          const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* ap, float* out_dev,
                                          int16_t* level_out_dev, int32_t* sum_out_dev, uint8_t* cnt_out_dev, int32_t* agg_out_dev, void* hip_stream) {
    MVS_TRACE();
    SgPlan pl;
    int rc = check_sg(__func__, n_seq, cam_off, cams, imgs_dev, p, ap, out_dev, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    SgRun run;
    if ((rc = run.launch(pl, cams, imgs_dev, out_dev, level_out_dev, sum_out_dev, cnt_out_dev, agg_out_dev, (hipStream_t)hip_stream))) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    return MVS_OK;
}

}  // extern "C"
