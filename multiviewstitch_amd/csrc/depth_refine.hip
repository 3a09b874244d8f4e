// depth_refine.hip — mvs_refine_depth_maps (include/mvs.h): the rendered inverse-depth rasters of every sequence taken back to the
// images, the stage DepthRecovery/DepthOptimizer names (RefineAllDepthMaps, DepthOptimizer.cpp:20-43; the frame window of
// RefineDepthMap, :45-63) and leaves without a body (DepthRefineCore is declared and never defined).  The rules are this library's
// definition, stated in include/mvs.h; their per-pixel part is depth_refine_rules.h, one body for this kernel and for host code.  The
// cost of rule 5 on the device — the grey launch, the squares launch, the LDS tile and DotSsd — is depth_cost_dev.h, shared with
// depth_recover.hip.
//
//   k_dr_refine  ONE launch for all frames of all sequences: a workgroup per DR_TILE x DR_TILE tile of the current frame, a thread per
//                pixel.  Frame and sequence come from blockIdx alone, so the cameras stay in scalar registers.  Every thread writes its
//                own pixel of every output and nothing else: no atomic, two runs give the same bytes.
#include "engine.h"
#include "trace.h"
#include "stitch.h"
#include "depth_cost_dev.h"
#include <cmath>

namespace {

__global__ __launch_bounds__(DR_TPB) void k_dr_refine(const float* __restrict__ depths, const uint8_t* __restrict__ grey, const uint32_t* __restrict__ sq,
                                                      const CamDev* __restrict__ cams, const DrSeq* __restrict__ seqs,
                                                      const int32_t* __restrict__ seq_of, int maxblk, DrRules q, float* __restrict__ out,
                                                      int8_t* __restrict__ k_out, int32_t* __restrict__ sum_out, uint8_t* __restrict__ cnt_out) {
    __shared__ DrTile lds;
    const int cam = blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const DrSeq s = seqs[seq_of[cam]];
    if (b >= s.tw * s.th) return;                                        // the whole workgroup: no barrier is skipped by a part of it
    const int f = cam - s.cam0, N = q.N;
    const int u0 = (b % s.tw) * DR_TILE, v0 = (b / s.tw) * DR_TILE;
    const int64_t npx = (int64_t)s.w * s.h;
    lds.load(grey + s.px_off + f * npx, s.w, s.h, u0, v0, N);
    const int tx = threadIdx.x % DR_TILE, ty = threadIdx.x / DR_TILE, u = u0 + tx, v = v0 + ty;
    if (u >= s.w || v >= s.h) return;
    const int64_t at = s.px_off + f * npx + (int64_t)v * s.w + u;
    const float d0 = depths[at];
    const DotSsd ssd = lds.ssd(grey, sq, s, at, tx, ty, N);
    const DrPixel r = dr_pixel(cams + s.cam0, s.n, f, u, v, d0, q, ssd);
    if (r.accepted) out[at] = (float)r.d;
    else ((uint32_t*)out)[at] = ((const uint32_t*)depths)[at];          // bit for bit, a NaN's payload included
    if (k_out) k_out[at] = (int8_t)r.k;
    if (sum_out) sum_out[at] = r.sum;
    if (cnt_out) cnt_out[at] = (uint8_t)r.cnt;
}

// what a call is made of, built by the argument checks on the host
struct DrPlan : DrSeqPlan {
    DrRules q;
};

int check_dr(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const void* imgs, const void* depths,
             const mvs_depth_refine_params* p, const void* out, DrPlan* pl) {
    if (!cam_off || !cams || !imgs || !depths || !p || !out) return bad(fn, "cam_off, cams, imgs, depths, params or out is NULL");
    if (n_seq < 1) return bad(fn, "need n_seq >= 1");
    int rc = check_offsets(fn, "cam_off", cam_off, n_seq);
    if (rc) return rc;
    if (!std::isfinite(p->dsp_min) || !std::isfinite(p->dsp_max) || !std::isfinite(p->rel_range) || !std::isfinite(p->ssd_err))
        return bad(fn, "a parameter is not finite");
    if (p->dsp_min <= 0.0 || p->dsp_min > p->dsp_max) return bad(fn, "need 0 < dsp_min <= dsp_max");
    if (p->rel_range <= 0.0 || p->rel_range >= 1.0) return bad(fn, "need 0 < rel_range < 1");
    if (p->ssd_err < 0.0) return bad(fn, "ssd_err is negative");
    if (p->ssd_win < 0 || p->ssd_win > DR_NMAX) return bad(fn, "ssd_win must lie in [0, 15]");
    if (p->ref_frm_count < 1 || p->ref_frm_count > DR_MAX_REFS + 1 || p->ref_frm_count % 2 == 0) return bad(fn, "ref_frm_count must be odd and lie in [1, 9]");
    if (p->steps < 1 || p->steps > 63) return bad(fn, "steps must lie in [1, 63]");
    if (p->flags & ~(int32_t)MVS_REFINE_SUBSTEP) return bad(fn, "unknown flag bits");
    if (out == depths) return bad(fn, "out must not alias depths");
    pl->q = DrRules{p->dsp_min, p->dsp_max, p->rel_range, p->ssd_err, p->ssd_win, p->ref_frm_count, p->steps, p->flags};
    return dr_plan_seqs(fn, n_seq, cam_off, cams, pl);
}

// grey pass, squares and refinement on device arrays, enqueued on s; the tables stay alive in the object until the caller has synchronised
struct DrRun {
    DrCost cost;
    int launch(const DrPlan& pl, const mvs_camera* cams, const uint8_t* imgs, const float* depths, float* out, int8_t* k_out, int32_t* sum_out,
               uint8_t* cnt_out, hipStream_t s) {
        int rc;
        if ((rc = cost.launch(pl, pl.q.N, cams, imgs, s))) return rc;
        k_dr_refine<<<DrCost::tiles(pl), dim3(DR_TPB), 0, s>>>(depths, cost.dgrey.as<uint8_t>(), cost.dsq.as<uint32_t>(), cost.dcam.as<CamDev>(),
                                                               cost.dseq.as<DrSeq>(), cost.dsof.as<int32_t>(), pl.maxblk, pl.q, out, k_out, sum_out, cnt_out);
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }
};

}  // namespace

// the host form under the name fn (mvs_refine_depth_maps, mvs_processor_refine_depths)
int refine_depth_maps_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                           const mvs_depth_refine_params* p, float* out, int8_t* k_out, int32_t* sum_out, uint8_t* cnt_out) {
    DrPlan pl;
    int rc = check_dr(fn, n_seq, cam_off, cams, imgs, depths, p, out, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    const size_t n = (size_t)pl.px;
    Scratch di, dd, dout, dk, dsum, dcnt;
    if ((rc = up(di, imgs, 3 * n)) || (rc = up(dd, depths, n)) || (rc = dout.alloc(sizeof(float) * n)) || (k_out && (rc = dk.alloc(n))) ||
        (sum_out && (rc = dsum.alloc(sizeof(int32_t) * n))) || (cnt_out && (rc = dcnt.alloc(n)))) return rc;
    DrRun run;
    if ((rc = run.launch(pl, cams, di.as<uint8_t>(), dd.as<float>(), dout.as<float>(), k_out ? dk.as<int8_t>() : nullptr,
                         sum_out ? dsum.as<int32_t>() : nullptr, cnt_out ? dcnt.as<uint8_t>() : nullptr, nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(out, dout, n))) return rc;
    if (k_out && (rc = down(k_out, dk, n))) return rc;
    if (sum_out && (rc = down(sum_out, dsum, n))) return rc;
    return cnt_out ? down(cnt_out, dcnt, n) : MVS_OK;
}

extern "C" {

void mvs_depth_refine_default_params(mvs_depth_refine_params* p) {
    if (!p) return;
    p->dsp_min = 0.0025; p->dsp_max = 0.3; p->rel_range = 0.04; p->ssd_err = 40.0;
    p->ssd_win = 7; p->ref_frm_count = 5; p->steps = 8; p->flags = MVS_REFINE_SUBSTEP;
}

int mvs_refine_depth_maps(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                          const mvs_depth_refine_params* p, float* out, int8_t* k_out, int32_t* sum_out, uint8_t* cnt_out) {
    MVS_TRACE();
    return refine_depth_maps_host(__func__, n_seq, cam_off, cams, imgs, depths, p, out, k_out, sum_out, cnt_out);
}

int mvs_refine_depth_maps_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev, const float* depths_dev,
                              const mvs_depth_refine_params* p, float* out_dev, int8_t* k_out_dev, int32_t* sum_out_dev, uint8_t* cnt_out_dev,
                              void* hip_stream) {
    MVS_TRACE();
    DrPlan pl;
    int rc = check_dr(__func__, n_seq, cam_off, cams, imgs_dev, depths_dev, p, out_dev, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    DrRun run;
    if ((rc = run.launch(pl, cams, imgs_dev, depths_dev, out_dev, k_out_dev, sum_out_dev, cnt_out_dev, (hipStream_t)hip_stream))) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    return MVS_OK;
}

}  // extern "C"
