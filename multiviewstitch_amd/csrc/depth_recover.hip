// depth_recover.hip — mvs_recover_depth_maps (include/mvs.h): the first inverse-depth rasters DATA/_depth<i>.raw of every sequence from
// its images alone, a plane sweep over `levels` disparities of [dsp_min, dsp_max].  The reference reads these rasters
// (Processor::CheckConsistency, Processor.cpp:37-38) and has no code that writes them; the rules R1-R9 are this library's definition,
// stated in include/mvs.h.  Their per-pixel part is depth_recover_rules.h, one body for this kernel and for host code; the cost of R5 on
// the device — the grey launch, the squares launch, the LDS tile and DotSsd — is depth_cost_dev.h, shared with depth_refine.hip.
//
//   k_rc_sweep   ONE launch for all frames of all sequences: a workgroup per DR_TILE x DR_TILE tile of the current frame, a thread per
//                pixel, every level walked by that thread.  Frame and sequence come from blockIdx alone, so the cameras stay in scalar
//                registers.  Every thread writes its own pixel of every output and nothing else: no atomic, two runs give the same bytes.
#include "engine.h"
#include "trace.h"
#include "stitch.h"
#include "depth_recover_plan.h"

namespace {

__global__ __launch_bounds__(DR_TPB) void k_rc_sweep(const uint8_t* __restrict__ grey, const uint32_t* __restrict__ sq, const CamDev* __restrict__ cams,
                                                     const DrSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int maxblk, RcRules q,
                                                     float* __restrict__ out, int16_t* __restrict__ level_out, int32_t* __restrict__ sum_out,
                                                     uint8_t* __restrict__ cnt_out) {
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
    const DotSsd ssd = lds.ssd(grey, sq, s, at, tx, ty, N);
    const RcPixel r = rc_pixel(cams + s.cam0, s.n, f, u, v, q, ssd);
    out[at] = r.out;
    if (level_out) level_out[at] = (int16_t)r.level;
    if (sum_out) sum_out[at] = r.sum;
    if (cnt_out) cnt_out[at] = (uint8_t)r.cnt;
}

// grey pass, squares and sweep on device arrays, enqueued on s; the tables stay alive in the object until the caller has synchronised
struct RcRun {
    DrCost cost;
    int launch(const RcPlan& pl, const mvs_camera* cams, const uint8_t* imgs, float* out, int16_t* level_out, int32_t* sum_out, uint8_t* cnt_out,
               hipStream_t s) {
        int rc;
        if ((rc = cost.launch(pl, pl.q.N, cams, imgs, s))) return rc;
        k_rc_sweep<<<DrCost::tiles(pl), dim3(DR_TPB), 0, s>>>(cost.dgrey.as<uint8_t>(), cost.dsq.as<uint32_t>(), cost.dcam.as<CamDev>(), cost.dseq.as<DrSeq>(),
                                                              cost.dsof.as<int32_t>(), pl.maxblk, pl.q, out, level_out, sum_out, cnt_out);
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }
};

}  // namespace

// the host form under the name fn (mvs_recover_depth_maps, mvs_processor_recover_depths)
int recover_depth_maps_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                            const mvs_depth_recover_params* p, float* out, int16_t* level_out, int32_t* sum_out, uint8_t* cnt_out) {
    RcPlan pl;
    int rc = check_rc(fn, n_seq, cam_off, cams, imgs, p, out, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    const size_t n = (size_t)pl.px;
    Scratch di, dout, dl, dsum, dcnt;
    if ((rc = up(di, imgs, 3 * n)) || (rc = dout.alloc(sizeof(float) * n)) || (level_out && (rc = dl.alloc(sizeof(int16_t) * n))) ||
        (sum_out && (rc = dsum.alloc(sizeof(int32_t) * n))) || (cnt_out && (rc = dcnt.alloc(n)))) return rc;
    RcRun run;
    if ((rc = run.launch(pl, cams, di.as<uint8_t>(), dout.as<float>(), level_out ? dl.as<int16_t>() : nullptr, sum_out ? dsum.as<int32_t>() : nullptr,
                         cnt_out ? dcnt.as<uint8_t>() : nullptr, nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(out, dout, n))) return rc;
    if (level_out && (rc = down(level_out, dl, n))) return rc;
    if (sum_out && (rc = down(sum_out, dsum, n))) return rc;
    return cnt_out ? down(cnt_out, dcnt, n) : MVS_OK;
}

extern "C" {

void mvs_depth_recover_default_params(mvs_depth_recover_params* p) {
    if (!p) return;
    p->dsp_min = 0.0025; p->dsp_max = 0.3; p->ssd_err = 40.0; p->peak = 0.9;
    p->ssd_win = 7; p->ref_frm_count = 5; p->levels = 128; p->min_refs = 2; p->flags = MVS_RECOVER_SUBSTEP; p->reserved = 0;
}

int mvs_recover_depth_maps(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const mvs_depth_recover_params* p,
                           float* out, int16_t* level_out, int32_t* sum_out, uint8_t* cnt_out) {
    MVS_TRACE();
    return recover_depth_maps_host(__func__, n_seq, cam_off, cams, imgs, p, out, level_out, sum_out, cnt_out);
}

int mvs_recover_depth_maps_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev, const mvs_depth_recover_params* p,
                               float* out_dev, int16_t* level_out_dev, int32_t* sum_out_dev, uint8_t* cnt_out_dev, void* hip_stream) {
    MVS_TRACE();
    RcPlan pl;
    int rc = check_rc(__func__, n_seq, cam_off, cams, imgs_dev, p, out_dev, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    RcRun run;
    if ((rc = run.launch(pl, cams, imgs_dev, out_dev, level_out_dev, sum_out_dev, cnt_out_dev, (hipStream_t)hip_stream))) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    return MVS_OK;
}

}  // extern "C"
