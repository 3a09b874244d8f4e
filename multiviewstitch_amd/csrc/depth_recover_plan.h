// depth_recover_plan.h — the argument checks of mvs_recover_depth_maps and what they build, shared by depth_recover.hip and
// depth_sgm.hip (mvs_recover_depth_maps_aggregated checks everything the plain sweep checks).  Internal linkage, as depth_cost_dev.h.
#ifndef MVS_DEPTH_RECOVER_PLAN_H_
#define MVS_DEPTH_RECOVER_PLAN_H_
#include "depth_cost_dev.h"
#include "depth_recover_rules.h"
#include <cmath>

namespace {

// what a call is made of, built by the argument checks on the host
struct RcPlan : DrSeqPlan {
    RcRules q;
};

int check_rc(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const void* imgs, const mvs_depth_recover_params* p,
             const void* out, RcPlan* pl) {
    if (!cam_off || !cams || !imgs || !p || !out) return bad(fn, "cam_off, cams, imgs, params or out is NULL");
    if (n_seq < 1) return bad(fn, "need n_seq >= 1");
    int rc = check_offsets(fn, "cam_off", cam_off, n_seq);
    if (rc) return rc;
    if (!std::isfinite(p->dsp_min) || !std::isfinite(p->dsp_max) || !std::isfinite(p->ssd_err) || !std::isfinite(p->peak))
        return bad(fn, "a parameter is not finite");
    if (p->dsp_min <= 0.0 || p->dsp_min >= p->dsp_max) return bad(fn, "need 0 < dsp_min < dsp_max");
    if (p->ssd_err < 0.0) return bad(fn, "ssd_err is negative");
    if (!(p->peak > 0.0 && p->peak <= 1.0)) return bad(fn, "peak must lie in (0, 1]");
    if (p->ssd_win < 0 || p->ssd_win > DR_NMAX) return bad(fn, "ssd_win must lie in [0, 15]");
    if (p->ref_frm_count < 1 || p->ref_frm_count > DR_MAX_REFS + 1 || p->ref_frm_count % 2 == 0) return bad(fn, "ref_frm_count must be odd and lie in [1, 9]");
    if (p->levels < 2 || p->levels > 1024) return bad(fn, "levels must lie in [2, 1024]");
    if (p->min_refs < 1 || p->min_refs > DR_MAX_REFS) return bad(fn, "min_refs must lie in [1, 8]");
    if (p->flags & ~(int32_t)MVS_RECOVER_SUBSTEP) return bad(fn, "unknown flag bits");
    if (p->reserved != 0) return bad(fn, "reserved must be 0");
    pl->q = RcRules{p->dsp_min, p->dsp_max, p->ssd_err, p->peak, p->ssd_win, p->ref_frm_count, p->levels, p->min_refs, p->flags};
    return dr_plan_seqs(fn, n_seq, cam_off, cams, pl);
}

}  // namespace

#endif
