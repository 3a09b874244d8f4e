// deform_host.h — what the host units of the deformation engine share (deform_*.cpp: the C-ABI of include/mvs.h, mvs_deform_*,
// the drop-in for class Deformation, R/Deformation/Deformation.h:224-252).  Internal to those units; engine.h stays the
// interface between the host layer and the kernels' launchers.
// Host orchestration only; every per-point / per-vertex operation is a HIP kernel.
#ifndef MVS_DEFORM_HOST_H_
#define MVS_DEFORM_HOST_H_
#include "engine.h"
#include "trace.h"
#include "knobs.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

// (none of this is part of the library's symbol table: the units of one layer call each other, nobody else does)
#pragma GCC visibility push(hidden)

// ---- deform_handle.cpp ----
int check_params(const mvs_deform_params* p);
int ready(mvs_deform_t h, const mvs_deform_params* p, bool need_target);
template <class T> int dmalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    return mvs_check_hip(hipMalloc((void**)p, n * sizeof(T)), "hipMalloc");
}
inline bool use_ras(const mvs_deform_s* h, const mvs_deform_params& p) { return h->has_ras && p.solver != MVS_SOLVER_CG; }
inline int ensure_nbr(mvs_deform_s* h, int nn) {
    // the node arena holds K * 64 neighbour slots (graph_k <= 63); the table in use is [K][nn]
    if (!h->d_nbr || nn < 1 || nn > 64) { mvs_set_error("no node set / graph_k out of range"); return MVS_E_STATE; }
    h->nbr_k = nn;
    return MVS_OK;
}

// ---- deform_timing.cpp ----
struct Tic { mvs_deform_s* h; const char* name; hipEvent_t a; };
bool timed(const mvs_deform_s* h, const char* name);
Tic  tic(mvs_deform_s* h, const char* name);
void toc(Tic& t, int launches);
void collect_timers(mvs_deform_s* h);
bool sample_room(mvs_deform_s* h, int64_t nslots);

// ---- deform_plan.cpp: the closed loop around the launch plans ----
// The stop criterion of a solve sits at STOP_AT * cg_tol: the sweep that finds its input at that level still runs (it
// cannot know) and normally improves it by another 10-20x, but near convergence the float32 / bfloat16 local corrections
// make the residual history noisy (a sweep may give back some of it in the ill-conditioned late regime of a long fit,
// scripts/pass_trace.py) — the factor 2 keeps the RESULT below cg_tol, which is what every solve is judged by.
#define STOP_AT MVS_KNOB("MVS_STOP_AT", 0.5, 0.01, 1.0)
constexpr int MAX_BATCH = 32;        // passes between two harvests, at most

struct CgPlan {                      // CG launches per ARAP iteration and where each solve's slots start
    int n[8];
    int64_t total_slots(int iters) const { int64_t t = 0; for (int i = 0; i < iters; ++i) t += n[i] + 2; return t; }
    int64_t offset(int it) const { return total_slots(it) * MVS_CG_SLOT; }
    int max(int iters) const { int m = 0; for (int i = 0; i < iters; ++i) m = std::max(m, n[i]); return m; }
};
struct RasPlan {                     // sweeps per ARAP iteration of the patch solver and where each solve's slots start
    int n[8];
    int64_t total(int iters) const { int64_t t = 0; for (int i = 0; i < iters; ++i) t += n[i]; return t; }
};
void    update_mix_state(mvs_deform_s* h, int arap_iters);
RasPlan probe_ras(const mvs_deform_s* h);
CgPlan  probe_cg(const mvs_deform_s* h, const mvs_deform_params& p);
int  ensure_ras_slots(mvs_deform_s* h, int arap_iters);
int  ensure_slots(mvs_deform_s* h, int arap_iters, const CgPlan& cg);
int  throttle(mvs_deform_s* h);
void peek_ring(mvs_deform_s* h, const mvs_deform_params& p, bool ras);
// after a sync: read the slots of the last pass's solves, fill stats, re-make the plans (CG or patch solver, as the handle runs)
int  harvest(mvs_deform_s* h, const mvs_deform_params& p, const CgPlan& plan, mvs_deform_stats* st);
// used != NULL: the plan the harvested pass ran with (a group's common plan) instead of the handle's own
int  harvest_ras(mvs_deform_s* h, const mvs_deform_params& p, mvs_deform_stats* st, const RasPlan* used = nullptr);

// what a call reports of the batches it harvested: the last batch's statistics, the verdict counters summed over all of them
struct BatchAcc {
    mvs_deform_stats st{};
    double worst = 0.0;
    int solves = 0, missed = 0, esc = 0;
    void add(const mvs_deform_stats& s) {
        st = s;
        worst = std::max(worst, s.worst_rel_residual_in_batch);
        solves += s.solves_in_batch; missed += s.unconverged_solves; esc |= s.escalated;
    }
    void finish(mvs_deform_stats* out, int outer_done) const {
        *out = st;
        out->outer_done = outer_done;
        out->worst_rel_residual_in_batch = worst; out->solves_in_batch = solves; out->unconverged_solves = missed; out->escalated = esc;
    }
};

// ---- deform_pass.cpp: the launch sequence of a pass ----
// the two heavy / mid lists of a handle alternate: the pair a pass with this flip fills and works off, and the other pair, whose
// counters it resets for the pass after it
struct AssocLists { int32_t *heavy, *heavy_next, *mid, *mid_next; };
AssocLists assoc_lists(const mvs_deform_s* h, int flip);
void enqueue_assoc_local(mvs_deform_s* h, const mvs_deform_params& p);
int  enqueue_solve(mvs_deform_s* h, const mvs_deform_params& p, const double* ctrl_src, bool graph_smooth, const CgPlan& plan, bool safe_local = false);

#pragma GCC visibility pop
#endif
