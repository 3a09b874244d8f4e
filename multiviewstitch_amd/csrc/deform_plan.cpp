// deform_plan.cpp — how many launches a solve gets and what the host learns from a pass: the launch plans of both solvers, the
// closed loop around them (throttle, peek_ring) and the harvests.
#include "deform_host.h"
#include <sched.h>

// How a solve ends.  The sweeps (CG iterations) of a solve stop themselves: the first one that finds its INPUT converged
// (the residual of a sweep's input is reduced by the NEXT launch) copies the result into both solution buffers and
// raises a flag, every later one returns at once (k_ras_sweep "fast skip").  The host therefore does not plan the
// number of sweeps a solve needs, it PROVISIONS: what the solve used last time plus RAS_SPARES — the device decides how
// many of them run.  A spare that is not needed costs a 5 us copy (the first) or a ~2.5 us skip (the others); a spare that
// IS needed (the mesh deforms, the system's conditioning moves) runs as a normal sweep and the residual ring tells the
// host, which restores the number of spares from the next pass it enqueues on (peek_ring).
constexpr int RAS_SPARES = 1;            // ... plus one per 8 sweeps a solve used (ras_spares)
static int ras_spares(int used) { return RAS_SPARES + used / 8; }
// (the stop criterion of a solve, STOP_AT * cg_tol: deform_host.h — the launches of a pass and of a group carry it)
// lowest bracket end the harvest goes to: with the step count capped at 32, a lower `a` only weakens the damping of every
// mode inside the bracket (1 / T_32 at a = 0.002 is 0.26, at 0.01 it is 0.02) — measured in the late regime of scripts/soak.py
#define RAS_A_FLOOR MVS_KNOB("MVS_RAS_FLOOR", 0.01, 0.001, 0.06)
constexpr double PEEK_AT = 1.0;          // CG: a solve that ends above PEEK_AT * cg_tol gets a longer plan inside the batch

// launches of a solve that has no history yet (first pass of a handle or of a node set): from the template pose 4-6 sweeps
// run at the usual node density, the launches left over return after one scalar load, and should the eight not suffice the
// last one keeps sweeping in the kernel (TAIL) — the DEVICE decides; round 2 probed such a solve in chunks of sweeps with a
// host look at the residual after each (five synchronisations per solve, 8 ms for the first outer iteration)
// (The later ARAP iterations of a pass start from the solution of the one before and need fewer sweeps: 6 5 4 4 4 ran of 8 8 8 8 8
//  on the metric workload's first pass with eight launches each, twelve of which returned at once.)
constexpr int RAS_FIRST_PLANS[8] = {7, 6, 5, 5, 5, 5, 5, 5};
constexpr int RAS_MAX_SWEEPS = 128;
// A solve whose plan has grown to this many launches has stalled sweeps behind it (healthy solves take 3-5 sweeps): its planned
// sweeps are launched as the mixing instantiation (schwarz.hip, RasMix).  A function of the plan, i.e. of the call sequence.
// Per HANDLE and sticky: in the regime where solves stall, WHICH of the five solves of a pass stalls changes from pass to pass (the
// later ARAP iterations start closer to their solution and often finish before the stalled mode matters); a solve that stalls
// with a short plan runs its extra sweeps in the last launch, unmixed, 15 us each (17-21 of them: 0.3 ms for one solve).  So once
// any plan reaches RAS_MIX_PLAN every solve of the handle gets mixing sweeps and a plan of at least RAS_MIX_PLAN launches (the
// ones a solve does not need return after one load, ~4 us each); back to lean sweeps after RAS_MIX_CALM passes in which every
// solve's need stayed at a healthy solve's length (<= RAS_MIX_OFF launches).
// (11, was 9 through round 3: the first solve of a pass of a small part — config 5's 13 K-vertex sub-meshes — runs 7-8 healthy sweeps,
//  and once it predicts cautiously in a fit's first passes (schwarz.hip, RAS_YOUNG_PASSES) its plan of "sweeps + spares" reached 9-10:
//  sixteen healthy handles switched to mixing sweeps and 45 launches per pass, 14 ms per outer iteration instead of 7.5)
#define RAS_MIX_PLAN ((int)MVS_KNOB("MVS_MIX_PLAN", 11, 2, 128))
constexpr int RAS_MIX_OFF = 7, RAS_MIX_CALM = 16;      // (healthy plans are 4-7 launches, a mixing solve's 8-12, a stalled one's 17+: config 4 went
                                                        //  on at a transient and, with "<= 5 for 64 passes", never came back: 45 launches for 20 sweeps)
void update_mix_state(mvs_deform_s* h, int arap_iters) {
    bool any_long = false, all_short = true;
    for (int it = 0; it < arap_iters; ++it) {
        if (h->ras_plan[it] >= RAS_MIX_PLAN) any_long = true;
        if (h->ras_plan[it] > RAS_MIX_OFF) all_short = false;
    }
    if (any_long) { h->ras_mix_any = 1; h->ras_mix_calm = 0; }
    else if (h->ras_mix_any) {
        if (!all_short) h->ras_mix_calm = 0;
        else if (++h->ras_mix_calm >= RAS_MIX_CALM) { h->ras_mix_any = 0; h->ras_mix_calm = 0; }
    }
}

RasPlan probe_ras(const mvs_deform_s* h) {
    RasPlan r;
    for (int i = 0; i < 8; ++i) r.n[i] = h->ras_plan[i] > 0 ? h->ras_plan[i] : RAS_FIRST_PLANS[i];
    if (h->ras_mix_any) for (int i = 0; i < 8; ++i) r.n[i] = std::max(r.n[i], RAS_MIX_PLAN);      // (update_mix_state)
    // experiment (scripts/host_bound.py): at most this many LAUNCHES per solve — the rest of the sweeps run inside the last one
    const int cap = h->dbg.plan_cap > 0 ? h->dbg.plan_cap : (int)MVS_KNOB("MVS_RAS_PLAN_CAP", 0, 0, 128);
    if (cap > 0) for (int i = 0; i < 8; ++i) r.n[i] = std::min(r.n[i], cap);
    return r;
}

int ensure_ras_slots(mvs_deform_s* h, int arap_iters) {
    // the sweep slots are part of the handle's table arena, sized once for the largest plan (RAS_MAX_SWEEPS sweeps of each of
    // 8 ARAP iterations, mesh_build): the host may add sweeps to a solve between two passes of a batch (peek_ring), and a
    // re-allocation would pull the buffer from under the passes still in flight
    if ((int64_t)RAS_MAX_SWEEPS * arap_iters > h->ras_slots_cap || !h->d_ras_slots) { mvs_set_error("sweep slots not provisioned"); return MVS_E_STATE; }
    return MVS_OK;
}

int ensure_slots(mvs_deform_s* h, int arap_iters, const CgPlan& cg) {
    int64_t need = cg.total_slots(arap_iters) * MVS_CG_SLOT;
    if (need > h->slots_cap) {
        need += need / 2;                                     // headroom: the host may lengthen a plan inside a batch (peek_ring)
        if (h->d_slots) (void)hipFree(h->d_slots);            // (hipFree waits for the device: passes in flight are safe)
        int rc = dmalloc(&h->d_slots, (size_t)need);
        if (rc) return rc;
        h->slots_cap = need;
    }
    return MVS_OK;
}

// ---- the closed loop around the launch plans (MVS_CTL_*, engine.h) ------------------------------------------------
// Every solve's result is judged on the device (true residual, k_arap_local -> judge_solve); the verdicts reach the host
// two ways: (a) the pinned mirror h_ctl, refreshed by the last kernel of every pass — read WITHOUT synchronising while a
// batch is being enqueued (throttle + peek_ring); (b) at a harvest, after the stream has been drained.
constexpr int THROTTLE_LAG = 3;          // passes the host may be ahead of the device inside a batch

// wait (spinning on the mirror, no HIP synchronisation) until the device is at most THROTTLE_LAG passes behind
int throttle(mvs_deform_s* h) {
    if (!h->h_ctl) return MVS_OK;
    for (unsigned spins = 0;; ++spins) {
        const uint64_t done = (uint64_t)h->h_ctl[MVS_CTL_SEQ];
        if (h->seq_enqueued <= done + THROTTLE_LAG) return MVS_OK;
        if ((spins & 0x3ff) == 0x3ff) {
            // a faulted kernel would leave the counter behind forever: ask the runtime now and then
            const hipError_t e = hipStreamQuery(h->stream);
            if (e == hipSuccess) return MVS_OK;                     // idle stream: nothing left to wait for
            if (e != hipErrorNotReady) return mvs_check_hip(e, "stream (throttle)");
            sched_yield();
        }
    }
}

// rows of the passes finalized since the last look.  Patch solver: a solve that used some of its spares gets them back
// (plan = sweeps it ran + RAS_SPARES) from the next pass enqueued on; CG: a solve that missed cg_tol gets a longer plan.
void peek_ring(mvs_deform_s* h, const mvs_deform_params& p, bool ras) {
    if (!h->h_ctl) return;
    // Only the passes the throttle has just waited for are looked at — enqueued - THROTTLE_LAG of them — not whatever else the
    // device has finished meanwhile: the plans are then a function of the call sequence, not of timing (every rank of a
    // sharded run re-plans alike; a run's launch counts are reproducible).
    uint64_t done = (uint64_t)h->h_ctl[MVS_CTL_SEQ];
    const uint64_t due = h->seq_enqueued > (uint64_t)THROTTLE_LAG ? h->seq_enqueued - THROTTLE_LAG : 0;
    if (done > due) done = due;
    uint64_t q = h->seq_peeked;
    if (q >= done) return;
    if (done > MVS_RING && q < done - MVS_RING) q = done - MVS_RING;
    const double tol2 = PEEK_AT * PEEK_AT * p.cg_tol * p.cg_tol;
    const bool plan_lowering = MVS_KNOB("MVS_PLAN_LOWER", 1, 0, 1) != 0.0;
    for (; q < done; ++q) {
        const volatile double* row = h->h_ctl + MVS_CTL_RING + (q % MVS_RING) * 8;
        const volatile double* used = h->h_ctl + MVS_CTL_USED + (q % MVS_RING) * 8;
        for (int it = 0; it < p.arap_iters; ++it) {
            const double rel2 = row[it];
            if (rel2 < 0.0) continue;                                   // the solve did not run
            int want = 0;
            if (ras) {
                if (h->ras_plan[it] <= 0) continue;
                const int u = (int)used[it];
                if (u != 0) {
                    const int ran = std::abs(u) + (u < 0 ? 1 : 0);
                    want = ran + ras_spares(ran);
                    // ... and a plan that has been more than generous for four passes in a row comes down to what they needed
                    // (plus the spare): right after a calibration or a harvest of a few passes the plans carry the first
                    // passes' needs, which fall quickly (the bench's window, passes 3-22: 27 launches for 19 sweeps that run)
                    int* hist = h->ras_hist[it];
                    if (h->ras_hist_n[it] == 4) { hist[0] = hist[1]; hist[1] = hist[2]; hist[2] = hist[3]; hist[3] = ran; }
                    else hist[h->ras_hist_n[it]++] = ran;
                    const int HN = (int)MVS_KNOB("MVS_PLAN_HIST", 4, 1, 4);
                    if (plan_lowering && h->ras_hist_n[it] >= HN && u > 0) {
                        int m = 0;
                        for (int k = h->ras_hist_n[it] - HN; k < h->ras_hist_n[it]; ++k) m = std::max(m, hist[k]);
                        const int low = m + ras_spares(m);
                        if (low < h->ras_plan[it] && want <= low) {
                            if (mvs_debug_level()) fprintf(stderr, "[mvs] pass %llu solve %d: plan %d -> %d (the last four passes ran <= %d sweeps)\n",
                                                                (unsigned long long)q, it, h->ras_plan[it], low, m);
                            h->ras_plan[it] = low;
                        }
                    }
                }
                if (rel2 > tol2) want = std::max(want, h->ras_plan[it] + ras_spares(h->ras_plan[it]) + 1);     // it missed although every sweep ran
                want = std::min(RAS_MAX_SWEEPS, want);
                if (want > h->ras_plan[it]) {
                    if (mvs_debug_level()) fprintf(stderr, "[mvs] pass %llu solve %d ran %d of %d sweeps (ended at %.2e of cg_tol): plan %d from pass %llu on\n",
                                                        (unsigned long long)q, it, std::abs(u), h->ras_plan[it], std::sqrt(rel2) / p.cg_tol, want, (unsigned long long)h->seq_enqueued);
                    h->ras_plan[it] = want;
                }
            } else if (h->cg_plan[it] > 0 && rel2 > tol2 && q >= h->bump_seq[it]) {
                h->cg_plan[it] = std::min(p.cg_max_iters, h->cg_plan[it] + std::max(2, h->cg_plan[it] / 8));
                h->bump_seq[it] = h->seq_enqueued;
            }
        }
    }
    h->seq_peeked = done;
}

// after the stream has been drained: the verdicts since the last harvest -> stats; resets the sticky part of the control block
namespace {
struct Judgement {
    double worst2 = 0.0, last_worst2 = 0.0; int solves = 0, missed = 0; bool esc = false; double last_row[8];
    int rows = 0; int used[MVS_RING][8];          // sweeps each solve ran in the passes since the last harvest (at most MVS_RING of them)
};
int read_judgement(mvs_deform_s* h, const mvs_deform_params& p, Judgement* j) {
    double ctl[MVS_CTL_SIZE];
    HIPCHK(hipMemcpyAsync(ctl, h->d_ctl, sizeof ctl, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    j->esc = ctl[MVS_CTL_ESC] != 0.0;
    for (int it = 0; it < 8; ++it)                             // a tail loop was abandoned since the last look: from now on a local-step launch of
        if (ctl[MVS_CTL_GAVEUP + it] > h->gaveup_seen[it]) {   // its own follows every solve of this handle (the chip is shared with somebody)
            h->gaveup_seen[it] = ctl[MVS_CTL_GAVEUP + it];
            h->saw_abandon = true;
        }
    if (mvs_debug_level()) fprintf(stderr, "[mvs] predicted stops: true / predicted residual (running maximum) %.2f\n", std::sqrt(std::max(1.0, ctl[MVS_CTL_PSAFE])));
    j->worst2 = ctl[MVS_CTL_WORST];
    j->missed = (int)ctl[MVS_CTL_MISSED];
    j->solves = (int)ctl[MVS_CTL_SOLVES];
    const double* row = ctl + MVS_CTL_RING + ((h->seq_enqueued + MVS_RING - 1) % MVS_RING) * 8;
    for (int it = 0; it < 8; ++it) { j->last_row[it] = row[it]; if (it < p.arap_iters && row[it] > j->last_worst2) j->last_worst2 = row[it]; }
    {
        const uint64_t since = std::min<uint64_t>(h->seq_enqueued - h->seq_harvested, MVS_RING);
        j->rows = (int)since;
        for (uint64_t q = 0; q < since; ++q) {
            const double* u = ctl + MVS_CTL_USED + ((h->seq_enqueued - 1 - q) % MVS_RING) * 8;
            for (int it = 0; it < 8; ++it) { const int v = (int)u[it]; j->used[q][it] = v < 0 ? 1 - v : v; }   // (no spare left: one more)
        }
        h->seq_harvested = h->seq_enqueued;
    }
    HIPCHK(hipMemsetAsync(h->d_ctl, 0, sizeof(double) * 4, h->stream));       // ESC, WORST, MISSED, SOLVES
    h->seq_peeked = h->seq_enqueued;
    return MVS_OK;
}
int judged_status(const Judgement& j, const mvs_deform_params& p) {
    if (j.missed == 0) return MVS_OK;
    mvs_set_error("%d of %d global solves ended above cg_tol = %.1e (worst relative residual %.3e)%s", j.missed, j.solves, p.cg_tol,
                  std::sqrt(j.worst2), j.esc ? "; the device switched the remaining solves to the strong local-solve coefficients" : "");
    return MVS_W_UNCONVERGED;
}

// What every harvest reads back behind its solver's own slots: the energies, the ARAP iterations that ran, the nodes' validity
// and the verdicts.  download() enqueues the copies and synchronises the stream ONCE (inside read_judgement); fill() is the
// part of the statistics that does not depend on the solver, and the end of a harvest.
struct PassReadback {
    std::vector<double> ered;
    int32_t info[8];
    std::vector<uint8_t> valid;
    Judgement jd;
    explicit PassReadback(const mvs_deform_s* h) : ered(MVS_ERED_SIZE), valid(h->K) {}
    int run() const { return info[0]; }
    int download(mvs_deform_s* h, const mvs_deform_params& p) {
        HIPCHK(hipMemcpyAsync(ered.data(), h->d_energy, sizeof(double) * MVS_ERED_SIZE, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(info, h->d_info, sizeof info, hipMemcpyDeviceToHost, h->stream));
        if (h->K) HIPCHK(hipMemcpyAsync(valid.data(), h->d_valid, (size_t)h->K, hipMemcpyDeviceToHost, h->stream));
        return read_judgement(h, p, &jd);                  // (synchronises the stream)
    }
    // cg_iters / launches / active: what the solver's own slots told
    mvs_deform_stats fill(mvs_deform_s* h, const mvs_deform_params& p, int cg_iters, int launches, int active, mvs_deform_stats* st) const {
        mvs_deform_stats out{};
        out.arap_iters_run = run();
        out.cg_iters = cg_iters;
        for (int i = 0; i < 8; ++i) out.energy[i] = i < p.arap_iters ? ered[MVS_ERED_FIN + i] : 0.0;
        out.cg_rel_residual = std::sqrt(std::max(0.0, jd.last_worst2));
        out.worst_rel_residual_in_batch = std::sqrt(std::max(0.0, jd.worst2));
        out.solves_in_batch = jd.solves;
        out.unconverged_solves = jd.missed;
        out.escalated = jd.esc ? 1 : 0;
        out.cg_launches = launches; out.cg_active = active;
        int nv = 0;
        for (uint8_t v : valid) nv += v;
        out.n_valid = nv;
        h->last = out;
        if (st) *st = out;
        collect_timers(h);
        return out;
    }
};

}  // namespace

// after a sync: read the CG slots of the last solve, fill stats, re-calibrate cg_iters
int harvest(mvs_deform_s* h, const mvs_deform_params& p, const CgPlan& plan, mvs_deform_stats* st) {
    if (use_ras(h, p)) return harvest_ras(h, p, st);
    const size_t n = (size_t)plan.total_slots(p.arap_iters) * MVS_CG_SLOT;
    std::vector<double> slots(n);
    PassReadback rb(h);
    HIPCHK(hipMemcpyAsync(slots.data(), h->d_slots, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int rc = rb.download(h, p);
    if (rc) return rc;
    const Judgement& jd = rb.jd;
    const int run = rb.run();
    const int nb = arap_grid_blocks(h->sell);
    int launches = 0, active = 0;
    bool all_conv = true;
    for (int it = 0; it < run; ++it) {
        const double* S = slots.data() + plan.offset(it);
        const int cg = plan.n[it];
        int first = -1;
        auto gamma_of = [&](int i, int c) {           // reduced by the consumer kernel for i < cg, folded here for i == cg
            if (i < cg) return S[(size_t)i * MVS_CG_SLOT + MVS_CG_FIN + 3 + c];
            double g = 0.0;
            for (int b = 0; b < nb; ++b) g += S[(size_t)i * MVS_CG_SLOT + c * MVS_NBMAX + b];
            return g;
        };
        for (int i = 0; i <= cg; ++i) {
            bool frozen = true;
            for (int c = 0; c < 3; ++c) {
                const double gam = gamma_of(i, c), bn = S[MVS_CG_FIN + 6 + c];
                if (gam > 0.0 && gam > STOP_AT * STOP_AT * p.cg_tol * p.cg_tol * bn) frozen = false;
            }
            if (frozen) { first = i; break; }
        }
        if (first < 0) { all_conv = false; h->cg_plan[it] = std::min(p.cg_max_iters, 2 * cg); first = cg; }
        else h->cg_plan[it] = std::min(p.cg_max_iters, first + first / 8 + 2);
        launches += cg; active += first;
        if (mvs_debug_level()) fprintf(stderr, "[mvs] arap it %d: CG frozen at %d of %d (gamma0 %.3e bn %.3e), true residual %.3e\n", it, first, cg, gamma_of(0, 0), S[MVS_CG_FIN + 6], std::sqrt(std::max(0.0, jd.last_row[it])));
    }
    for (int it = run; it < p.arap_iters; ++it)            // solves skipped by the energy stop rule keep a safe count
        if (h->cg_plan[it] == 0 || h->cg_iters == 0) h->cg_plan[it] = h->cg_plan[std::max(0, run - 1)];
    h->cg_iters = 1;
    const int cg = plan.max(p.arap_iters);
    const mvs_deform_stats out = rb.fill(h, p, cg, launches, active, st);
    if (!all_conv && cg >= p.cg_max_iters) {
        mvs_set_error("global solve did not reach cg_tol in cg_max_iters=%d (rel residual %.3e)", cg, out.worst_rel_residual_in_batch);
        return MVS_E_SOLVER;
    }
    return judged_status(jd, p);
}

// patch solver: read the sweep slots of the last solve, fill stats, re-plan the sweep counts.
// NOTE the plan used by the solve being harvested is probe_ras() of the state BEFORE this call.
// used != NULL: the plan the harvested pass ran with (a group's common plan) instead of the handle's own
int harvest_ras(mvs_deform_s* h, const mvs_deform_params& p, mvs_deform_stats* st, const RasPlan* used) {
    const RasPlan rp = used ? *used : probe_ras(h);
    const int ss = ras_slot_size(h), NP = h->ras.NP, NPpad = h->ras.NPpad;
    const size_t nslots = (size_t)rp.total(p.arap_iters);
    // per sweep only its 8 scalars (gamma[3] of its input, folded by the following sweep; bn[3]; idle flag; sweeps that ran)
    // travel to the host, plus the local step counts
    std::vector<double> fin(nslots * 8);
    std::vector<int32_t> iters(nslots * NP);
    PassReadback rb(h);
    HIPCHK(hipMemcpy2DAsync(fin.data(), 8 * sizeof(double), h->d_ras_slots + 3 * (size_t)NPpad, (size_t)ss * sizeof(double), 8 * sizeof(double), nslots,
                            hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(iters.data(), h->d_ras_iters, iters.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    int rc = rb.download(h, p);
    if (rc) return rc;
    const Judgement& jd = rb.jd;
    const int run = rb.run();
    const double tol2 = p.cg_tol * p.cg_tol;
    int launches = 0, active = 0, max_local = 0, worst_first = 0;
    bool all_conv = true;
    size_t slot = 0;
    for (int it = 0; it < p.arap_iters; ++it) {
        const int n = rp.n[it];
        if (it >= run) { slot += n; continue; }
        const double* F = fin.data() + (slot + n - 1) * 8;               // scalars of the solve's last sweep slot
        const double bn[3] = {F[3], F[4], F[5]};
        const bool idle = F[6] != 0.0;                                   // some sweep found the solve finished (spares were left)
        const int ran = (int)F[7];                                       // sweeps that did work, the confirming one included
        const double final2 = jd.last_row[it];                           // true residual of the result (local step)
        // gamma of the INPUT of sweep i, reduced on the device by sweep i+1 (valid for i < ran when spares were left)
        auto rel2_at = [&](int i) {
            double worst = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double g = fin[(slot + i) * 8 + c];
                if (g > 0.0 && bn[c] > 0.0) worst = std::max(worst, g / bn[c]);
                else if (g > 0.0) worst = INFINITY;
            }
            return worst;
        };
        for (int i = 0; i < n; ++i) {
            int mx = 0;
            for (int q = 0; q < NP; ++q) mx = std::max(mx, iters[(slot + i) * NP + q]);
            max_local += mx;
        }
        launches += n; active += ran;
        const bool ok = final2 >= 0.0 && final2 <= tol2;
        if (!ok) { all_conv = false; h->ras_plan[it] = std::min(RAS_MAX_SWEEPS, 2 * n); worst_first = std::max(worst_first, n); }
        else {
            // provision what the solve used — the most over the passes since the last harvest that the ring still holds, not
            // only the last one: in an ill-conditioned regime the need moves by several sweeps from pass to pass — plus
            // the spares (one more when it used every planned sweep: how many it needed is then not known)
            int most = ran + (idle ? 0 : 1);
            for (int q = 0; q < jd.rows; ++q) most = std::max(most, jd.used[q][it]);
            h->ras_plan[it] = std::min(RAS_MAX_SWEEPS, most + ras_spares(most));
            // (a mixing solve's 7-9 sweeps say nothing about the bracket: its stalled mode lies below any bracket and is taken
            //  out by the mixing — it neither lowers the bracket nor keeps it from drifting back to the default)
            if (!h->ras_mix_any) worst_first = std::max(worst_first, ran - 1);
        }
        if (mvs_debug_level()) {
            fprintf(stderr, "[mvs] arap it %d: %d of %d planned sweeps ran%s (true final residual %.3e) -> plan %d\n", it, ran, n, idle ? "" : " — no spare left",
                    std::sqrt(std::max(0.0, final2)), h->ras_plan[it]);
            if (mvs_debug_level() >= 2) {
                fprintf(stderr, "[mvs]   residual of each sweep's input:");
                for (int i = 0; i < std::min(n - 1, ran); ++i) fprintf(stderr, " %.2e", std::sqrt(rel2_at(i)));
                fprintf(stderr, "\n");
            }
        }
        slot += n;
    }
    {   // adapt the Chebyshev bracket of the local solves to what the sweeps showed: many sweeps (or a miss) mean
        // the smooth modes are under-damped -> lower the bracket and take more steps; very few sweeps -> drift back up
        double a0; int m0;
        ras_default_bracket(h, &a0, &m0);
        double a = h->ras_a > 0.0 ? h->ras_a : a0;
        if (!all_conv || jd.esc || worst_first > 9) {
            a = std::max(a / 3.0, RAS_A_FLOOR);
        } else if (worst_first <= 4 && a < a0) {
            a = std::min(a0, a * 1.5);
            for (int it = 0; it < run; ++it) h->ras_plan[it] = std::min(RAS_MAX_SWEEPS, h->ras_plan[it] + 2);   // the old plan was measured with stronger local solves
        }
        if (a != h->ras_a) { h->ras_a = a; h->ras_m = ras_steps_for(a); }
        if (mvs_debug_level()) fprintf(stderr, "[mvs] patch solver bracket a = %.4f, %d steps per sweep\n", h->ras_a, h->ras_m);
    }
    for (int it = run; it < p.arap_iters; ++it)            // solves skipped by the energy stop rule keep a safe count
        if (h->ras_plan[it] == 0) h->ras_plan[it] = h->ras_plan[std::max(0, run - 1)];
    // (a solve that ends above cg_tol with the plan at RAS_MAX_SWEEPS is reported like any other miss: MVS_W_UNCONVERGED.
    //  Round 1 switched the handle to CG here; CG's recurrence residual drifts in exactly the ill-conditioned
    //  systems that bring a handle to this point — scripts/soak.py cg — so it is no safer.)
    rb.fill(h, p, max_local, launches, active, st);        // max_local: local Chebyshev steps on the critical path (max over patches, summed over sweeps)
    h->cg_iters = std::max(h->cg_iters, 1);                // "calibrated": async solves allowed
    return judged_status(jd, p);
}

CgPlan probe_cg(const mvs_deform_s* h, const mvs_deform_params& p) {
    CgPlan c;
    for (int i = 0; i < 8; ++i)
        c.n[i] = (h->cg_iters > 0 && h->cg_plan[i] > 0) ? std::min(h->cg_plan[i], p.cg_max_iters) : std::min(p.cg_max_iters, 192);
    return c;
}
