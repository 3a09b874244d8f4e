// api_deform.cpp — C-ABI of the deformation engine (include/mvs.h, mvs_deform_*):
// the drop-in for class Deformation (R/Deformation/Deformation.h:224-252).
// Host orchestration only; every per-point / per-vertex operation is a HIP kernel.
#include "engine.h"
#include "trace.h"
#include "knobs.h"
#include "../../include/mvs_test.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <cstdlib>
#include <tuple>
#include <sched.h>

extern "C" {

void mvs_deform_default_params(mvs_deform_params* p) {
    if (!p) return;
    p->proj_len_err = 100.0; p->proj_dist_err = 100.0; p->min_cos = 0.1;
    p->max_result = 10000; p->top_k = 8; p->graph_k = 8; p->smooth_sweeps = 2;
    p->arap_iters = 5; p->arap_tol = 1e-4; p->cg_tol = 1e-8; p->cg_max_iters = 2000;
    p->update_normals = 0;
    p->solver = MVS_SOLVER_AUTO; p->reserved0 = 0;
}

}  // extern "C"

// ------------------------------------------------------------------ helpers ----
namespace {

template <class T> int dmalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    return mvs_check_hip(hipMalloc((void**)p, n * sizeof(T)), "hipMalloc");
}
template <class T> void dfree(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

int check_params(const mvs_deform_params* p) {
    if (!p) { mvs_set_error("params is NULL"); return MVS_E_INVALID_ARG; }
    if (p->top_k < 1 || p->top_k > 8 || p->graph_k < 0 || p->graph_k > 63 || p->smooth_sweeps < 0 ||
        p->arap_iters < 1 || p->arap_iters > 8 || p->cg_max_iters < 1 || !(p->cg_tol > 0)) {
        mvs_set_error("params out of range (top_k 1..8, graph_k 0..63, arap_iters 1..8, cg_tol > 0)");
        return MVS_E_INVALID_ARG;
    }
    return MVS_OK;
}

// ---- timing ----
hipEvent_t get_event(mvs_deform_s* h) {
    if (!h->event_pool.empty()) { hipEvent_t e = h->event_pool.back(); h->event_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
struct Tic { mvs_deform_s* h; const char* name; hipEvent_t a; };
// timing: 0 off, 1 every phase, 2 only the global-solve groups ("cg": the planned sweeps of a solve, "tail": its last launch; two
// events per group: +30 us and more per outer iteration of the metric workload, scripts/timing_overhead.py), 3 the planned sweeps
// of every EIGHTH pass (what bench.py keeps on inside its timed region — the sampled passes hold the same launch mix as the others)
bool timed(const mvs_deform_s* h, const char* name) {
    if (h->timing == 1) return true;
    const bool cg = std::strcmp(name, "cg") == 0, tail = std::strcmp(name, "tail") == 0;
    if (!cg && !tail) return false;
    // (an event pair costs ~4 us of stream time — the marker packets break the back-to-back dispatch of the launches around them:
    //  bench.py's timed region keeps only the pair around the planned sweeps of every EIGHTH pass, ~0.2 % of a step)
    return h->timing == 2 || (cg && h->timing == 3 && (h->seq_enqueued & 7) == 0);
}
Tic tic(mvs_deform_s* h, const char* name) {
    Tic t{h, name, nullptr};
    if (timed(h, name)) { t.a = get_event(h); (void)hipEventRecord(t.a, h->stream); }
    return t;
}
void toc(Tic& t, int launches) {
    if (!t.a) return;
    hipEvent_t b = get_event(t.h);
    (void)hipEventRecord(b, t.h->stream);
    t.h->pending.push_back({t.name, {t.a, b}});
    t.h->pending_launches[t.name] += launches;
}
void collect_timers(mvs_deform_s* h) {
    // (mode 3) the k-th "cg" bracket of the pending list is the k-th sampled solve: its launches that found the solve finished are
    // counted from the flags copied out behind its pass (the stream has been synchronised: the copies have landed), and the
    // bracket is also filed under its composition — "cg:a<active>:i<idle>": total ms, number of brackets — so that a caller
    // can separate the cost of an active launch from that of an idle one and from the bracket's own overhead (bench.py)
    size_t k_cg = 0, q = 0;
    for (auto& pr : h->pending) {
        float ms = 0;
        const bool okms = hipEventElapsedTime(&ms, pr.second.first, pr.second.second) == hipSuccess;
        if (okms) h->timers[pr.first].total_ms += ms;
        if (h->timing == 3 && pr.first == "cg" && k_cg < h->samples.size()) {
            while (q + 1 < h->sample_off.size() && (size_t)h->sample_pass_first[q + 1] <= k_cg) ++q;
            const mvs_deform_s::SweepSample& sm = h->samples[k_cg++];
            const double* F = h->h_sample + h->sample_off[q];
            int idle = 0;
            for (int i = 0; i < sm.n_a; ++i) if (F[(size_t)(sm.first + i) * 8 + 6] != 0.0) ++idle;
            h->timers["cg_idle"].launches += idle;
            char key[48];
            snprintf(key, sizeof key, "cg:a%d:i%d", sm.n_a - idle, idle);
            if (okms) { h->timers[key].total_ms += ms; h->timers[key].launches += 1; }
        }
        h->event_pool.push_back(pr.second.first);
        h->event_pool.push_back(pr.second.second);
    }
    h->pending.clear();
    for (auto& kv : h->pending_launches) h->timers[kv.first].launches += kv.second;
    h->pending_launches.clear();
    h->samples.clear(); h->sample_off.clear(); h->sample_pass_first.clear(); h->sample_used = 0;
}

void free_nodes(mvs_deform_s* h) {
    if (h->arena_nodes) { (void)hipFree(h->arena_nodes); h->arena_nodes = nullptr; }
    h->d_nodes = nullptr; h->d_nbr = nullptr; h->d_node_pts = nullptr; h->d_node_nrm = nullptr; h->d_ctrl_raw = nullptr;
    h->d_ctrl_a = nullptr; h->d_ctrl_b = nullptr; h->d_valid = nullptr; h->d_d2min = nullptr; h->d_counts = nullptr;
    h->d_records = nullptr; h->d_top_idx = nullptr; h->d_heavy = nullptr; h->d_heavy2 = nullptr;
    h->d_prev_d2 = nullptr; h->d_prev_node = nullptr; h->d_knn_ws = nullptr;
    h->d_near_prev = nullptr; h->d_lim = nullptr; h->d_mid = nullptr; h->d_mid2 = nullptr; h->d_ng_sync = nullptr;
    h->near_age = 0; h->graph_prev_nn = 0;
    h->prev_valid = false;
    h->d_ctrl_final = nullptr; h->K = 0; h->nbr_k = 0; h->h_nodes.clear();
    h->graph_ready_nn = 0; h->weights_ready = false; h->heavy_pending = nullptr;
}

// How a solve ends.  The sweeps (CG iterations) of a solve stop themselves: the first one that finds its INPUT converged
// (the residual of a sweep's input is reduced by the NEXT launch) copies the result into both solution buffers and
// raises a flag, every later one returns at once (k_ras_sweep "fast skip").  The host therefore does not plan the
// number of sweeps a solve needs, it PROVISIONS: what the solve used last time plus RAS_SPARES — the device decides how
// many of them run.  A spare that is not needed costs a 5 us copy (the first) or a ~2.5 us skip (the others); a spare that
// IS needed (the mesh deforms, the system's conditioning moves) runs as a normal sweep and the residual ring tells the
// host, which restores the number of spares from the next pass it enqueues on (peek_ring).
constexpr int RAS_SPARES = 1;            // ... plus one per 8 sweeps a solve used (ras_spares)
inline int ras_spares(int used) { return RAS_SPARES + used / 8; }
// The stop criterion of a solve sits at STOP_AT * cg_tol: the sweep that finds its input at that level still runs (it
// cannot know) and normally improves it by another 10-20x, but near convergence the float32 / bfloat16 local corrections
// make the residual history noisy (a sweep may give back some of it in the ill-conditioned late regime of a long fit,
// scripts/pass_trace.py) — the factor 2 keeps the RESULT below cg_tol, which is what every solve is judged by.
#define STOP_AT MVS_KNOB("MVS_STOP_AT", 0.5, 0.01, 1.0)
// lowest bracket end the harvest goes to: with the step count capped at 32, a lower `a` only weakens the damping of every
// mode inside the bracket (1 / T_32 at a = 0.002 is 0.26, at 0.01 it is 0.02) — measured in the late regime of scripts/soak.py
#define RAS_A_FLOOR MVS_KNOB("MVS_RAS_FLOOR", 0.01, 0.001, 0.06)
constexpr double PEEK_AT = 1.0;          // CG: a solve that ends above PEEK_AT * cg_tol gets a longer plan inside the batch

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
    const int cap = h->dbg_plan_cap > 0 ? h->dbg_plan_cap : (int)MVS_KNOB("MVS_RAS_PLAN_CAP", 0, 0, 128);
    if (cap > 0) for (int i = 0; i < 8; ++i) r.n[i] = std::min(r.n[i], cap);
    return r;
}
bool use_ras(const mvs_deform_s* h, const mvs_deform_params& p) { return h->has_ras && p.solver != MVS_SOLVER_CG; }

int ensure_ras_slots(mvs_deform_s* h, int arap_iters, const RasPlan& rp) {
    // the sweep slots are part of the handle's table arena, sized once for the largest plan (RAS_MAX_SWEEPS sweeps of each of
    // 8 ARAP iterations, mesh_build): the host may add sweeps to a solve between two passes of a batch (peek_ring), and a
    // re-allocation would pull the buffer from under the passes still in flight
    (void)rp;
    if ((int64_t)RAS_MAX_SWEEPS * arap_iters > h->ras_slots_cap || !h->d_ras_slots) { mvs_set_error("sweep slots not provisioned"); return MVS_E_STATE; }
    return MVS_OK;
}

int ensure_slots(mvs_deform_s* h, int arap_iters, const CgPlan& cg) {
    int64_t need = cg.total_slots(arap_iters) * MVS_CG_SLOT;
    if (need > h->slots_cap) {
        need += need / 2;                                     // headroom: the host may lengthen a plan inside a batch (peek_ring)
        dfree(h->d_slots);                                    // (hipFree waits for the device: passes in flight are safe)
        int rc = dmalloc(&h->d_slots, (size_t)need);
        if (rc) return rc;
        h->slots_cap = need;
    }
    return MVS_OK;
}

// association of the handle's nodes against the handle's (local) target, nranks = 1
static int ensure_nbr(mvs_deform_s* h, int nn) {
    // the node arena holds K * 64 neighbour slots (graph_k <= 63); the table in use is [K][nn]
    if (!h->d_nbr || nn < 1 || nn > 64) { mvs_set_error("no node set / graph_k out of range"); return MVS_E_STATE; }
    h->nbr_k = nn;
    return MVS_OK;
}

// (timing mode 3) room for one more sampled pass's slot scalars in the pinned buffer?  Allocated at the first sampled pass.
bool sample_room(mvs_deform_s* h, int64_t nslots) {
    if (!h->h_sample) {
        void* hp = nullptr;
        const size_t cap = (size_t)64 * 8 * 64;                              // 64 passes of 64 slots (a pass holds 20-40)
        if (hipHostMalloc(&hp, cap * sizeof(double), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        h->h_sample = (double*)hp; h->sample_cap = cap; h->sample_used = 0;
    }
    return h->sample_used + (size_t)nslots * 8 <= h->sample_cap;
}

void enqueue_assoc_local(mvs_deform_s* h, const mvs_deform_params& p) {
    Tic t = tic(h, "assoc");
    const int K = (int)h->K;
    int32_t* cur = h->heavy_flip ? h->d_heavy2 : h->d_heavy;
    int32_t* nxt = h->heavy_flip ? h->d_heavy : h->d_heavy2;
    int32_t* mcur = h->heavy_flip ? h->d_mid2 : h->d_mid;
    int32_t* mnxt = h->heavy_flip ? h->d_mid : h->d_mid2;
    h->heavy_flip ^= 1;
    // (the SECOND association of a fit still searches unbounded: the first deformation has moved the nodes by whole grid cells, the
    //  bounds are loose — 4 680 of 8 142 nodes of the metric workload came out as heavy, 380 us — while their true nearest points
    //  are a fraction of a cell away by then, which the shell walk finds at once)
    if (h->near_age >= 2 && h->grid.P > 0 && K > 0 && p.graph_k + 1 <= 16 && MVS_KNOB("MVS_ASSOC_BOUNDED", 1, 0, 1) != 0.0) {
        // Bounded pass (assoc.hip): the last association of this node set against this target left every node's nearest distance
        // (d_d2min) and position (d_near_prev).  Two launches: bounds + classes (+ the node grid of the graph search in the same
        // launch's first workgroup), then heavy / mid / near nodes, the graph queries and the cotangent weights side by side.
        const int nn = p.graph_k + 1;
        const bool graph_here = h->d_knn_ws != nullptr && knn_grid_is_single(K) && ensure_nbr(h, nn) == MVS_OK;
        const bool bounded_graph = graph_here && h->graph_prev_nn == nn && K >= nn;
        const bool w = graph_here && use_ras(h, p);
        // (the node grid: inside the second launch, beside the searches, when one of its workgroups can build it; else by the first)
        const bool build_in_all = graph_here && assoc_all_builds_grid(K) && MVS_KNOB("MVS_NG_IN_ALL", 1, 0, 1) != 0.0;
        launch_assoc_prep(h->grid, h->d_node_pts, K, h->d_d2min, h->d_near_prev, h->d_lim, cur, mcur, (graph_here && !build_in_all) ? h->d_knn_ws : nullptr, h->stream);
        launch_assoc_all(h->grid, h->d_node_pts, h->d_node_nrm, K, p, h->d_lim, h->d_d2min, h->d_records, h->d_counts, cur, mcur, nxt, mnxt, h->d_ctrl_raw,
                         h->d_valid, h->d_top_idx, nn, h->d_nbr, graph_here ? h->d_knn_ws : nullptr, bounded_graph, w ? &h->sell : nullptr, h->d_pts,
                         arap_grid_blocks(h->sell), h->stream, build_in_all ? h->d_ng_sync : nullptr, build_in_all ? ++h->ng_pass : 0);
        h->assoc_passes++;
        h->near_age++;
        h->graph_in_local = false; h->heavy_pending = nullptr;
        if (graph_here) { h->graph_ready_nn = nn; h->weights_ready = w; h->graph_prev_nn = nn; }
        toc(t, 2);
        return;
    }
    // unbounded pass (the first association of a fit): what the bounded passes start from is recorded behind it
    (void)hipMemsetAsync(mcur, 0, sizeof(int32_t), h->stream); (void)hipMemsetAsync(mnxt, 0, sizeof(int32_t), h->stream);
    if (K > 0) (void)hipMemcpyAsync(h->d_near_prev, h->d_node_pts, sizeof(double) * 3 * (size_t)K, hipMemcpyDeviceToDevice, h->stream);
    h->near_age = (K > 0 && h->grid.P > 0) ? h->near_age + 1 : 0;
    // the heavy-node pass shares a launch with the node-graph search of enqueue_solve when that search runs on the grid
    const bool defer = h->d_knn_ws != nullptr && p.graph_k + 1 <= 64;
    // the 9-NN graph of the nodes needs only their positions: its grid is built first and the queries ride with the nodes' own
    // searches (k_assoc_local); the heavy-node launch of enqueue_solve then carries the heavy nodes and the cotangent weights
    const int nn = p.graph_k + 1;
    const bool graph_here = defer && ensure_nbr(h, nn) == MVS_OK;
    if (graph_here) knn_grid_build(h->d_node_pts, K, h->d_knn_ws, h->stream);
    // The first association of a fit meets the template far from the scan: a third of the nodes have balls wider than 25 grid rows
    // (2 664 of 8 142 on the metric workload, ten rounds of the workgroup-per-node pass: 276 us) — up to 64 rows a single wave still
    // copes (one row per lane); from the second pass on ~220 nodes are left and the lower threshold keeps the slowest wave short
    // (0.7 % of a steady step).  Same results either way.
    const int heavy_rows = h->assoc_passes == 0 ? 64 : 0;
    h->assoc_passes++;
    launch_assoc_local(h->grid, h->d_node_pts, h->d_node_nrm, K, p, h->d_d2min, h->d_records, h->d_counts, cur, nxt, K, h->d_ctrl_raw,
                       h->d_valid, h->d_top_idx, h->stream, defer, nn, h->d_nbr, graph_here ? h->d_knn_ws : nullptr, heavy_rows);
    h->graph_in_local = graph_here;
    h->heavy_pending = defer ? cur : nullptr;
    toc(t, defer ? 1 : 2);
}


// graph smoothing (optional) + ARAP + geometry update.  ctrl_src: K*3 node targets.
// safe_local: behind every patch solve a k_arap_local launch of its own follows even when the solve's last launch performs the
// local step itself (fused mode) — it returns at once when that happened.  Callers that do not follow the solves (enqueue-only
// batches of several handles sharing the chip, where a tail loop may have to be abandoned) and handles that have seen an
// abandoned solve ask for it; a handle stepping on its own does not pay the extra launch.
int enqueue_solve(mvs_deform_s* h, const mvs_deform_params& p, const double* ctrl_src, bool graph_smooth, const CgPlan& plan, bool safe_local = false) {
    hipStream_t s = h->stream;
    const int K = (int)h->K, V = (int)h->V;
    const int slot = (int)(h->seq_enqueued % MVS_RING);          // this pass's row of the residual ring (MVS_CTL_RING)
    double* host_ctl = const_cast<double*>(h->h_ctl);
    const double* ctrl = ctrl_src;
    bool weights_done = false;
    RasSmooth last_sweep{nullptr, nullptr, 0, nullptr};
    if (graph_smooth) {
        const int nn = p.graph_k + 1;
        int rc = ensure_nbr(h, nn);
        if (rc) return rc;
        int first_sweep = 0;
        {                                                                                       // Deformation.cpp:359
            Tic t = tic(h, "graph");
            if (h->graph_ready_nn == nn) {
                // sharded step: the graph (and the weights) came with the heavy-node pass of mvs_deform_assoc_select
                weights_done = h->weights_ready && use_ras(h, p);
                toc(t, 0);
            } else if (h->d_knn_ws && h->heavy_pending) {
                // single-rank iteration: the deferred heavy nodes of the association and the graph queries in one launch
                // (the node targets are complete only after it: every smoothing sweep is a k_smooth launch)
                if (!h->graph_in_local) knn_grid_build(h->d_node_pts, K, h->d_knn_ws, s);
                // ... and, for the patch solver, the cotangent weights (they need the rest geometry only; the start of the
                // solve, which needs the smoothed targets, moves into k_ras_prepare)
                weights_done = use_ras(h, p);
                launch_assoc_heavy_knn(h->grid, h->d_node_pts, h->d_node_nrm, K, p, h->d_d2min, h->d_records, h->d_counts, h->heavy_pending, K,
                                       h->d_ctrl_raw, h->d_valid, h->d_top_idx, nn, h->d_nbr, h->d_knn_ws, s,
                                       weights_done ? &h->sell : nullptr, h->d_pts, arap_grid_blocks(h->sell), !h->graph_in_local);
                h->heavy_pending = nullptr; h->graph_in_local = false;
                toc(t, knn_grid_launches(K));
            } else if (h->d_knn_ws) {
                // the grid kNN also performs the first smoothing sweep (its wave holds the neighbour list)
                const bool fuse = p.smooth_sweeps > 0;
                launch_knn_grid(h->d_node_pts, K, nn, h->d_nbr, h->d_knn_ws, s, fuse ? ctrl : nullptr, fuse ? h->d_ctrl_a : nullptr);
                if (fuse) { ctrl = h->d_ctrl_a; first_sweep = 1; }
                toc(t, knn_grid_launches(K));
            } else { launch_knn(h->d_node_pts, K, nn, h->d_nbr, s); toc(t, 1); }
        }
        h->graph_prev_nn = nn;               // d_nbr holds this pass's complete graph: the bound of the next pass's graph queries
        Tic t = tic(h, "smooth");
        double* bufs[2] = {h->d_ctrl_a, h->d_ctrl_b};
        // (patch-solver iteration: the last sweep is done by k_ras_prepare, node by node, as it starts the solve)
        const int by_prepare = (weights_done && p.smooth_sweeps > first_sweep) ? 1 : 0;
        for (int sw = first_sweep; sw < p.smooth_sweeps - by_prepare; ++sw) {                     // :362-381
            launch_smooth(h->d_node_pts, ctrl, h->d_nbr, nn, K, bufs[sw & 1], s);
            ctrl = bufs[sw & 1];
        }
        toc(t, p.smooth_sweeps - first_sweep - by_prepare);
        if (by_prepare) {
            double* out = bufs[(p.smooth_sweeps - 1) & 1];
            last_sweep = RasSmooth{h->d_node_pts, h->d_nbr, nn, out};
            h->d_ctrl_final = out;
        }
    }
    if (!last_sweep.out) h->d_ctrl_final = const_cast<double*>(ctrl);
    const bool ras = use_ras(h, p);
    if (ras) update_mix_state(h, p.arap_iters);
    const RasPlan rp = probe_ras(h);
    int rc = ras ? ensure_ras_slots(h, p.arap_iters, rp) : ensure_slots(h, p.arap_iters, plan);
    if (rc) return rc;
    {
        Tic t = tic(h, "weights");
        if (weights_done) {
            launch_ras_prepare(h, s, ctrl, last_sweep);                                                   // set_target_position :383-392
            toc(t, 1);
        } else {
            launch_cot_weights(h->sell, h->d_pts, ras ? nullptr : h->d_coef, ctrl, h->d_sol, h->d_rot, s);   // preprocess() :393 + set_target_position :383-392
            if (ras) launch_ras_prepare(h, s);
            toc(t, 2);
        }
    }
    double* x_cur = h->d_sol;            // the patch solver ping-pongs between d_sol and d_ras_x2
    int64_t ras_slot = 0;
    // fused mode: the last planned launch of every solve ends with the ARAP local step on its patches' owned rows (schwarz.hip);
    // nl = partial sums per reduction the local step leaves, whoever performs it
    const bool fused = ras && ras_can_fuse_local(h);
    if (h->saw_abandon) safe_local = true;
    const int nl = ras ? ras_local_parts(h) : 0;
    const int demand_local = (fused && !safe_local) ? 1 : 0;          // the judge of a solve insists that its fused local step ran
    const double* prev_scal = nullptr;   // the 8 scalars of the last sweep slot of the previous solve (idle flag, sweeps that ran)
    const bool sampling = ras && h->timing == 3 && timed(h, "cg") && sample_room(h, rp.total(p.arap_iters));
    if (sampling) h->sample_pass_first.push_back((int)h->samples.size());
    for (int it = 0; ras && it < p.arap_iters; ++it) {
        {
            Tic t = tic(h, "rhs");
            launch_arap_rhs(h->sell, h->d_pts, x_cur, h->d_rot, it, p.arap_tol, h->d_energy, nullptr, nullptr, h->d_ras_b, p.cg_tol, h->d_ctl, slot, prev_scal, h->d_bar, h->d_bpure, s,
                            nl, demand_local);
            toc(t, 1);
        }
        {
            Tic t = (h->timing == 3 && !sampling) ? Tic{h, "cg", nullptr} : tic(h, "cg");      // (mode 3 times exactly the sampled brackets)
            const int ss = ras_slot_size(h);
            auto sweep = [&](int i, bool last) {
                double* x_next = x_cur == h->d_sol ? h->d_ras_x2 : h->d_sol;
                double* cur = h->d_ras_slots + (size_t)ras_slot * ss;
                // the last planned sweep of a solve is a TAIL launch: should the plan turn out too short it keeps sweeping in
                // the kernel (its extra sweeps' partial sums go to the solve's tail slots)
                launch_ras_sweep(h, h->d_ras_b, x_cur, x_next, it, p.arap_tol, i, p.cg_tol, STOP_AT, i > 0 ? cur - ss : nullptr, cur,
                                 h->d_ras_iters + (size_t)ras_slot * h->ras.NP, s, last ? h->d_ras_tail + (size_t)it * RAS_TAIL_MAX * ss : nullptr, fused,
                                 h->ras_mix_any != 0);
                x_cur = x_next;
                ++ras_slot;
            };
            // ("cg" = the planned sweeps, "tail" = the solve's last launch — in fused mode the deciding launch + the local step)
            // Sampled passes of timing mode 3: which of the bracketed launches did work is READ BACK (the idle flags of this pass's
            // sweep slots are copied out behind the pass); collect_timers files every bracket under its composition.
            const int planned = rp.n[it] - 1;
            if (sampling) h->samples.push_back({(int)ras_slot, planned, 0});
            for (int i = 0; i < planned; ++i) sweep(i, false);
            toc(t, planned);
            Tic tl = tic(h, "tail");
            sweep(rp.n[it] - 1, true);
            toc(tl, 1);
            prev_scal = h->d_ras_slots + (size_t)(ras_slot - 1) * ss + 3 * (size_t)h->ras.NPpad;
        }
        if (!fused || safe_local) {
            Tic t = tic(h, "local");
            launch_arap_local(h->sell, h->d_pts, x_cur, it, p.arap_tol, h->d_energy, h->d_rot, h->d_bpure, s, fused ? h->d_ctl : nullptr, nl);
            toc(t, 1);
        }
    }
    for (int it = 0; !ras && it < p.arap_iters; ++it) {                                           // deform(5, 1e-4), :398
        double* slots = h->d_slots + plan.offset(it);
        const int cg = plan.n[it];
        {
            Tic t = tic(h, "rhs");
            launch_arap_rhs(h->sell, h->d_pts, h->d_sol, h->d_rot, it, p.arap_tol, h->d_energy, h->d_rws[0], h->d_p, h->d_ras_b, p.cg_tol, h->d_ctl, slot, nullptr, nullptr, h->d_bpure, s);
            launch_cg_w0(h->sell, h->d_coef, it, p.arap_tol, h->d_energy, h->d_rws[0], slots, s);
            toc(t, 2);
        }
        {
            Tic t = tic(h, "cg");
            for (int i = 0; i < cg; ++i) {
                const int a = i & 1, b = a ^ 1;
                launch_cg_iter(h->sell, h->d_coef, it, p.arap_tol, h->d_energy, i, STOP_AT * p.cg_tol, slots, slots + (size_t)i * MVS_CG_SLOT,
                               slots + (size_t)(i + 1) * MVS_CG_SLOT, h->d_rws[a], h->d_rws[b], h->d_p, h->d_sol, s);
            }
            toc(t, cg);
        }
        { Tic t = tic(h, "local"); launch_arap_local(h->sell, h->d_pts, h->d_sol, it, p.arap_tol, h->d_energy, h->d_rot, h->d_bpure, s, nullptr, 0); toc(t, 1); }
    }
    Tic t = tic(h, "finalize");
    int n = 1;
    if (p.update_normals) {              // the node normals change too: separate gather after the normals kernel
        launch_arap_finalize(h->sell, p.arap_iters, p.arap_tol, h->d_energy, x_cur, h->d_pts, h->d_info, nullptr, nullptr, nullptr, p.cg_tol, h->d_ctl, slot, host_ctl, prev_scal, s, nl, demand_local, (double)(h->seq_enqueued + 1));   // :400
        launch_vertex_normals(h->d_pts, h->d_faces, h->d_vf_ptr, h->d_vf, V, h->d_nrm, s);
        launch_gather_nodes(h->d_pts, h->d_nrm, h->d_nodes, K, h->d_node_pts, h->d_node_nrm, s);
        n = 3;
    } else {
        launch_arap_finalize(h->sell, p.arap_iters, p.arap_tol, h->d_energy, x_cur, h->d_pts, h->d_info, h->d_nrm, h->d_node_pts, h->d_node_nrm, p.cg_tol, h->d_ctl, slot, host_ctl, prev_scal, s, nl, demand_local, (double)(h->seq_enqueued + 1));
    }
    toc(t, n);
    if (sampling) {      // the 8 scalars of every sweep slot of this pass -> pinned memory (a few KB, every eighth pass)
        const int ss = ras_slot_size(h);
        const size_t nslots = (size_t)rp.total(p.arap_iters);
        h->sample_off.push_back(h->sample_used);
        (void)hipMemcpy2DAsync(h->h_sample + h->sample_used, 8 * sizeof(double), h->d_ras_slots + 3 * (size_t)h->ras.NPpad, (size_t)ss * sizeof(double),
                               8 * sizeof(double), nslots, hipMemcpyDeviceToHost, s);
        h->sample_used += nslots * 8;
    }
    (void)V;
    h->graph_ready_nn = 0; h->weights_ready = false;     // the nodes have moved
    h->seq_enqueued++;
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
void fill_judgement(const Judgement& j, mvs_deform_stats* out) {
    out->cg_rel_residual = std::sqrt(std::max(0.0, j.last_worst2));
    out->worst_rel_residual_in_batch = std::sqrt(std::max(0.0, j.worst2));
    out->solves_in_batch = j.solves;
    out->unconverged_solves = j.missed;
    out->escalated = j.esc ? 1 : 0;
}
int judged_status(const Judgement& j, const mvs_deform_params& p) {
    if (j.missed == 0) return MVS_OK;
    mvs_set_error("%d of %d global solves ended above cg_tol = %.1e (worst relative residual %.3e)%s", j.missed, j.solves, p.cg_tol,
                  std::sqrt(j.worst2), j.esc ? "; the device switched the remaining solves to the strong local-solve coefficients" : "");
    return MVS_W_UNCONVERGED;
}

// after a sync: read the CG slots of the last solve, fill stats, re-calibrate cg_iters
int harvest_ras(mvs_deform_s* h, const mvs_deform_params& p, mvs_deform_stats* st, bool* converged, const RasPlan* used = nullptr);

int harvest(mvs_deform_s* h, const mvs_deform_params& p, const CgPlan& plan, mvs_deform_stats* st, bool* converged) {
    if (use_ras(h, p)) return harvest_ras(h, p, st, converged);
    const size_t n = (size_t)plan.total_slots(p.arap_iters) * MVS_CG_SLOT;
    std::vector<double> slots(n);
    std::vector<double> ered(MVS_ERED_SIZE);
    int32_t info[8];
    HIPCHK(hipMemcpyAsync(slots.data(), h->d_slots, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ered.data(), h->d_energy, sizeof(double) * MVS_ERED_SIZE, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(info, h->d_info, sizeof info, hipMemcpyDeviceToHost, h->stream));
    std::vector<uint8_t> valid(h->K);
    if (h->K) HIPCHK(hipMemcpyAsync(valid.data(), h->d_valid, (size_t)h->K, hipMemcpyDeviceToHost, h->stream));
    Judgement jd;
    int rc = read_judgement(h, p, &jd);                    // (synchronises the stream)
    if (rc) return rc;
    const int run = info[0];
    const int nb = arap_grid_blocks(h->sell);
    int need = 0, launches = 0, active = 0;
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
        need = std::max(need, first);
        launches += cg; active += first;
        if (mvs_debug_level()) fprintf(stderr, "[mvs] arap it %d: CG frozen at %d of %d (gamma0 %.3e bn %.3e), true residual %.3e\n", it, first, cg, gamma_of(0, 0), S[MVS_CG_FIN + 6], std::sqrt(std::max(0.0, jd.last_row[it])));
    }
    if (converged) *converged = all_conv && jd.missed == 0;
    for (int it = run; it < p.arap_iters; ++it)            // solves skipped by the energy stop rule keep a safe count
        if (h->cg_plan[it] == 0 || h->cg_iters == 0) h->cg_plan[it] = h->cg_plan[std::max(0, run - 1)];
    h->cg_iters = 1;
    const int cg = plan.max(p.arap_iters);
    (void)need;
    mvs_deform_stats out{};
    out.arap_iters_run = run;
    out.cg_iters = cg;
    for (int i = 0; i < 8; ++i) out.energy[i] = i < p.arap_iters ? ered[MVS_ERED_FIN + i] : 0.0;
    fill_judgement(jd, &out);
    out.cg_launches = launches; out.cg_active = active;
    int nv = 0;
    for (uint8_t v : valid) nv += v;
    out.n_valid = nv;
    h->last = out;
    if (st) *st = out;
    collect_timers(h);
    if (!all_conv && cg >= p.cg_max_iters) {
        mvs_set_error("global solve did not reach cg_tol in cg_max_iters=%d (rel residual %.3e)", cg, out.worst_rel_residual_in_batch);
        return MVS_E_SOLVER;
    }
    return judged_status(jd, p);
}

// patch solver: read the sweep slots of the last solve, fill stats, re-plan the sweep counts.
// NOTE the plan used by the solve being harvested is probe_ras() of the state BEFORE this call.
// used != NULL: the plan the harvested pass ran with (a group's common plan) instead of the handle's own
int harvest_ras(mvs_deform_s* h, const mvs_deform_params& p, mvs_deform_stats* st, bool* converged, const RasPlan* used) {
    const RasPlan rp = used ? *used : probe_ras(h);
    const int ss = ras_slot_size(h), NP = h->ras.NP, NPpad = h->ras.NPpad;
    const size_t nslots = (size_t)rp.total(p.arap_iters);
    // per sweep only its 8 scalars (gamma[3] of its input, folded by the following sweep; bn[3]; idle flag; sweeps that ran)
    // travel to the host, plus the local step counts
    std::vector<double> fin(nslots * 8), ered(MVS_ERED_SIZE);
    std::vector<int32_t> iters(nslots * NP);
    int32_t info[8];
    HIPCHK(hipMemcpy2DAsync(fin.data(), 8 * sizeof(double), h->d_ras_slots + 3 * (size_t)NPpad, (size_t)ss * sizeof(double), 8 * sizeof(double), nslots,
                            hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(iters.data(), h->d_ras_iters, iters.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ered.data(), h->d_energy, sizeof(double) * MVS_ERED_SIZE, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(info, h->d_info, sizeof info, hipMemcpyDeviceToHost, h->stream));
    std::vector<uint8_t> valid(h->K);
    if (h->K) HIPCHK(hipMemcpyAsync(valid.data(), h->d_valid, (size_t)h->K, hipMemcpyDeviceToHost, h->stream));
    Judgement jd;
    int rc = read_judgement(h, p, &jd);                    // (synchronises the stream)
    if (rc) return rc;
    const int run = info[0];
    const double tol2 = p.cg_tol * p.cg_tol;
    int launches = 0, active = 0, max_local = 0, max_plan = 0, worst_first = 0;
    bool all_conv = true;
    size_t slot = 0;
    for (int it = 0; it < p.arap_iters; ++it) {
        const int n = rp.n[it];
        max_plan = std::max(max_plan, n);
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
    if (converged) *converged = all_conv && jd.missed == 0;
    mvs_deform_stats out{};
    out.arap_iters_run = run;
    out.cg_iters = max_local;                              // local Chebyshev steps on the critical path (max over patches, summed over sweeps)
    for (int i = 0; i < 8; ++i) out.energy[i] = i < p.arap_iters ? ered[MVS_ERED_FIN + i] : 0.0;
    fill_judgement(jd, &out);
    out.cg_launches = launches; out.cg_active = active;
    int nv = 0;
    for (uint8_t v : valid) nv += v;
    out.n_valid = nv;
    h->last = out;
    if (st) *st = out;
    collect_timers(h);
    (void)max_plan;     // (a solve that ends above cg_tol with the plan at RAS_MAX_SWEEPS is reported like any other miss: MVS_W_UNCONVERGED.
                        //  Round 1 switched the handle to CG here; CG's recurrence residual drifts in exactly the ill-conditioned
                        //  systems that bring a handle to this point — scripts/soak.py cg — so it is no safer.)
    h->cg_iters = std::max(h->cg_iters, 1);                // "calibrated": async solves allowed
    return judged_status(jd, p);
}

CgPlan probe_cg(const mvs_deform_s* h, const mvs_deform_params& p) {
    CgPlan c;
    for (int i = 0; i < 8; ++i)
        c.n[i] = (h->cg_iters > 0 && h->cg_plan[i] > 0) ? std::min(h->cg_plan[i], p.cg_max_iters) : std::min(p.cg_max_iters, 192);
    return c;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------- create ----
// Deformation::Deformation(points, normals, facets), Deformation.cpp:29-46: the mesh is checked and every table the solvers
// need is built ON THE DEVICE (meshbuild.hip) — two allocations, three uploads, one synchronisation.
int mvs_deform_create(int64_t V, const double* points, const double* normals, int64_t F, const int32_t* faces,
                      mvs_deform_t* out) {
    MVS_TRACE();
    if (!out) { mvs_set_error("out is NULL"); return MVS_E_INVALID_ARG; }
    *out = nullptr;
    if (V <= 0 || F < 0 || !points || !normals || (F > 0 && !faces) || V > 0x7ffffff0LL || F > 0x2aaaaaa0LL) {
        mvs_set_error("bad mesh arguments"); return MVS_E_INVALID_ARG;
    }
    const auto t_c0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (mvs_debug_level()) fprintf(stderr, "[mvs] create (api): %s at %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_c0).count()); };
    int rc = need_device();
    if (rc) return rc;
    const int dev = mvs_current_device();
    mvs_preload(dev);
    lap("device");
    mvs_deform_s* h = new mvs_deform_s;
    h->device = dev; h->V = V; h->F = F;
#define TRY(x) do { rc = (x); if (rc) { mvs_deform_destroy(h); return rc; } } while (0)
    TRY(stream_acquire(dev, &h->own_stream));
    h->stream = h->own_stream;
    lap("stream");
    {   // pinned, host-coherent mirror of the control block: the last kernel of every pass writes it, the host reads it
        // without synchronising (throttle / peek_ring)
        void* hp = nullptr;
        TRY(mvs_check_hip(hipHostMalloc(&hp, sizeof(double) * MVS_CTL_SIZE, hipHostMallocCoherent | hipHostMallocMapped), "hipHostMalloc"));
        std::memset(hp, 0, sizeof(double) * MVS_CTL_SIZE);
        h->h_ctl = (volatile double*)hp;
    }
    lap("pinned mirror");
    TRY(mesh_build(h, points, normals, faces));
    lap("mesh_build");
#undef TRY
    *out = h;
    return MVS_OK;
}

int mvs_deform_destroy(mvs_deform_t h) {
    MVS_TRACE();
    if (!h) return MVS_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_nodes(h);
    for (void* a : {h->arena_mesh, h->arena_tab, h->arena_target, h->arena_probe}) if (a) (void)hipFree(a);
    dfree(h->d_slots);
    dfree(h->d_cheb);
    if (h->d_sh) { (void)hipFree(h->d_sh); h->d_sh = nullptr; }
    if (h->h_ctl) { (void)hipHostFree((void*)h->h_ctl); h->h_ctl = nullptr; }
    if (h->h_sample) { (void)hipHostFree(h->h_sample); h->h_sample = nullptr; }
    for (auto& pr : h->pending) { (void)hipEventDestroy(pr.second.first); (void)hipEventDestroy(pr.second.second); }
    for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
    if (h->own_stream) stream_release(h->device, h->own_stream);
    delete h;
    return MVS_OK;
}

// -------------------------------------------------------------------- nodes ----
// device side of a node set (indices validated by the caller): ONE allocation for the 17 per-node arrays
static int install_nodes(mvs_deform_s* h, const int32_t* vertex_idx, int64_t K) {
    free_nodes(h);
    h->K = K;
    h->h_nodes.assign(vertex_idx, vertex_idx + K);
    const size_t ws_bytes = K >= 1024 ? knn_grid_ws_bytes((int)K) : 0;     // small graphs: brute force
    auto lay = [&](Arena& a) {
        h->d_heavy = a.take<int32_t>((size_t)K + 1); h->d_heavy2 = a.take<int32_t>((size_t)K + 1);      // (their counters are zeroed below)
        h->d_valid = a.take<uint8_t>((size_t)K);
        h->d_nodes = a.take<int32_t>(K); h->d_node_pts = a.take<double>((size_t)K * 3); h->d_node_nrm = a.take<double>((size_t)K * 3);
        h->d_ctrl_raw = a.take<double>((size_t)K * 3); h->d_ctrl_a = a.take<double>((size_t)K * 3); h->d_ctrl_b = a.take<double>((size_t)K * 3);
        h->d_d2min = a.take<float>(K); h->d_counts = a.take<int32_t>((size_t)K * 2);
        h->d_prev_d2 = a.take<float>(K); h->d_prev_node = a.take<double>((size_t)K * 3);
        h->d_near_prev = a.take<double>((size_t)K * 3); h->d_lim = a.take<float>(K);
        h->d_mid = a.take<int32_t>((size_t)K + 1); h->d_mid2 = a.take<int32_t>((size_t)K + 1);
        h->d_ng_sync = a.take<unsigned long long>(32);
        h->d_records = a.take<mvs_cand>((size_t)K * 8); h->d_top_idx = a.take<int64_t>((size_t)K * 8);
        h->d_nbr = a.take<int32_t>((size_t)K * 64);                            // graph_k <= 63
        h->d_knn_ws = ws_bytes ? (void*)a.take<char>(ws_bytes) : nullptr;
    };
    {
        Arena a; lay(a);
        HIPCHK(hipMalloc(&h->arena_nodes, a.off + 256));
        Arena b; b.base = (char*)h->arena_nodes; lay(b);
    }
    HIPCHK(hipMemsetAsync(h->d_heavy, 0, sizeof(int32_t), h->stream)); HIPCHK(hipMemsetAsync(h->d_heavy2, 0, sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->d_mid, 0, sizeof(int32_t), h->stream)); HIPCHK(hipMemsetAsync(h->d_mid2, 0, sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->d_ng_sync, 0, sizeof(unsigned long long) * 32, h->stream));
    h->ng_pass = 0;
    HIPCHK(hipMemsetAsync(h->d_valid, 0, (size_t)std::max<int64_t>(K, 1), h->stream));
    h->heavy_flip = 0;
    HIPCHK(hipMemsetAsync(h->d_is_ctrl, 0, sizeof(int32_t) * h->V, h->stream));
    if (K) HIPCHK(hipMemcpyAsync(h->d_nodes, h->h_nodes.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, h->stream));   // (from the handle's own copy: it outlives the call)
    launch_gather_nodes(h->d_pts, h->d_nrm, h->d_nodes, (int)K, h->d_node_pts, h->d_node_nrm, h->stream, h->d_is_ctrl);
    if (K) HIPCHK(hipMemcpyAsync(h->d_ctrl_raw, h->d_node_pts, sizeof(double) * K * 3, hipMemcpyDeviceToDevice, h->stream));
    h->d_ctrl_final = h->d_ctrl_raw;
    h->cg_iters = 0;                                  // new node set: every launch plan and the solver bracket start over
    for (int i = 0; i < 8; ++i) { h->cg_plan[i] = 0; h->ras_plan[i] = 0; h->bump_seq[i] = 0; h->ras_hist_n[i] = 0; }
    h->ras_mix_any = 0; h->ras_mix_calm = 0; h->assoc_passes = 0;
    HIPCHK(hipMemsetAsync(h->d_ctl, 0, sizeof(double) * 4, h->stream));     // verdicts of the old node set say nothing about the new one
    h->ras_a = 0.0; h->ras_m = 0;
    return MVS_OK;
}

int mvs_deform_set_nodes(mvs_deform_t h, const int32_t* vertex_idx, int64_t K) {
    MVS_TRACE();
    if (!h || K < 0 || (K > 0 && !vertex_idx)) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    HIPCHK(hipSetDevice(h->device));
    std::vector<char> seen(h->V, 0);
    for (int64_t k = 0; k < K; ++k) {
        const int v = vertex_idx[k];
        if (v < 0 || v >= h->V) { mvs_set_error("node %lld: vertex index out of range", (long long)k); return MVS_E_INVALID_ARG; }
        if (seen[v]) { mvs_set_error("node %lld: vertex %d listed twice", (long long)k, v); return MVS_E_INVALID_ARG; }
        seen[v] = 1;
    }
    return install_nodes(h, vertex_idx, K);
}

// Same topology, new positions (e.g. the template's rest pose again, for the next scan): everything that depends on the
// topology alone — adjacency tables, patch tables, node set, launch plans — is kept, which is what mvs_deform_create spends
// its 20 ms on.
int mvs_deform_set_vertices(mvs_deform_t h, const double* points, const double* normals) {
    MVS_TRACE();
    if (!h || !points) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyAsync(h->d_pts, points, sizeof(double) * 3 * (size_t)h->V, hipMemcpyHostToDevice, h->stream));
    if (normals) HIPCHK(hipMemcpyAsync(h->d_nrm, normals, sizeof(double) * 3 * (size_t)h->V, hipMemcpyHostToDevice, h->stream));
    if (h->K > 0) {
        launch_gather_nodes(h->d_pts, h->d_nrm, h->d_nodes, (int)h->K, h->d_node_pts, h->d_node_nrm, h->stream);
        HIPCHK(hipMemcpyAsync(h->d_ctrl_raw, h->d_node_pts, sizeof(double) * h->K * 3, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemsetAsync(h->d_valid, 0, (size_t)h->K, h->stream));
        h->d_ctrl_final = h->d_ctrl_raw;
    }
    h->graph_ready_nn = 0; h->weights_ready = false; h->heavy_pending = nullptr; h->graph_in_local = false;
    h->near_age = 0;                                   // a new fit: its first association searches unbounded
    HIPCHK(hipStreamSynchronize(h->stream));                 // (the host arrays may be released on return)
    return mvs_check_hip(hipGetLastError(), "set_vertices");
}

int mvs_deform_sample_nodes(mvs_deform_t h, int knn, int64_t* K) {
    MVS_TRACE();
    // UniformSampling, Deformation.cpp:63-106: exact kNN table on the GPU, greedy suppression
    // in vertex order on the host (inherently sequential).
    if (!h || knn < 1 || knn > 64) { mvs_set_error("knn must be 1..64"); return MVS_E_INVALID_ARG; }
    HIPCHK(hipSetDevice(h->device));
    const int64_t V = h->V;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (mvs_debug_level()) fprintf(stderr, "[mvs] sample_nodes: %s at %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    // one block of the scratch pool: the table, then the search grid's workspace; the host table is runtime.cpp's one-slot cache
    const size_t tab_bytes = (sizeof(int32_t) * (size_t)V * knn + 255) & ~(size_t)255;
    const size_t ws_bytes = V >= 1024 ? knn_grid_ws_bytes((int)V) : 0;
    int32_t* tab = nullptr;
    int rc;
    {
        Scratch d_mem;
        if ((rc = d_mem.alloc(tab_bytes + ws_bytes + 256, h->stream))) return rc;
        if ((rc = host_table_acquire(tab_bytes, (void**)&tab))) return rc;
        int32_t* d_tab = d_mem.as<int32_t>();
        lap("allocation");
        if (ws_bytes) launch_knn_grid(h->d_pts, (int)V, knn, d_tab, d_mem.as<char>() + tab_bytes, h->stream);
        else launch_knn(h->d_pts, (int)V, knn, d_tab, h->stream);
        rc = mvs_check_hip(hipMemcpyAsync(tab, d_tab, sizeof(int32_t) * V * knn, hipMemcpyDeviceToHost, h->stream), "download");
        if (!rc) rc = mvs_check_hip(hipStreamSynchronize(h->stream), "sync");
        lap("kNN table on the host");
    }
    if (rc) { host_table_release(tab, tab_bytes); return rc; }
    // greedy suppression in vertex order.  The rows of the table come straight from a DMA write (none of them in a CPU cache):
    // every row is requested a few vertices ahead — the loop's branch ("removed?") is predicted well enough for the core to run
    // ahead, a formulation without it (next zero bit of a bitmap) made every row fetch a serial DRAM round trip: 0.9 ms against 0.5
    std::vector<char> removed(V, 0);
    std::vector<int32_t> samp;
    samp.reserve((size_t)V / 4 + 16);
    for (int64_t i = 0; i < V; ++i) {
        if (i + 24 < V) __builtin_prefetch(tab + (size_t)(i + 24) * knn);
        if (removed[i]) continue;                           // :85
        samp.push_back((int32_t)i);
        const int32_t* row = tab + (size_t)i * knn;
        for (int j = 0; j < knn; ++j) {
            const int nb = row[j];
            if (nb >= 0 && nb != i) removed[nb] = 1;        // :98-102
        }
    }
    host_table_release(tab, tab_bytes);
    lap("greedy suppression");
    rc = install_nodes(h, samp.data(), (int64_t)samp.size());   // (distinct and in range by construction)
    if (rc) return rc;
    lap("nodes installed");
    if (K) *K = (int64_t)samp.size();
    return MVS_OK;
}

int mvs_deform_get_nodes(mvs_deform_t h, int32_t* vertex_idx) {
    if (!h || !vertex_idx) return MVS_E_INVALID_ARG;
    std::memcpy(vertex_idx, h->h_nodes.data(), h->h_nodes.size() * sizeof(int32_t));
    return MVS_OK;
}
int mvs_deform_sizes(mvs_deform_t h, int64_t* V, int64_t* F, int64_t* K, int64_t* P) {
    if (!h) return MVS_E_INVALID_ARG;
    if (V) *V = h->V; if (F) *F = h->F; if (K) *K = h->K; if (P) *P = h->P;
    return MVS_OK;
}

// ------------------------------------------------------------------- target ----
int mvs_deform_set_target_dev(mvs_deform_t h, int64_t P, const double* pts_dev, const double* normals_dev, int64_t index_base) {
    MVS_TRACE();
    if (!h || P < 0 || (P > 0 && (!pts_dev || !normals_dev))) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    HIPCHK(hipSetDevice(h->device));
    // the caller's buffers were produced on some other stream (torch's current stream, the legacy default stream ...);
    // the handle's stream is non-blocking and is not ordered after any of them.  This is a set-up call that synchronises
    // several times anyway: wait for the whole device once so that the index is never built from a half-written target.
    HIPCHK(hipDeviceSynchronize());
    return grid_build(h, P, pts_dev, normals_dev, index_base);
}
int mvs_deform_set_target(mvs_deform_t h, int64_t P, const double* pts, const double* normals, int64_t index_base) {
    MVS_TRACE();
    if (!h || P < 0 || (P > 0 && (!pts || !normals))) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    HIPCHK(hipSetDevice(h->device));
    double *dp = nullptr, *dn = nullptr;
    int rc = dmalloc(&dp, (size_t)P * 3);
    if (!rc) rc = dmalloc(&dn, (size_t)P * 3);
    if (!rc && P) rc = mvs_check_hip(hipMemcpyAsync(dp, pts, sizeof(double) * P * 3, hipMemcpyHostToDevice, h->stream), "upload");
    if (!rc && P) rc = mvs_check_hip(hipMemcpyAsync(dn, normals, sizeof(double) * P * 3, hipMemcpyHostToDevice, h->stream), "upload");
    if (!rc) rc = mvs_deform_set_target_dev(h, P, dp, dn, index_base);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(dp); (void)hipFree(dn);
    return rc;
}

// ------------------------------------------------------------------ iterate ----
static int ready(mvs_deform_t h, const mvs_deform_params* p, bool need_target) {
    if (!h) { mvs_set_error("handle is NULL"); return MVS_E_INVALID_ARG; }
    int rc = check_params(p);
    if (rc) return rc;
    if (need_target && !h->has_target) { mvs_set_error("no target set: call mvs_deform_set_target first"); return MVS_E_STATE; }
    if (h->K == 0) { mvs_set_error("no nodes: call mvs_deform_sample_nodes / _set_nodes first"); return MVS_E_STATE; }
    return mvs_check_hip(hipSetDevice(h->device), "hipSetDevice");
}

static constexpr int MAX_BATCH = 32;

int mvs_deform_iterate(mvs_deform_t h, const mvs_deform_params* p, int n_outer, mvs_deform_stats* stats) {
    MVS_TRACE();
    int rc = ready(h, p, true);
    if (rc) return rc;
    if (n_outer < 0) return MVS_E_INVALID_ARG;
    int done = 0;
    mvs_deform_stats st = h->last;
    if (!stats && h->cg_iters > 0) {
        // enqueue only (no host synchronisation): several handles on their own streams overlap this way; the launch plan
        // stays the one of the last harvest until mvs_deform_collect (or a call with stats) reads the statistics back.
        // Nobody follows the ring here: a solve that misses cg_tol raises the device-side escalation (strong local solves
        // for the rest of what is enqueued) and is reported by the collecting call.
        const CgPlan cg = probe_cg(h, *p);
        for (int o = 0; o < n_outer; ++o) {
            enqueue_assoc_local(h, *p);
            rc = enqueue_solve(h, *p, h->d_ctrl_raw, true, cg, true);
            if (rc) return rc;
        }
        return MVS_OK;
    }
    int status = MVS_OK;
    double worst = 0.0;
    int solves = 0, missed = 0, esc = 0;
    while (done < n_outer) {
        // enqueue as many outer iterations as the current calibration allows, then harvest once
        const bool calibrated = h->cg_iters > 0;
        // (at most MAX_BATCH passes between two harvests; inside a batch the host follows the residual ring — throttle,
        //  peek_ring — and lengthens the plan of a solve as soon as its margin gets thin)
        const int batch = calibrated ? std::min(n_outer - done, MAX_BATCH) : 1;
        CgPlan cg = probe_cg(h, *p);
        for (int o = 0; o < batch; ++o) {
            if (calibrated && o > 0) {
                if ((rc = throttle(h))) return rc;
                peek_ring(h, *p, use_ras(h, *p));
                cg = probe_cg(h, *p);
            }
            enqueue_assoc_local(h, *p);
            rc = enqueue_solve(h, *p, h->d_ctrl_raw, true, cg);
            if (rc) return rc;
        }
        bool conv = true;
        rc = harvest(h, *p, cg, &st, &conv);
        if (rc < 0) return rc;
        if (rc > 0) status = rc;
        worst = std::max(worst, st.worst_rel_residual_in_batch);
        solves += st.solves_in_batch; missed += st.unconverged_solves; esc |= st.escalated;
        done += batch;
    }
    st.outer_done = done;
    st.worst_rel_residual_in_batch = worst; st.solves_in_batch = solves; st.unconverged_solves = missed; st.escalated = esc;
    h->last = st;
    if (stats) *stats = st;
    return status;
}

int mvs_deform_assoc_dmin(mvs_deform_t h, const mvs_deform_params* p, float* d2min_dev) {
    MVS_TRACE();
    int rc = ready(h, p, true);
    if (rc) return rc;
    if (!d2min_dev) return MVS_E_INVALID_ARG;
    h->near_age = 0;              // (the sharded step keeps its own bound, d_prev_d2 / d_prev_node)
    Tic t = tic(h, "assoc");
    launch_assoc_dmin(h->grid, h->d_node_pts, (int)h->K, d2min_dev, h->stream, h->prev_valid ? h->d_prev_d2 : nullptr, h->d_prev_node);
    toc(t, 1);
    return mvs_check_hip(hipGetLastError(), "assoc_dmin");
}
int mvs_deform_assoc_select(mvs_deform_t h, const mvs_deform_params* p, const float* d2min_dev, mvs_cand* records_dev,
                            int32_t* counts_dev) {
    MVS_TRACE();
    int rc = ready(h, p, true);
    if (rc) return rc;
    if (!d2min_dev || !records_dev || !counts_dev) return MVS_E_INVALID_ARG;
    h->near_age = 0;
    Tic t = tic(h, "assoc");
    // The heavy-node pass shares its launch with two pieces of the solve that need nothing from the exchange: the node
    // graph and (patch solver) the cotangent weights — they then overlap with the heavy nodes instead of following the
    // collectives (mvs_deform_solve finds them done).
    const int K = (int)h->K, nn = p->graph_k + 1;
    const bool fuse = h->d_knn_ws != nullptr && nn <= 64 && ensure_nbr(h, nn) == MVS_OK;
    // (the heavy pass writes d2min only for entries whose coarse walk was deferred: the single-rank k_assoc_local makes those, never this path)
    launch_assoc_select(h->grid, h->d_node_pts, h->d_node_nrm, K, p->top_k, const_cast<float*>(d2min_dev), records_dev, counts_dev, h->d_heavy, K, h->stream, fuse,
                        h->d_prev_d2, h->d_prev_node);
    h->prev_valid = h->d_prev_d2 != nullptr;
    if (fuse) {
        const bool w = use_ras(h, *p);
        knn_grid_build(h->d_node_pts, K, h->d_knn_ws, h->stream);
        launch_assoc_heavy_knn(h->grid, h->d_node_pts, h->d_node_nrm, K, *p, const_cast<float*>(d2min_dev), records_dev, counts_dev, h->d_heavy, K,
                               nullptr, nullptr, nullptr, nn, h->d_nbr, h->d_knn_ws, h->stream, w ? &h->sell : nullptr, h->d_pts,
                               arap_grid_blocks(h->sell));
        h->graph_ready_nn = nn; h->weights_ready = w;
    }
    toc(t, fuse ? 3 : 2);
    return mvs_check_hip(hipGetLastError(), "assoc_select");
}
int mvs_deform_assoc_merge(mvs_deform_t h, const mvs_deform_params* p, const mvs_cand* records_all_dev,
                           const int32_t* counts_all_dev, int nranks) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (!records_all_dev || !counts_all_dev || nranks < 1) return MVS_E_INVALID_ARG;
    Tic t = tic(h, "assoc");
    launch_assoc_merge(h->d_node_pts, h->d_node_nrm, (int)h->K, *p, records_all_dev, counts_all_dev, nranks, h->d_ctrl_raw,
                       h->d_valid, h->d_top_idx, h->stream);
    toc(t, 1);
    return mvs_check_hip(hipGetLastError(), "assoc_merge");
}
int mvs_deform_assoc_merge_packed(mvs_deform_t h, const mvs_deform_params* p, const void* packed_all_dev, int nranks) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (!packed_all_dev || nranks < 1) return MVS_E_INVALID_ARG;
    const int64_t K = h->K, rec_bytes = K * 8 * (int64_t)sizeof(mvs_cand), stride = rec_bytes + K * 2 * (int64_t)sizeof(int32_t);
    Tic t = tic(h, "assoc");
    launch_assoc_merge(h->d_node_pts, h->d_node_nrm, (int)K, *p, (const mvs_cand*)packed_all_dev,
                       (const int32_t*)((const char*)packed_all_dev + rec_bytes), nranks, h->d_ctrl_raw, h->d_valid, h->d_top_idx, h->stream,
                       stride, stride);
    toc(t, 1);
    return mvs_check_hip(hipGetLastError(), "assoc_merge");
}
// owner-merges exchange (N >= 4 ranks): a rank merges only the node block [k0, k1) it owns, into ONE block buffer
// [block_nodes * 3 doubles | block_nodes bytes] (block_nodes >= k1 - k0: the padded size every rank all-gathers) ...
int mvs_deform_assoc_merge_block(mvs_deform_t h, const mvs_deform_params* p, const mvs_cand* records_blk_dev, const int32_t* counts_blk_dev,
                                 int nranks, int64_t k0, int64_t k1, int64_t block_nodes, void* block_dev) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (!records_blk_dev || !counts_blk_dev || !block_dev || nranks < 1 || k0 < 0 || k1 < k0 || k1 > h->K || block_nodes < k1 - k0) {
        mvs_set_error("bad arguments (0 <= k0 <= k1 <= K, block_nodes >= k1 - k0)"); return MVS_E_INVALID_ARG;
    }
    Tic t = tic(h, "assoc");
    launch_assoc_merge(h->d_node_pts, h->d_node_nrm, (int)(k1 - k0), *p, records_blk_dev, counts_blk_dev, nranks, (double*)block_dev,
                       (uint8_t*)block_dev + sizeof(double) * 3 * (size_t)block_nodes, nullptr, h->stream, 0, 0, (int)k0);
    toc(t, 1);
    return mvs_check_hip(hipGetLastError(), "assoc_merge_block");
}
// ... and every rank installs the all-gathered blocks (what mvs_deform_assoc_merge would have left) before _solve: node k
// is entry k % block_nodes of block k / block_nodes
int mvs_deform_set_node_targets_dev(mvs_deform_t h, const void* blocks_dev, int nblocks, int64_t block_nodes, int64_t block_stride_bytes) {
    MVS_TRACE();
    if (!h || !blocks_dev || nblocks < 1 || block_nodes < 1) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    if (h->K == 0) { mvs_set_error("no nodes"); return MVS_E_STATE; }
    if ((int64_t)nblocks * block_nodes < h->K || block_stride_bytes < block_nodes * 25) {
        mvs_set_error("the blocks do not cover the %lld nodes", (long long)h->K); return MVS_E_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(h->device));
    launch_install_targets(blocks_dev, (int)h->K, (int)block_nodes, block_stride_bytes, h->d_ctrl_raw, h->d_valid, h->d_top_idx, h->stream);
    return mvs_check_hip(hipGetLastError(), "set_node_targets");
}
int mvs_deform_solve(mvs_deform_t h, const mvs_deform_params* p, mvs_deform_stats* stats) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (h->cg_iters > 0) {              // calibrated: stay at most THROTTLE_LAG passes ahead of the device and follow the residual ring
        if ((rc = throttle(h))) return rc;
        peek_ring(h, *p, use_ras(h, *p));
    }
    const CgPlan cg = probe_cg(h, *p);
    rc = enqueue_solve(h, *p, h->d_ctrl_raw, true, cg);
    if (rc) return rc;
    // stats == NULL on a calibrated handle: enqueue only (no host sync); the next call with stats harvests
    if (!stats && h->cg_iters > 0) return MVS_OK;
    return harvest(h, *p, cg, stats, nullptr);
}
int mvs_deform_collect(mvs_deform_t h, const mvs_deform_params* p, mvs_deform_stats* stats) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (h->cg_iters <= 0) { mvs_set_error("nothing enqueued: the first mvs_deform_iterate / _solve of a handle runs synchronously"); return MVS_E_STATE; }
    return harvest(h, *p, probe_cg(h, *p), stats, nullptr);
}
int mvs_deform_arap(mvs_deform_t h, const mvs_deform_params* p, const double* ctrl_targets, mvs_deform_stats* stats) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (!ctrl_targets) return MVS_E_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(h->d_ctrl_a, ctrl_targets, sizeof(double) * h->K * 3, hipMemcpyHostToDevice, h->stream));
    const CgPlan cg = probe_cg(h, *p);
    rc = enqueue_solve(h, *p, h->d_ctrl_a, false, cg);
    if (rc) return rc;
    return harvest(h, *p, cg, stats, nullptr);
}
int mvs_deform_solver_info(mvs_deform_t h, const mvs_deform_params* p, int32_t* kind, int64_t* patches, int64_t* local_rows, int32_t* width) {
    if (!h) { mvs_set_error("handle is NULL"); return MVS_E_INVALID_ARG; }
    const bool ras = h->has_ras && (!p || p->solver != MVS_SOLVER_CG);
    if (kind) *kind = ras ? 1 : 0;
    if (patches) *patches = ras ? h->ras.NP : 0;
    if (local_rows) *local_rows = ras ? h->ras_rows : 0;
    if (width) *width = ras ? h->ras.W : 0;
    return MVS_OK;
}
int mvs_deform_sync(mvs_deform_t h) {
    MVS_TRACE();
    if (!h) return MVS_E_INVALID_ARG;
    return mvs_check_hip(hipStreamSynchronize(h->stream), "sync");
}
void* mvs_deform_stream(mvs_deform_t h) { return h ? (void*)h->stream : nullptr; }
int mvs_deform_set_stream(mvs_deform_t h, void* hip_stream) {
    MVS_TRACE();
    if (!h) return MVS_E_INVALID_ARG;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return MVS_OK;
}

// ---------------------------------------------------------------- read-back ----
static int download(mvs_deform_t h, void* dst, const void* src, size_t n) {
    if (!h || !dst) return MVS_E_INVALID_ARG;
    HIPCHK(hipSetDevice(h->device));
    if (n) HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, h->stream));
    return mvs_check_hip(hipStreamSynchronize(h->stream), "sync");
}
int mvs_deform_get_vertices(mvs_deform_t h, double* pts) { return download(h, pts, h ? h->d_pts : nullptr, h ? sizeof(double) * h->V * 3 : 0); }
int mvs_deform_get_normals(mvs_deform_t h, double* n) { return download(h, n, h ? h->d_nrm : nullptr, h ? sizeof(double) * h->V * 3 : 0); }
int mvs_deform_get_rotations(mvs_deform_t h, double* R) { return download(h, R, h ? h->d_rot : nullptr, h ? sizeof(double) * h->V * 9 : 0); }
int mvs_deform_get_node_targets(mvs_deform_t h, int smoothed, double* controls, uint8_t* valid, float* d2min, int32_t* counts,
                                int64_t* top_idx) {
    MVS_TRACE();
    if (!h || !controls) return MVS_E_INVALID_ARG;
    const size_t K = (size_t)h->K;
    int rc = download(h, controls, smoothed ? h->d_ctrl_final : h->d_ctrl_raw, sizeof(double) * K * 3);
    if (!rc && valid) rc = download(h, valid, h->d_valid, K);
    if (!rc && d2min) rc = download(h, d2min, h->d_d2min, sizeof(float) * K);
    if (!rc && counts) rc = download(h, counts, h->d_counts, sizeof(int32_t) * K * 2);
    if (!rc && top_idx) rc = download(h, top_idx, h->d_top_idx, sizeof(int64_t) * K * 8);
    return rc;
}
int mvs_deform_get_node_graph(mvs_deform_t h, int32_t* nbr) {
    MVS_TRACE();
    if (!h || !nbr) return MVS_E_INVALID_ARG;
    if (!h->d_nbr || h->nbr_k == 0) { mvs_set_error("node graph not built yet"); return MVS_E_STATE; }
    return download(h, nbr, h->d_nbr, sizeof(int32_t) * (size_t)h->K * h->nbr_k);
}
int mvs_deform_compute_normals(mvs_deform_t h, double* normals) {
    MVS_TRACE();
    if (!h || !normals) return MVS_E_INVALID_ARG;
    HIPCHK(hipSetDevice(h->device));
    double* d = nullptr;
    int rc = dmalloc(&d, (size_t)h->V * 3);
    if (rc) return rc;
    launch_vertex_normals(h->d_pts, h->d_faces, h->d_vf_ptr, h->d_vf, (int)h->V, d, h->stream);
    rc = download(h, normals, d, sizeof(double) * h->V * 3);
    (void)hipFree(d);
    return rc;
}

int mvs_knn_points(const double* pts, int64_t n, int k, int32_t* out_idx) {
    MVS_TRACE();
    if (!pts || !out_idx || n <= 0 || k < 1 || k > 64 || n > 0x7ffffff0LL) { mvs_set_error("bad arguments (k 1..64)"); return MVS_E_INVALID_ARG; }
    int rc = need_device();
    if (rc) return rc;
    mvs_preload(mvs_current_device());
    double* d = nullptr; int32_t* o = nullptr;
    rc = dmalloc(&d, (size_t)n * 3);
    if (!rc) rc = dmalloc(&o, (size_t)n * k);
    if (!rc) rc = mvs_check_hip(hipMemcpy(d, pts, sizeof(double) * n * 3, hipMemcpyHostToDevice), "upload");
    void* ws = nullptr;
    if (!rc && n >= 1024) rc = mvs_check_hip(hipMalloc(&ws, knn_grid_ws_bytes((int)n)), "hipMalloc");
    if (!rc) {
        if (ws) launch_knn_grid(d, (int)n, k, o, ws, nullptr); else launch_knn(d, (int)n, k, o, nullptr);
        rc = mvs_check_hip(hipDeviceSynchronize(), "knn");
    }
    if (ws) (void)hipFree(ws);
    if (!rc) rc = mvs_check_hip(hipMemcpy(out_idx, o, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost), "download");
    (void)hipFree(d); (void)hipFree(o);
    return rc;
}

// ---- test hooks (include/mvs_test.h; not part of the ABI of include/mvs.h): all state they set lives in the handle ----
// the heavy list of the last association — entries, and how many of them had their coarse nearest-distance walk deferred
int mvs_test_heavy_count(mvs_deform_t h, int* n, int* flagged) {
    if (!h || !h->d_heavy) return MVS_E_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    const int32_t* cur = h->heavy_flip ? h->d_heavy : h->d_heavy2;      // (the list the LAST association filled)
    std::vector<int32_t> l((size_t)h->K + 1);
    HIPCHK(hipMemcpy(l.data(), cur, sizeof(int32_t) * l.size(), hipMemcpyDeviceToHost));
    int f = 0;
    for (int i = 0; i < l[0] && i < (int)h->K; ++i) f += (l[1 + i] & 0x40000000) != 0;
    if (n) *n = l[0];
    if (flagged) *flagged = f;
    return MVS_OK;
}

// the handle's solver control block (engine.h, MVS_CTL_*: verdict ring, sweeps used, prediction safety factor ...) -> out[n], n <= MVS_CTL_SIZE
int mvs_test_ctl(mvs_deform_t h, double* out, int n) {
    if (!h || !out || n < 1 || n > MVS_CTL_SIZE) return MVS_E_INVALID_ARG;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->d_ctl, sizeof(double) * n, hipMemcpyDeviceToHost));
    return MVS_OK;
}

// waits until the cold-start helper thread of the current device has loaded the code objects and primed the stream pool
int mvs_test_preload_wait(void) { mvs_preload_join(mvs_current_device()); return MVS_OK; }

// maxspin = polls a workgroup waits at the tail loop's device-wide barrier before it abandons the solve (<= 0: default);
// plan_cap = at most this many launches per solve, the remaining sweeps run inside the last one (0: no cap); skip_wg = the
// workgroup of every tail launch that never arrives at the barrier, so that the wait of every other one expires (-1: none).
// State of THIS handle only.
int mvs_test_tail(mvs_deform_t h, int maxspin, int plan_cap, int skip_wg) {
    if (!h) return MVS_E_INVALID_ARG;
    h->dbg_maxspin = maxspin > 0 ? maxspin : 0;
    h->dbg_plan_cap = plan_cap > 0 ? plan_cap : 0;
    h->dbg_skip_wg = skip_wg >= 0 ? skip_wg : -1;
    return MVS_OK;
}

// Geometry of the handle's target grid: out[0..2] = origin, [3] = cell edge, [4..6] = fine cells per axis, [7] = target points.
int mvs_test_grid(mvs_deform_t h, double* out) {
    if (!h || !out) return MVS_E_INVALID_ARG;
    out[0] = h->grid.minx; out[1] = h->grid.miny; out[2] = h->grid.minz; out[3] = h->grid.h;
    out[4] = h->grid.nx; out[5] = h->grid.ny; out[6] = h->grid.nz; out[7] = (double)h->grid.P;
    return MVS_OK;
}

// The handle stops qualifying for group launches once it has been harvested `after_batches` times inside group calls (0: never):
// forces the mid-call hand-over of mvs_deform_group_iterate to handle-by-handle stepping.
int mvs_test_group_leave(mvs_deform_t h, int after_batches) {
    if (!h) return MVS_E_INVALID_ARG;
    h->dbg_group_leave = after_batches > 0 ? after_batches : 0;
    return MVS_OK;
}

// Chebyshev steps every patch ran in the launch of sweep slot `slot` of the handle's last pass (slots are numbered through the
// pass: solve 0's launches first) -> out[NP].  A tail launch that swept k times in the kernel reports k * steps-per-sweep.
int mvs_test_sweep_steps(mvs_deform_t h, int slot, int32_t* out) {
    if (!h || !out || !h->has_ras || slot < 0 || (int64_t)slot >= h->ras_slots_cap) return MVS_E_INVALID_ARG;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->d_ras_iters + (size_t)slot * h->ras.NP, sizeof(int32_t) * h->ras.NP, hipMemcpyDeviceToHost));
    return MVS_OK;
}

// (tests/test_gpu_meshbuild.py) the tables the device build left, copied to the host.
// what = 0: dims as int64[8] {NP, LS, W, nslices, ne, single_pass, has_patches, total local rows}; 1 slice_off, 2 col, 3 opp0,
// 4 opp1, 5 vf_ptr, 6 vf, 7 pnloc, 8 pown, 9 pnh, 10 l2g, 11 hl2g, 12 lcol (int16), 13 gent, 14 gcol.  out == NULL: only *bytes.
int mvs_test_mesh_table(mvs_deform_t h, int what, void* out, int64_t* bytes) {
    if (!h || !bytes) return MVS_E_INVALID_ARG;
    HIPCHK(hipSetDevice(h->device));
    const RasDev& R = h->ras;
    const int64_t rows = h->has_ras ? (int64_t)R.NP * R.LS : 0, ent = rows * R.W, ne = h->n_entries, ns = h->sell.nslices;
#ifdef MVS_EXPERIMENTS
    if (what >= 112 && what <= 114) {      // experiments (scripts/slot_assign_ab.py): overwrite an entry table of the patches
        if (!h->has_ras || !out) return MVS_E_STATE;
        HIPCHK(hipStreamSynchronize(h->stream));
        void* dst = what == 112 ? (void*)R.lcol : what == 113 ? (void*)R.gent : (void*)R.gcol;
        HIPCHK(hipMemcpy(dst, out, (size_t)((what == 112 ? 2 : 4) * ent), hipMemcpyHostToDevice));
        return MVS_OK;
    }
#endif
    const void* src = nullptr;
    int64_t n = 0;
    int64_t dims[8] = {h->has_ras ? R.NP : 0, h->has_ras ? R.LS : 0, h->has_ras ? R.W : 0, ns, ne, h->sell.single_pass, h->has_ras ? 1 : 0, h->ras_rows};
    switch (what) {
        case 0: n = sizeof dims; break;
        case 1: src = h->d_slice_off; n = 4 * (ns + 1); break;
        case 2: src = h->d_col; n = 4 * ne; break;
        case 3: src = h->d_opp0; n = 4 * ne; break;
        case 4: src = h->d_opp1; n = 4 * ne; break;
        case 5: src = h->d_vf_ptr; n = 4 * (h->V + 1); break;
        case 6: src = h->d_vf; n = 4 * 3 * h->F; break;
        case 7: src = R.pnloc; n = 4 * (int64_t)R.NP; break;
        case 8: src = R.pown; n = 4 * (int64_t)R.NP; break;
        case 9: src = R.pnh; n = 4 * (int64_t)R.NP; break;
        case 10: src = R.l2g; n = 4 * rows; break;
        case 11: src = R.hl2g; n = 4 * rows; break;
        case 12: src = R.lcol; n = 2 * ent; break;
        case 13: src = R.gent; n = 4 * ent; break;
        case 14: src = R.gcol; n = 4 * ent; break;
        default: return MVS_E_INVALID_ARG;
    }
    *bytes = n;
    if (!out) return MVS_OK;
    if (what == 0) { std::memcpy(out, dims, sizeof dims); return MVS_OK; }
    if (what >= 7 && !h->has_ras) return MVS_E_STATE;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n) HIPCHK(hipMemcpy(out, src, (size_t)n, hipMemcpyDeviceToHost));
    return MVS_OK;
}

int mvs_deform_enable_timing(mvs_deform_t h, int on) {
    if (!h) return MVS_E_INVALID_ARG;
    h->timing = on;
    h->timers.clear();
    h->samples.clear(); h->sample_off.clear(); h->sample_pass_first.clear(); h->sample_used = 0;
    return MVS_OK;
}
int mvs_deform_kernel_time(mvs_deform_t h, const char* name, double* total_ms, int64_t* launches) {
    if (!h || !name) return MVS_E_INVALID_ARG;
    auto it = h->timers.find(name);
    if (total_ms) *total_ms = it == h->timers.end() ? 0.0 : it->second.total_ms;
    if (launches) *launches = it == h->timers.end() ? 0 : it->second.launches;
    return MVS_OK;
}


// ---------------------------------------------------------------------------------------------------- groups ----
// Several handles on one device stepping in lockstep — BASELINE config 5's sixteen per-part graphs (partwise.py) — as ONE
// sequence of launches: every kernel of a bounded pass is launched once with grid (x, part) and takes its part's record
// (engine.h, PartDev).  Sixteen parts cost sixteen launch chains before (~640 launches per outer iteration at the runtime's
// ~3.3 us per launch: 2.0 ms, whatever the streams and host threads); a group's pass is ~40 launches.  Each part keeps its
// own control block, verdict ring, energy stop rule and plan history; the arithmetic of a part is what its handle computes
// alone (the launch plan is the longest of the parts': a part that needs fewer sweeps finds its solve finished and its
// launches return after one load, as spare launches always do).  Every solve of a group ends with a local-step launch of its
// own (k_arap_local_multi): the fused deciding launch of a single handle needs a barrier among ONE part's workgroups.
struct mvs_group_s {
    std::vector<mvs_deform_s*> h;
    std::vector<PartDev> host;
    PartDev* d_parts = nullptr;
    GroupDims dims{};
    int device = 0;
    int flip = 0;                       // which of every handle's two heavy / mid lists the next pass fills
    unsigned long long ng_pass = 0;
};

static int group_member_ok(const mvs_deform_s* h, const mvs_deform_params& p, int nn, std::string* why) {
    auto bad = [&](const char* m) { *why = m; return 0; };
    if (!h->has_ras || p.solver == MVS_SOLVER_CG) return bad("a part's mesh runs the CG solver");
    if (h->ras_mix_any) return bad("a part's solves stall (mixing sweeps)");
    if (h->near_age < 2 || h->cg_iters <= 0) return bad("a part has not stepped twice on its own yet (unbounded first passes, calibration)");
    if (!h->d_knn_ws || h->graph_prev_nn != nn || h->K < nn || !assoc_all_builds_grid((int)h->K)) return bad("a part's node graph cannot be searched bounded");
    if (h->grid.P <= 0) return bad("a part has no target points");
    if (h->timing) return bad("a part has timing enabled");
    if (h->saw_abandon) return bad("a part has seen an abandoned solve");
    if (h->dbg_group_leave > 0 && h->group_batches >= h->dbg_group_leave) return bad("a part was told to leave the group (mvs_test_group_leave)");
    return 1;
}

int mvs_deform_group_create(mvs_deform_t* handles, int n, mvs_group_t* out) {
    MVS_TRACE();
    if (!handles || n < 1 || n > 1024 || !out) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    *out = nullptr;
    for (int i = 0; i < n; ++i) {
        if (!handles[i] || handles[i]->device != handles[0]->device) { mvs_set_error("the handles of a group live on one device"); return MVS_E_INVALID_ARG; }
        for (int j = 0; j < i; ++j) if (handles[j] == handles[i]) { mvs_set_error("a handle is listed twice"); return MVS_E_INVALID_ARG; }
    }
    HIPCHK(hipSetDevice(handles[0]->device));
    mvs_group_s* g = new mvs_group_s;
    g->h.assign(handles, handles + n);
    g->host.resize(n);
    g->device = handles[0]->device;
    if (hipMalloc((void**)&g->d_parts, sizeof(PartDev) * n) != hipSuccess) { delete g; mvs_set_error("out of device memory"); return MVS_E_OOM; }
    *out = g;
    return MVS_OK;
}

int mvs_deform_group_destroy(mvs_group_t g) {
    MVS_TRACE();
    if (!g) return MVS_OK;
    (void)hipSetDevice(g->device);
    if (!g->h.empty() && g->h[0]->stream) (void)hipStreamSynchronize(g->h[0]->stream);
    if (g->d_parts) (void)hipFree(g->d_parts);
    delete g;
    return MVS_OK;
}

// n_outer outer iterations of every part; stats[n] (may be NULL).  MVS_E_STATE (nothing done) when the parts cannot step as a
// group yet — mvs_last_error says why; the caller then steps the handles one by one (mvs_deform_iterate).
int mvs_deform_group_iterate(mvs_group_t g, const mvs_deform_params* pp, int n_outer, mvs_deform_stats* stats) {
    MVS_TRACE();
    if (!g || n_outer < 0) { mvs_set_error("bad arguments"); return MVS_E_INVALID_ARG; }
    int rc = check_params(pp);
    if (rc) return rc;
    const mvs_deform_params& p = *pp;
    const int n = (int)g->h.size(), nn = p.graph_k + 1;
    if (p.smooth_sweeps != 2 || p.update_normals || nn > 16) { mvs_set_error("a group steps with smooth_sweeps = 2, update_normals = 0, graph_k <= 15"); return MVS_E_STATE; }
    HIPCHK(hipSetDevice(g->device));
    std::string why;
    for (mvs_deform_s* h : g->h) if (!group_member_ok(h, p, nn, &why)) { mvs_set_error("the handles cannot step as a group yet: %s", why.c_str()); return MVS_E_STATE; }
    for (mvs_deform_s* h : g->h) if (h->ras.W != g->h[0]->ras.W) { mvs_set_error("the parts' patch tables differ in width"); return MVS_E_STATE; }
    if (n_outer == 0) return MVS_OK;                          // (a probe: can the handles step as a group?)
    for (mvs_deform_s* h : g->h) HIPCHK(hipStreamSynchronize(h->stream));
    hipStream_t s = g->h[0]->stream;
    int status = MVS_OK;
    std::vector<mvs_deform_stats> acc(n);
    std::vector<double> worst(n, 0.0);
    std::vector<int> solves(n, 0), missed(n, 0), esc(n, 0);
    int done = 0;
    for (; done < n_outer;) {
        if (done > 0) {
            // the last harvest may have changed a part's regime (its solves stall: mixing sweeps; an abandoned solve): the group's
            // launches do not serve those — the rest of this call is then stepped handle by handle, below
            bool ok = true;
            for (mvs_deform_s* h : g->h) { update_mix_state(h, p.arap_iters); if (!group_member_ok(h, p, nn, &why)) ok = false; }
            if (!ok) break;
        }
        const int batch = std::min(n_outer - done, MAX_BATCH);
        // ---- the parts' records (the coefficient sets and the plans move at every harvest) and the launch dimensions
        GroupDims d{};
        d.n = n; d.W = g->h[0]->ras.W;
        RasPlan plan{};
        for (int i = 0; i < 8; ++i) plan.n[i] = 0;
        size_t lds = 0;
        for (int k = 0; k < n; ++k) {
            mvs_deform_s* h = g->h[k];
            // (the lists a pass fills alternate: bring every handle's pair into the group's phase)
            int32_t* hv[2] = {h->heavy_flip ? h->d_heavy2 : h->d_heavy, h->heavy_flip ? h->d_heavy : h->d_heavy2};
            int32_t* md[2] = {h->heavy_flip ? h->d_mid2 : h->d_mid, h->heavy_flip ? h->d_mid : h->d_mid2};
            PartDev& P = g->host[k];
            P.sell = h->sell; P.ras = h->ras; P.grid = h->grid;
            P.K = (int)h->K; P.V = (int)h->V; P.ras_block = h->ras_block; P.NC = knn_grid_cells_per_axis((int)h->K); P.ss = ras_slot_size(h); P.pad0 = 0;
            ras_cheb_sets(h, &P.cc, &P.cheb_m, &P.cc2, &P.m2);
            P.pts = h->d_pts; P.nrm = h->d_nrm; P.sol = h->d_sol; P.x2 = h->d_ras_x2; P.rot = h->d_rot; P.b = h->d_ras_b; P.bpure = h->d_bpure;
            P.pw = h->d_ras_pw; P.pd = h->d_ras_pd; P.slots = h->d_ras_slots; P.energy = h->d_energy; P.ctl = h->d_ctl; P.host_ctl = const_cast<double*>(h->h_ctl);
            P.iters = h->d_ras_iters; P.info = h->d_info; P.bar = h->d_bar;
            P.node_pts = h->d_node_pts; P.node_nrm = h->d_node_nrm; P.ctrl_raw = h->d_ctrl_raw; P.ctrl_a = h->d_ctrl_a; P.ctrl_b = h->d_ctrl_b; P.near_prev = h->d_near_prev;
            P.d2min = h->d_d2min; P.lim = h->d_lim; P.counts = h->d_counts; P.nbr = h->d_nbr;
            P.heavy[g->flip] = hv[0]; P.heavy[g->flip ^ 1] = hv[1]; P.mid[g->flip] = md[0]; P.mid[g->flip ^ 1] = md[1];
            P.rec = h->d_records; P.top_idx = h->d_top_idx; P.valid = h->d_valid;
            const void *geo, *sorted; const int* cs;
            knn_grid_views(h->d_knn_ws, (int)h->K, &geo, &cs, &sorted);
            P.ng_geo = const_cast<void*>(geo); P.ng_start = const_cast<int*>(cs); P.ng_sorted = const_cast<void*>(sorted); P.ng_sync = h->d_ng_sync;
            g->ng_pass = std::max(g->ng_pass, h->ng_pass);
            if ((rc = ensure_nbr(h, nn))) return rc;
            const RasPlan rp = probe_ras(h);
            if ((rc = ensure_ras_slots(h, p.arap_iters, rp))) return rc;
            for (int i = 0; i < p.arap_iters; ++i) plan.n[i] = std::max(plan.n[i], rp.n[i]);
            d.block = std::max(d.block, h->ras_block); d.Kmax = std::max(d.Kmax, (int)h->K); d.Vmax = std::max(d.Vmax, (int)h->V);
            // (row kernels: with four lanes per row — degree <= 8 — a 16-wave workgroup takes 256 rows; the handle's own grid holds twice
            //  the workgroups that then have rows, which costs nothing alone and whole rounds of the chip with sixteen parts in one launch)
            const int row_wgs = h->sell.single_pass ? ((((h->sell.nslices + 1) >> 1) + 15) / 16 + 1) : arap_grid_blocks(h->sell);
            d.NPmax = std::max(d.NPmax, h->ras.NP); d.Grow = std::max(d.Grow, std::min(row_wgs, arap_grid_blocks(h->sell)));
            int HB, MB, NB, GB, CB;
            assoc_all_dims((int)h->K, arap_grid_blocks(h->sell), true, &HB, &MB, &NB, &GB, &CB);
            HB = std::min(HB, 64); MB = std::min(MB, 4);          // (a part's lists hold a few dozen nodes; the workgroups loop over them)
            d.HB = std::max(d.HB, HB); d.MB = std::max(d.MB, MB); d.NB = std::max(d.NB, NB); d.GB = std::max(d.GB, GB); d.CB = std::max(d.CB, CB);
            lds = std::max(lds, assoc_all_lds_bytes((int)h->K, true));
        }
        d.lds_all = lds;
        g->dims = d;
        HIPCHK(hipMemcpyAsync(g->d_parts, g->host.data(), sizeof(PartDev) * n, hipMemcpyHostToDevice, s));
        // ---- the passes
        int last_slot = -1;
        for (int o = 0; o < batch; ++o) {
            const int par = g->flip;
            g->flip ^= 1;
            launch_group_assoc(g->d_parts, d, par, p, nn, ++g->ng_pass, s);
            launch_group_smooth(g->d_parts, d, nn, s);                                            // Deformation.cpp:362-381, first sweep
            launch_group_prepare(g->d_parts, d, nn, s);                                           // ... second sweep, patch matrices, start of the solve
            int parity = 0, slot = 0, prev_slot = -1;
            for (int it = 0; it < p.arap_iters; ++it) {
                launch_group_rhs(g->d_parts, d, parity, it, p.arap_tol, p.cg_tol, prev_slot, s);
                double predict = 1e300;
                for (mvs_deform_s* h : g->h) predict = std::min(predict, ras_predict_margin(h, it));
                for (int i = 0; i < plan.n[it]; ++i) { launch_group_sweep(g->d_parts, d, parity, it, p.arap_tol, i, p.cg_tol, STOP_AT, predict, slot, s); parity ^= 1; ++slot; }
                prev_slot = slot - 1;
                launch_group_local(g->d_parts, d, parity, it, p.arap_tol, s);
            }
            launch_group_finalize(g->d_parts, d, parity, p.arap_iters, p.arap_tol, p.cg_tol, prev_slot, s);
            last_slot = prev_slot;
            for (mvs_deform_s* h : g->h) {
                h->seq_enqueued++; h->assoc_passes++; h->near_age++;
                h->heavy_flip ^= 1;
                h->ng_pass = g->ng_pass;
                h->graph_prev_nn = nn; h->graph_ready_nn = 0; h->weights_ready = false; h->heavy_pending = nullptr; h->graph_in_local = false;
                h->d_ctrl_final = h->d_ctrl_b;
            }
        }
        (void)last_slot;
        HIPCHK(hipStreamSynchronize(s));
        rc = mvs_check_hip(hipGetLastError(), "group pass");
        if (rc) return rc;
        // ---- every part's verdicts and statistics, its plans re-made from what ITS solves ran
        for (int k = 0; k < n; ++k) {
            mvs_deform_stats st{};
            bool conv = true;
            rc = harvest_ras(g->h[k], p, &st, &conv, &plan);
            if (rc < 0) return rc;
            if (rc > 0) status = rc;
            worst[k] = std::max(worst[k], st.worst_rel_residual_in_batch);
            solves[k] += st.solves_in_batch; missed[k] += st.unconverged_solves; esc[k] |= st.escalated;
            acc[k] = st;
            g->h[k]->group_batches++;
        }
        done += batch;
    }
    if (done < n_outer) {
        for (int k = 0; k < n; ++k) {
            mvs_deform_stats st{};
            rc = mvs_deform_iterate(g->h[k], pp, n_outer - done, &st);
            if (rc < 0) return rc;
            if (rc > 0) status = rc;
            worst[k] = std::max(worst[k], st.worst_rel_residual_in_batch);
            solves[k] += st.solves_in_batch; missed[k] += st.unconverged_solves; esc[k] |= st.escalated;
            acc[k] = st;
        }
    }
    for (int k = 0; k < n; ++k) {
        mvs_deform_stats& st = acc[k];
        st.outer_done = n_outer;
        st.worst_rel_residual_in_batch = worst[k]; st.solves_in_batch = solves[k]; st.unconverged_solves = missed[k]; st.escalated = esc[k];
        g->h[k]->last = st;
        if (stats) stats[k] = st;
    }
    return status;
}

}  // extern "C"
