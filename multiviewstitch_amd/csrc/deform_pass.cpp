// deform_pass.cpp — the launch sequence of one pass of a handle: the association of the nodes against the handle's (local)
// target, then graph smoothing, the global solves of the ARAP iterations and the geometry update.
#include "deform_host.h"

AssocLists assoc_lists(const mvs_deform_s* h, int flip) {
    if (flip) return {h->d_heavy2, h->d_heavy, h->d_mid2, h->d_mid};
    return {h->d_heavy, h->d_heavy2, h->d_mid, h->d_mid2};
}

// association of the handle's nodes against the handle's (local) target, nranks = 1
void enqueue_assoc_local(mvs_deform_s* h, const mvs_deform_params& p) {
    Tic t = tic(h, "assoc");
    const int K = (int)h->K;
    const AssocLists l = assoc_lists(h, h->heavy_flip);
    int32_t *cur = l.heavy, *nxt = l.heavy_next, *mcur = l.mid, *mnxt = l.mid_next;
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

namespace {

// what the stages of a pass hand on: the solution buffer the next launch reads, the next sweep slot, the 8 scalars of the last
// sweep slot of the previous solve (idle flag, sweeps that ran), whether this pass is a sampled one of timing mode 3
struct SolveState {
    double* x_cur;                       // the patch solver ping-pongs between d_sol and d_ras_x2
    int64_t ras_slot = 0;
    const double* prev_scal = nullptr;
    bool sampling = false;
};
// the node targets the solve starts from (after all smoothing sweeps but the one k_ras_prepare performs: last_sweep)
struct Smoothed { const double* ctrl; bool weights_done = false; RasSmooth last_sweep{nullptr, nullptr, 0, nullptr}; };

// node graph + smoothing sweeps
int graph_and_smooth(mvs_deform_s* h, const mvs_deform_params& p, Smoothed* out) {
    hipStream_t s = h->stream;
    const int K = (int)h->K;
    const double* ctrl = out->ctrl;
    bool weights_done = false;
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
        double* o = bufs[(p.smooth_sweeps - 1) & 1];
        out->last_sweep = RasSmooth{h->d_node_pts, h->d_nbr, nn, o};
        h->d_ctrl_final = o;
    }
    out->ctrl = ctrl; out->weights_done = weights_done;
    return MVS_OK;
}

// cotangent weights (unless they came with an association launch) and the start of the solve
void weights_and_prepare(mvs_deform_s* h, const Smoothed& sm, bool ras) {
    hipStream_t s = h->stream;
    const double* ctrl = sm.ctrl;
    Tic t = tic(h, "weights");
    if (sm.weights_done) {
        launch_ras_prepare(h, s, ctrl, sm.last_sweep);                                                // set_target_position :383-392
        toc(t, 1);
    } else {
        launch_cot_weights(h->sell, h->d_pts, ras ? nullptr : h->d_coef, ctrl, h->d_sol, h->d_rot, s);   // preprocess() :393 + set_target_position :383-392
        if (ras) launch_ras_prepare(h, s);
        toc(t, 2);
    }
}

// what the launches of a patch-solver pass share
struct RasPass {
    int slot;                // this pass's row of the residual ring (MVS_CTL_RING)
    bool fused;              // the last planned launch of every solve ends with the ARAP local step on its patches' owned rows (schwarz.hip)
    bool safe_local;         // a k_arap_local launch of its own follows every solve all the same (enqueue_solve)
    int nl;                  // partial sums per reduction the local step leaves, whoever performs it
    int demand_local;        // the judge of a solve insists that its fused local step ran
};

// one sweep launch of solve `it`, from st.x_cur into the other solution buffer, on the next sweep slot
void ras_sweep(mvs_deform_s* h, const mvs_deform_params& p, const RasPass& c, int it, int i, bool last, SolveState& st) {
    const int ss = ras_slot_size(h);
    double* x_next = st.x_cur == h->d_sol ? h->d_ras_x2 : h->d_sol;
    double* cur = h->d_ras_slots + (size_t)st.ras_slot * ss;
    // the last planned sweep of a solve is a TAIL launch: should the plan turn out too short it keeps sweeping in
    // the kernel (its extra sweeps' partial sums go to the solve's tail slots)
    launch_ras_sweep(h, h->d_ras_b, st.x_cur, x_next, it, p.arap_tol, i, p.cg_tol, STOP_AT, i > 0 ? cur - ss : nullptr, cur,
                     h->d_ras_iters + (size_t)st.ras_slot * h->ras.NP, h->stream, last ? h->d_ras_tail + (size_t)it * RAS_TAIL_MAX * ss : nullptr, c.fused,
                     h->ras_mix_any != 0);
    st.x_cur = x_next;
    ++st.ras_slot;
}

// the global solves of the ARAP iterations, patch solver
void ras_solves(mvs_deform_s* h, const mvs_deform_params& p, const RasPlan& rp, const RasPass& c, SolveState& st) {
    hipStream_t s = h->stream;
    for (int it = 0; it < p.arap_iters; ++it) {
        {
            Tic t = tic(h, "rhs");
            launch_arap_rhs(h->sell, h->d_pts, st.x_cur, h->d_rot, it, p.arap_tol, h->d_energy, nullptr, nullptr, h->d_ras_b, p.cg_tol, h->d_ctl, c.slot, st.prev_scal, h->d_bar, h->d_bpure, s,
                            c.nl, c.demand_local);
            toc(t, 1);
        }
        {
            Tic t = (h->timing.mode == 3 && !st.sampling) ? Tic{h, "cg", nullptr} : tic(h, "cg");      // (mode 3 times exactly the sampled brackets)
            // ("cg" = the planned sweeps, "tail" = the solve's last launch — in fused mode the deciding launch + the local step)
            // Sampled passes of timing mode 3: which of the bracketed launches did work is READ BACK (the idle flags of this pass's
            // sweep slots are copied out behind the pass); collect_timers files every bracket under its composition.
            const int planned = rp.n[it] - 1;
            if (st.sampling) h->timing.samples.push_back({(int)st.ras_slot, planned, 0});
            for (int i = 0; i < planned; ++i) ras_sweep(h, p, c, it, i, false, st);
            toc(t, planned);
            Tic tl = tic(h, "tail");
            ras_sweep(h, p, c, it, rp.n[it] - 1, true, st);
            toc(tl, 1);
            st.prev_scal = h->d_ras_slots + (size_t)(st.ras_slot - 1) * ras_slot_size(h) + 3 * (size_t)h->ras.NPpad;
        }
        if (!c.fused || c.safe_local) {
            Tic t = tic(h, "local");
            launch_arap_local(h->sell, h->d_pts, st.x_cur, it, p.arap_tol, h->d_energy, h->d_rot, h->d_bpure, s, c.fused ? h->d_ctl : nullptr, c.nl);
            toc(t, 1);
        }
    }
}

// the global solves of the ARAP iterations, CG
void cg_solves(mvs_deform_s* h, const mvs_deform_params& p, const CgPlan& plan, int slot) {
    hipStream_t s = h->stream;
    for (int it = 0; it < p.arap_iters; ++it) {                                                   // deform(5, 1e-4), :398
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
}

// geometry update (+ normals, node gather) and, on a sampled pass, the copy of its sweep slots' scalars
void finalize_pass(mvs_deform_s* h, const mvs_deform_params& p, const RasPlan& rp, const RasPass& c, const SolveState& st) {
    hipStream_t s = h->stream;
    const int K = (int)h->K, V = (int)h->V;
    double* host_ctl = const_cast<double*>(h->h_ctl);
    Tic t = tic(h, "finalize");
    int n = 1;
    if (p.update_normals) {              // the node normals change too: separate gather after the normals kernel
        launch_arap_finalize(h->sell, p.arap_iters, p.arap_tol, h->d_energy, st.x_cur, h->d_pts, h->d_info, nullptr, nullptr, nullptr, p.cg_tol, h->d_ctl, c.slot, host_ctl, st.prev_scal, s, c.nl, c.demand_local, (double)(h->seq_enqueued + 1));   // :400
        launch_vertex_normals(h->d_pts, h->d_faces, h->d_vf_ptr, h->d_vf, V, h->d_nrm, s);
        launch_gather_nodes(h->d_pts, h->d_nrm, h->d_nodes, K, h->d_node_pts, h->d_node_nrm, s);
        n = 3;
    } else {
        launch_arap_finalize(h->sell, p.arap_iters, p.arap_tol, h->d_energy, st.x_cur, h->d_pts, h->d_info, h->d_nrm, h->d_node_pts, h->d_node_nrm, p.cg_tol, h->d_ctl, c.slot, host_ctl, st.prev_scal, s, c.nl, c.demand_local, (double)(h->seq_enqueued + 1));
    }
    toc(t, n);
    if (st.sampling) {   // the 8 scalars of every sweep slot of this pass -> pinned memory (a few KB, every eighth pass)
        auto& T = h->timing;
        const int ss = ras_slot_size(h);
        const size_t nslots = (size_t)rp.total(p.arap_iters);
        T.sample_off.push_back(T.sample_used);
        (void)hipMemcpy2DAsync(T.h_sample + T.sample_used, 8 * sizeof(double), h->d_ras_slots + 3 * (size_t)h->ras.NPpad, (size_t)ss * sizeof(double),
                               8 * sizeof(double), nslots, hipMemcpyDeviceToHost, s);
        T.sample_used += nslots * 8;
    }
}

}  // namespace

// graph smoothing (optional) + ARAP + geometry update.  ctrl_src: K*3 node targets.
// safe_local: behind every patch solve a k_arap_local launch of its own follows even when the solve's last launch performs the
// local step itself (fused mode) — it returns at once when that happened.  Callers that do not follow the solves (enqueue-only
// batches of several handles sharing the chip, where a tail loop may have to be abandoned) and handles that have seen an
// abandoned solve ask for it; a handle stepping on its own does not pay the extra launch.
int enqueue_solve(mvs_deform_s* h, const mvs_deform_params& p, const double* ctrl_src, bool graph_smooth, const CgPlan& plan, bool safe_local) {
    Smoothed sm;
    sm.ctrl = ctrl_src;
    if (graph_smooth) {
        int rc = graph_and_smooth(h, p, &sm);
        if (rc) return rc;
    }
    if (!sm.last_sweep.out) h->d_ctrl_final = const_cast<double*>(sm.ctrl);
    const bool ras = use_ras(h, p);
    if (ras) update_mix_state(h, p.arap_iters);
    const RasPlan rp = probe_ras(h);
    int rc = ras ? ensure_ras_slots(h, p.arap_iters) : ensure_slots(h, p.arap_iters, plan);
    if (rc) return rc;
    weights_and_prepare(h, sm, ras);
    RasPass c;
    c.slot = (int)(h->seq_enqueued % MVS_RING);
    c.fused = ras && ras_can_fuse_local(h);
    c.safe_local = safe_local || h->saw_abandon;
    c.nl = ras ? ras_local_parts(h) : 0;
    c.demand_local = (c.fused && !c.safe_local) ? 1 : 0;
    SolveState st;
    st.x_cur = h->d_sol;
    st.sampling = ras && h->timing.mode == 3 && timed(h, "cg") && sample_room(h, rp.total(p.arap_iters));
    if (st.sampling) h->timing.sample_pass_first.push_back((int)h->timing.samples.size());
    if (ras) ras_solves(h, p, rp, c, st);
    else cg_solves(h, p, plan, c.slot);
    finalize_pass(h, p, rp, c, st);
    h->graph_ready_nn = 0; h->weights_ready = false;     // the nodes have moved
    h->seq_enqueued++;
    return MVS_OK;
}
