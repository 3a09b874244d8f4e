// deform_iterate.cpp — the stepping entries of a handle (include/mvs.h): mvs_deform_iterate, the sharded association entries,
// _solve / _collect / _arap, _solver_info.  They compose deform_pass.cpp (what a pass launches) and deform_plan.cpp (how long its
// solves are planned, what a harvest reads back).
#include "deform_host.h"

extern "C" {

int mvs_deform_iterate(mvs_deform_t h, const mvs_deform_params* p, int n_outer, mvs_deform_stats* stats) {
    MVS_TRACE();
    int rc = ready(h, p, true);
    if (rc) return rc;
    if (n_outer < 0) return MVS_E_INVALID_ARG;
    int done = 0;
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
    BatchAcc acc;
    acc.st = h->last;
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
        mvs_deform_stats st;
        rc = harvest(h, *p, cg, &st);
        if (rc < 0) return rc;
        if (rc > 0) status = rc;
        acc.add(st);
        done += batch;
    }
    acc.finish(&h->last, done);
    if (stats) *stats = h->last;
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
    return harvest(h, *p, cg, stats);
}
int mvs_deform_collect(mvs_deform_t h, const mvs_deform_params* p, mvs_deform_stats* stats) {
    MVS_TRACE();
    int rc = ready(h, p, false);
    if (rc) return rc;
    if (h->cg_iters <= 0) { mvs_set_error("nothing enqueued: the first mvs_deform_iterate / _solve of a handle runs synchronously"); return MVS_E_STATE; }
    return harvest(h, *p, probe_cg(h, *p), stats);
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
    return harvest(h, *p, cg, stats);
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

}  // extern "C"
