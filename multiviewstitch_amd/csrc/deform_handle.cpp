// deform_handle.cpp — life cycle and plain state of a deformation handle (include/mvs.h, mvs_deform_*): parameters, create /
// destroy, node sets, vertices, targets, stream, read-back; mvs_knn_points.
#include "deform_host.h"
#include <chrono>

int check_params(const mvs_deform_params* p) {
    if (!p) { mvs_set_error("params is NULL"); return MVS_E_INVALID_ARG; }
    if (p->top_k < 1 || p->top_k > 8 || p->graph_k < 0 || p->graph_k > 63 || p->smooth_sweeps < 0 ||
        p->arap_iters < 1 || p->arap_iters > 8 || p->cg_max_iters < 1 || !(p->cg_tol > 0)) {
        mvs_set_error("params out of range (top_k 1..8, graph_k 0..63, arap_iters 1..8, cg_tol > 0)");
        return MVS_E_INVALID_ARG;
    }
    return MVS_OK;
}

static void free_nodes(mvs_deform_s* h) {
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

int ready(mvs_deform_t h, const mvs_deform_params* p, bool need_target) {
    if (!h) { mvs_set_error("handle is NULL"); return MVS_E_INVALID_ARG; }
    int rc = check_params(p);
    if (rc) return rc;
    if (need_target && !h->has_target) { mvs_set_error("no target set: call mvs_deform_set_target first"); return MVS_E_STATE; }
    if (h->K == 0) { mvs_set_error("no nodes: call mvs_deform_sample_nodes / _set_nodes first"); return MVS_E_STATE; }
    return mvs_check_hip(hipSetDevice(h->device), "hipSetDevice");
}

extern "C" {

void mvs_deform_default_params(mvs_deform_params* p) {
    if (!p) return;
    p->proj_len_err = 100.0; p->proj_dist_err = 100.0; p->min_cos = 0.1;
    p->max_result = 10000; p->top_k = 8; p->graph_k = 8; p->smooth_sweeps = 2;
    p->arap_iters = 5; p->arap_tol = 1e-4; p->cg_tol = 1e-8; p->cg_max_iters = 2000;
    p->update_normals = 0;
    p->solver = MVS_SOLVER_AUTO; p->reserved0 = 0;
}

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
    if (h->d_slots) (void)hipFree(h->d_slots);
    if (h->d_cheb) (void)hipFree(h->d_cheb);
    if (h->d_sh) { (void)hipFree(h->d_sh); h->d_sh = nullptr; }
    if (h->h_ctl) { (void)hipHostFree((void*)h->h_ctl); h->h_ctl = nullptr; }
    if (h->timing.h_sample) { (void)hipHostFree(h->timing.h_sample); h->timing.h_sample = nullptr; }
    for (auto& pr : h->timing.pending) { (void)hipEventDestroy(pr.second.first); (void)hipEventDestroy(pr.second.second); }
    for (hipEvent_t e : h->timing.event_pool) (void)hipEventDestroy(e);
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

}  // extern "C"
