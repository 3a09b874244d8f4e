// deform_test.cpp — the test hooks of include/mvs_test.h (not part of the ABI of include/mvs.h): all state they set lives in
// the handle (mvs_deform_s::dbg, engine.h).
#include "deform_host.h"
#include "../../include/mvs_test.h"

extern "C" {

// the heavy list of the last association — entries, and how many of them had their coarse nearest-distance walk deferred
int mvs_test_heavy_count(mvs_deform_t h, int* n, int* flagged) {
    if (!h || !h->d_heavy) return MVS_E_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    const int32_t* cur = assoc_lists(h, h->heavy_flip ^ 1).heavy;       // (the list the LAST association filled)
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
    h->dbg.maxspin = maxspin > 0 ? maxspin : 0;
    h->dbg.plan_cap = plan_cap > 0 ? plan_cap : 0;
    h->dbg.skip_wg = skip_wg >= 0 ? skip_wg : -1;
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
    h->dbg.group_leave = after_batches > 0 ? after_batches : 0;
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

}  // extern "C"
