// deform_timing.cpp — HIP-event timing of the deformation passes (mvs_deform_enable_timing / _kernel_time) and the sweep
// sampling of timing mode 3.  State: mvs_deform_s::timing (engine.h).
#include "deform_host.h"

static hipEvent_t get_event(mvs_deform_s* h) {
    auto& T = h->timing;
    if (!T.event_pool.empty()) { hipEvent_t e = T.event_pool.back(); T.event_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
// timing: 0 off, 1 every phase, 2 only the global-solve groups ("cg": the planned sweeps of a solve, "tail": its last launch; two
// events per group: +30 us and more per outer iteration of the metric workload, scripts/timing_overhead.py), 3 the planned sweeps
// of every EIGHTH pass (what bench.py keeps on inside its timed region — the sampled passes hold the same launch mix as the others)
bool timed(const mvs_deform_s* h, const char* name) {
    if (h->timing.mode == 1) return true;
    const bool cg = std::strcmp(name, "cg") == 0, tail = std::strcmp(name, "tail") == 0;
    if (!cg && !tail) return false;
    // (an event pair costs ~4 us of stream time — the marker packets break the back-to-back dispatch of the launches around them:
    //  bench.py's timed region keeps only the pair around the planned sweeps of every EIGHTH pass, ~0.2 % of a step)
    return h->timing.mode == 2 || (cg && h->timing.mode == 3 && (h->seq_enqueued & 7) == 0);
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
    t.h->timing.pending.push_back({t.name, {t.a, b}});
    t.h->timing.pending_launches[t.name] += launches;
}
void collect_timers(mvs_deform_s* h) {
    // (mode 3) the k-th "cg" bracket of the pending list is the k-th sampled solve: its launches that found the solve finished are
    // counted from the flags copied out behind its pass (the stream has been synchronised: the copies have landed), and the
    // bracket is also filed under its composition — "cg:a<active>:i<idle>": total ms, number of brackets — so that a caller
    // can separate the cost of an active launch from that of an idle one and from the bracket's own overhead (bench.py)
    auto& T = h->timing;
    size_t k_cg = 0, q = 0;
    for (auto& pr : T.pending) {
        float ms = 0;
        const bool okms = hipEventElapsedTime(&ms, pr.second.first, pr.second.second) == hipSuccess;
        if (okms) T.timers[pr.first].total_ms += ms;
        if (T.mode == 3 && pr.first == "cg" && k_cg < T.samples.size()) {
            while (q + 1 < T.sample_off.size() && (size_t)T.sample_pass_first[q + 1] <= k_cg) ++q;
            const auto& sm = T.samples[k_cg++];
            const double* F = T.h_sample + T.sample_off[q];
            int idle = 0;
            for (int i = 0; i < sm.n_a; ++i) if (F[(size_t)(sm.first + i) * 8 + 6] != 0.0) ++idle;
            T.timers["cg_idle"].launches += idle;
            char key[48];
            snprintf(key, sizeof key, "cg:a%d:i%d", sm.n_a - idle, idle);
            if (okms) { T.timers[key].total_ms += ms; T.timers[key].launches += 1; }
        }
        T.event_pool.push_back(pr.second.first);
        T.event_pool.push_back(pr.second.second);
    }
    T.pending.clear();
    for (auto& kv : T.pending_launches) T.timers[kv.first].launches += kv.second;
    T.pending_launches.clear();
    T.samples.clear(); T.sample_off.clear(); T.sample_pass_first.clear(); T.sample_used = 0;
}

// (timing mode 3) room for one more sampled pass's slot scalars in the pinned buffer?  Allocated at the first sampled pass.
bool sample_room(mvs_deform_s* h, int64_t nslots) {
    auto& T = h->timing;
    if (!T.h_sample) {
        void* hp = nullptr;
        const size_t cap = (size_t)64 * 8 * 64;                              // 64 passes of 64 slots (a pass holds 20-40)
        if (hipHostMalloc(&hp, cap * sizeof(double), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        T.h_sample = (double*)hp; T.sample_cap = cap; T.sample_used = 0;
    }
    return T.sample_used + (size_t)nslots * 8 <= T.sample_cap;
}

extern "C" {

int mvs_deform_enable_timing(mvs_deform_t h, int on) {
    if (!h) return MVS_E_INVALID_ARG;
    auto& T = h->timing;
    T.mode = on;
    T.timers.clear();
    T.samples.clear(); T.sample_off.clear(); T.sample_pass_first.clear(); T.sample_used = 0;
    return MVS_OK;
}
int mvs_deform_kernel_time(mvs_deform_t h, const char* name, double* total_ms, int64_t* launches) {
    if (!h || !name) return MVS_E_INVALID_ARG;
    auto it = h->timing.timers.find(name);
    if (total_ms) *total_ms = it == h->timing.timers.end() ? 0.0 : it->second.total_ms;
    if (launches) *launches = it == h->timing.timers.end() ? 0 : it->second.launches;
    return MVS_OK;
}

}  // extern "C"
