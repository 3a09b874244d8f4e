// knobs.h — experiment knobs and the debug trace of libmvs_hip.
//
// Product build: every knob IS its default, a compile-time constant — the library reads no tuning variable from the
// environment.  Diagnostics build (make EXPERIMENTS=1 -> -DMVS_EXPERIMENTS, used by scripts/*.py only): a knob is read from
// the environment ONCE, at its first use, and clamped to [lo, hi]; a malformed or out-of-range value falls back to the
// default.  Nothing is read per pass.
#ifndef MVS_KNOBS_H_
#define MVS_KNOBS_H_
#include <cstdlib>

#ifdef MVS_EXPERIMENTS
inline double mvs_knob_env(const char* name, double dflt, double lo, double hi) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const double v = strtod(e, &end);
    if (end == e || !(v >= lo) || !(v <= hi)) return dflt;
    return v;
}
#define MVS_KNOB(name, dflt, lo, hi) ([]() -> double { static const double v_ = mvs_knob_env(name, dflt, lo, hi); return v_; }())
#else
#define MVS_KNOB(name, dflt, lo, hi) (static_cast<double>(dflt))
#endif

// matchpairs.hip: 64-bit match keys of ONE frame pair that its cascade kernel holds in LDS (a power of two: the bitonic sort pads to
// one).  4096 keys = 32 KiB of the CU's 160 KB, so four workgroups (one per SIMD's worth of waves at 256 threads) stay resident on
// a CU, and SIFT leaves a few thousand raw matches per frame pair at most; a larger bucket sorts in a global-memory workspace.  Not
// an experiment knob: MVS_MATCH_PAIRS_LDS_CAP (environment, read at every call) can only lower it and never changes a result.
#define MVS_MATCH_PAIRS_LDS_KEYS 4096

// depth_sgm.hip: megabytes of device memory that the two uint16 volumes (C and S, 4 bytes per pixel and level) of one group of frames
// may take when mvs_depth_aggregate_params.max_volume_mb is 0.  A 640 x 480 frame at 128 levels and N = 7 needs 143 MB, so a group holds
// 28 such frames: 13000 rows for the row family, more waves than the device has slots.  The grouping never changes a result.
#define MVS_SGM_VOLUME_MB 4096

// trace level of the host side: MVS_DEBUG_CG=1 (plans, verdicts, set-up laps) or 2 (+ residual histories) in the
// environment when the library is loaded; read once (runtime.cpp), 0 otherwise.  It changes no result.
int mvs_debug_level();

#endif
