// assoc_dev.h — the rules of the correspondence search (R/Deformation/Deformation.cpp:286-353), each stated ONCE for every search
// path of assoc.hip: the projection keys of a target point, the wave-resident sorted top-k list, the merge slots of a heavy node's
// workgroup and their exact rank merge, the record write and the node verdict (means, rejection tests, node target).  The searches
// of assoc.hip (select_node, near_nodes, heavy_bounded, k_assoc_merge) differ in how they FIND the members of a node's ball; what
// they do with them is this file.  The results must be the oracle's bit for bit: a change here changes every path at once.
#ifndef MVS_ASSOC_DEV_H_
#define MVS_ASSOC_DEV_H_

#include "engine.h"
#include "dev_common.h"
#include "grid_dev.h"

namespace {

// ------------------------------------------------------------------ time stamps (diagnostics build, -DMVS_STAMPS) ----
// One line per stamp in the searches; without MVS_STAMPS every macro is empty.  ASTAMP_BEGIN starts a search's clock (t0_),
// ASTAMP_LAP stores the cycles since then; ASTAMP_AT / ASTAMP_AT_ISSUE read the clock into a variable of the caller's, after
// draining the wave's memory operations or without; ASTAMP_PUT stores a value under a condition; ASTAMP_ONLY is code of the
// diagnostics build alone.
#ifdef MVS_STAMPS
__device__ unsigned long long g_wave_stamps[8 * 20000];       // k_assoc_local: start / end of every one-wave workgroup
__device__ unsigned long long g_assoc_cycles[2 * 16384];      // per node: cycles of k_assoc_dmin, k_assoc_select
__device__ unsigned long long g_dmin_shell[16384 * 8];        // per node: cycles at the end of coarse shells 0..5, cycles at the start of the coarse walk
__device__ unsigned long long g_all_stamps[4 * 4096];         // k_assoc_all: per workgroup {start, end (100 MHz constant clock), section, work items}
template <bool REAL = false> __device__ __forceinline__ unsigned long long stamp_issue() {         // the clock, whatever is in flight
    unsigned long long t;
    if (REAL) asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    else asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
template <bool REAL = false> __device__ __forceinline__ unsigned long long stamp_drained() {       // ... after the wave's memory operations
    unsigned long long t;
    if (REAL) asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#define ASTAMP_ONLY(...) __VA_ARGS__
#define ASTAMP_AT_ISSUE(var) const unsigned long long var = stamp_issue()
#define ASTAMP_AT(var) const unsigned long long var = stamp_drained()
#define ASTAMP_PUT(cond, dst, val) do { if (cond) (dst) = (val); } while (0)
#define ASTAMP_BEGIN ASTAMP_AT_ISSUE(t0_)
#define ASTAMP_LAP(cond, dst) do { ASTAMP_AT(t1_); ASTAMP_PUT(cond, dst, t1_ - t0_); } while (0)
#else
#define ASTAMP_ONLY(...)
#define ASTAMP_AT_ISSUE(var)
#define ASTAMP_AT(var)
#define ASTAMP_PUT(cond, dst, val) do {} while (0)
#define ASTAMP_BEGIN
#define ASTAMP_LAP(cond, dst) do {} while (0)
#endif
#define ASTAMP_END(slot) ASTAMP_LAP((threadIdx.x & 63) == 0 && node < 16384, g_assoc_cycles[2 * node + (slot)])

// ------------------------------------------------------------------ projection keys ----
// projLen / projDist of target point tp against the node (orig, normal nn of length nlen), Deformation.cpp:330-335
struct ProjKeys { double pd, pl; };
__device__ __forceinline__ ProjKeys proj_keys(d3 orig, d3 nn, double nlen, d3 tp) {
    const d3 dir = tp - orig;                                 // :331
    const double pl = dot3(dir, nn) / nlen;                   // :332
    const double x = sqn3(dir) - pl * pl;
    return {sqrt((0.0 < x) ? x : 0.0), pl};                   // :334, clamped (Appendix A.2)
}
// float32 radix key of a projection distance: rounding is monotone and pd >= +0, so the bit patterns order like the values (NaN: +inf)
__device__ __forceinline__ unsigned proj_dist_key(double pd) {
    const float f = (float)pd;
    return (f == f) ? __float_as_uint(f) : 0x7f800000u;
}
// the total order of the candidates: (projDist, |projLen|, index)
__device__ inline bool key_less(double pd_a, double apl_a, long long i_a, double pd_b, double apl_b, long long i_b) {
    if (pd_a != pd_b) return pd_a < pd_b;
    if (apl_a != apl_b) return apl_a < apl_b;
    return i_a < i_b;
}

// ------------------------------------------------------------------ merge slots of a heavy node's workgroup ----
#ifndef MVS_HEAVY_WAVES
#define MVS_HEAVY_WAVES 16
#endif
constexpr int HEAVY_WAVES = MVS_HEAVY_WAVES;                // waves of a workgroup that takes a heavy node (16, or 8: two such workgroups to a CU)
constexpr int HEAVY_RANGES = 2048;
constexpr int HEAVY_CAND = 10240;                           // members of a ball the workgroup list holds (>= params.max_result = 10000)
constexpr int HEAVY_PIECE = 256;                            // a listed cell is dealt out in pieces of this many points
constexpr int HEAVY_ROWS = 25;                              // rows of the ball's bounding box above which a node is deferred
struct HeavyLds { double pd[HEAVY_WAVES][8], pl[HEAVY_WAVES][8], x[HEAVY_WAVES][8], y[HEAVY_WAVES][8], z[HEAVY_WAVES][8];
                  long long idx[HEAVY_WAVES][8]; int nb[HEAVY_WAVES], np[HEAVY_WAVES];
                  int nr, ra[HEAVY_RANGES], rb[HEAVY_RANGES];         // occupied coarse cells of the ball, found by all waves
                  float fmin[HEAVY_WAVES];                            // per-wave nearest distances of dmin_coarse_wg
                  int next;                                           // next piece of the range list nobody has taken yet
                  int hist[256], sel_bin, sel_before, nwin, npass;    // radix select of the 8th smallest (float) projection distance
                  int cand[HEAVY_CAND];                               // ball members (sorted-order indices) found by phase 1 of the listed pieces
                  int len[HEAVY_WAVES];                               // live entries of each wave's list (rank merge)
                  double r_pd[8], r_pl[8], r_x[8], r_y[8], r_z[8]; long long r_idx[8];   // the merged list, best first
                  int ball;                                           // ball members counted so far by all waves (full-result cut-off)
                  unsigned w8[HEAVY_WAVES][8], T; int ovf; };         // bounded pass (heavy_bounded): the waves' smallest keys, the threshold, "does not fit"

// the members at or below the float threshold T (ukey: proj_dist_key of this thread's members of lds->cand, 0xffffffff = none),
// recomputed in fp64 into the merge slots; lds->nwin counts them, also the ones that found no slot
template <int PARTS, int KMAX>
__device__ __forceinline__ void slots_fill(const GridDev& g, HeavyLds* lds, const unsigned (&ukey)[KMAX], unsigned T, int tid, d3 orig, d3 nn, double nlen) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (ukey[k] <= T && ukey[k] != 0xffffffffu) {
            const int slot = atomicAdd(&lds->nwin, 1);
            if (slot < PARTS * 8) {
                const int i = lds->cand[k * 64 * PARTS + tid];
                const d3 tp = ld3(g.tpos + 3 * (int64_t)i);
                const ProjKeys key = proj_keys(orig, nn, nlen, tp);
                lds->pd[slot >> 3][slot & 7] = key.pd;
                lds->pl[slot >> 3][slot & 7] = key.pl;
                lds->x[slot >> 3][slot & 7] = tp.x; lds->y[slot >> 3][slot & 7] = tp.y; lds->z[slot >> 3][slot & 7] = tp.z;
                lds->idx[slot >> 3][slot & 7] = g.index_base + (long long)__float_as_int(g.spos[i].w);
            }
        }
    }
}
// The PARTS * 8 slots merged by RANK (all PARTS * 64 threads, between two workgroup barriers of the caller's): every live slot
// (idx >= 0) counts how many others precede it in the total order (8 lanes per slot, PARTS comparisons each) and the ones with
// fewer than top_k predecessors ARE the node's list, at the position their count says -> lds->r_*.  (One wave re-inserting all
// candidates took 20-30 K cycles at the end of every heavy node's chain; a tree of pairwise insertions still 33 K.)
template <int PARTS>
__device__ __forceinline__ void slots_rank(HeavyLds* lds, int top_k) {
    const int cand = (int)(threadIdx.x >> 3), chunk = (int)(threadIdx.x & 7);      // PARTS * 64 threads: PARTS * 8 slots x 8 lanes
    const int cw = cand >> 3, cl = cand & 7;
    const long long my_i = lds->idx[cw][cl];
    const double my_pd = lds->pd[cw][cl], my_apl = fabs(lds->pl[cw][cl]);
    int before = 0;
    for (int k = 0; k < PARTS; ++k) {
        const int j = chunk * PARTS + k, jw = j >> 3, jl = j & 7;
        const long long o_i = lds->idx[jw][jl];
        if (o_i >= 0 && key_less(lds->pd[jw][jl], fabs(lds->pl[jw][jl]), o_i, my_pd, my_apl, my_i)) ++before;
    }
    before += __shfl_xor(before, 1, 64); before += __shfl_xor(before, 2, 64); before += __shfl_xor(before, 4, 64);
    if (chunk == 0 && my_i >= 0 && before < top_k) {
        lds->r_pd[before] = my_pd; lds->r_pl[before] = lds->pl[cw][cl];
        lds->r_x[before] = lds->x[cw][cl]; lds->r_y[before] = lds->y[cw][cl]; lds->r_z[before] = lds->z[cw][cl];
        lds->r_idx[before] = my_i;
    }
}

// ------------------------------------------------------------------ sorted top-k list ----
// value of the lane below (lane 0 of a 16-lane row keeps its own): DPP row_shr:1, one VALU move per 32 bits.  The
// candidate lists live in lanes 0..7 (top_k <= 8), so the row-local shift is all an insertion needs (__shfl_up would
// go through the LDS crossbar: ~12 ds_bpermute per insertion).
__device__ inline int shr1_i(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false); }
__device__ inline long long shfl_up_ll(long long b) {
    const int lo = shr1_i((int)(b & 0xffffffffLL));
    const int hi = shr1_i((int)(b >> 32));
    return ((long long)hi << 32) | (unsigned int)lo;
}
__device__ inline double shfl_up_d(double v) { return __longlong_as_double(shfl_up_ll(__double_as_longlong(v))); }

// one element of a node's list
struct Cand { double pd, pl, x, y, z; long long idx; };

// wave-resident sorted list: lane i (< len) holds the i-th best candidate; the key of the top_k-th element is the threshold
struct TopK {
    double L_pd = 0, L_pl = 0, L_x = 0, L_y = 0, L_z = 0;
    long long L_idx = -1;
    int len = 0;
    double t_pd = 0, t_apl = 0; long long t_idx = 0;
#ifdef MVS_STAMP_INSERT
    unsigned long long ins_cycles = 0, ins_count = 0;
    int stamp_node = -1;                                     // >= 0: cycles and count of this node's insertions -> g_assoc_cycles
#endif
    // the lanes' candidates (has: this lane holds one) into the list: a ballot, twelve lane reads and six fp64 row shifts each
    __device__ __forceinline__ void insert(int top_k, bool has, double pd, double pl, d3 tp, long long gi) {
        const int lane = threadIdx.x & 63;
#ifdef MVS_STAMP_INSERT
        ASTAMP_AT_ISSUE(ti0_);
#endif
        const double apl = fabs(pl);
        unsigned long long pend = __ballot(has && (len < top_k || key_less(pd, apl, gi, t_pd, t_apl, t_idx)));
        while (pend) {
            const int src = __ffsll((long long)pend) - 1;
            const double c_pd = rl_d(pd, src), c_pl = rl_d(pl, src);
            const double c_x = rl_d(tp.x, src), c_y = rl_d(tp.y, src), c_z = rl_d(tp.z, src);
            const long long c_i = rl_ll(gi, src);
            const bool less = lane < len && key_less(L_pd, fabs(L_pl), L_idx, c_pd, fabs(c_pl), c_i);
            const int pos = __popcll(__ballot(less));
            const double u_pd = shfl_up_d(L_pd), u_pl = shfl_up_d(L_pl);
            const double u_x = shfl_up_d(L_x), u_y = shfl_up_d(L_y), u_z = shfl_up_d(L_z);
            const long long u_i = shfl_up_ll(L_idx);
            if (lane > pos && lane <= len && lane < top_k) {
                L_pd = u_pd; L_pl = u_pl; L_x = u_x; L_y = u_y; L_z = u_z; L_idx = u_i;
            } else if (lane == pos) {
                L_pd = c_pd; L_pl = c_pl; L_x = c_x; L_y = c_y; L_z = c_z; L_idx = c_i;
            }
            len = min(len + 1, top_k);
            if (len == top_k) {
                t_pd = rl_d(L_pd, top_k - 1); t_apl = fabs(rl_d(L_pl, top_k - 1)); t_idx = rl_ll(L_idx, top_k - 1);
            }
            if (lane == src) has = false;
            pend = __ballot(has && (len < top_k || key_less(pd, apl, gi, t_pd, t_apl, t_idx)));
#ifdef MVS_STAMP_INSERT
            ++ins_count;
#endif
        }
#ifdef MVS_STAMP_INSERT
        ASTAMP_AT_ISSUE(ti1_);
        ins_cycles += ti1_ - ti0_;
        if (stamp_node >= 0 && lane == 0 && stamp_node < 16384) g_assoc_cycles[2 * stamp_node] = ins_cycles | (ins_count << 32);
#endif
    }
    // this wave's list into its row of the merge slots (lanes 0..7)
    __device__ __forceinline__ void to_slots(HeavyLds* lds, int part, int lane) const {
        const bool live = lane < len;
        lds->pd[part][lane] = L_pd; lds->pl[part][lane] = L_pl; lds->x[part][lane] = L_x; lds->y[part][lane] = L_y; lds->z[part][lane] = L_z;
        lds->idx[part][lane] = live ? L_idx : -1;
    }
    // the first n of the ranked slots (slots_rank) become the list
    __device__ __forceinline__ void from_ranked(const HeavyLds* lds, int n, int lane) {
        len = n;
        if (lane < len) { L_pd = lds->r_pd[lane]; L_pl = lds->r_pl[lane]; L_x = lds->r_x[lane]; L_y = lds->r_y[lane]; L_z = lds->r_z[lane]; L_idx = lds->r_idx[lane]; }
    }
    // the lane's own element, and element sidx (uniform) for every lane
    __device__ __forceinline__ Cand own(int) const { return {L_pd, L_pl, L_x, L_y, L_z, L_idx}; }
    __device__ __forceinline__ Cand at(int sidx) const { return {rl_d(L_pd, sidx), rl_d(L_pl, sidx), rl_d(L_x, sidx), rl_d(L_y, sidx), rl_d(L_z, sidx), 0}; }
};

// ------------------------------------------------------------------ node output ----
// `list` is where a finished list of `len` elements lives: a TopK (lane registers) or the NearSlots of a 16-lane group (LDS);
// own(l) is the element of lane l (< 8) itself, at(sidx) element sidx for every lane.

// the records of the node's list (8, the dead ones empty) and the node's counts {ball members, members that face the node}
template <class List>
__device__ __forceinline__ void write_records(mvs_cand* __restrict__ rec, int32_t* __restrict__ counts, int64_t node, int l, const List& list, int len,
                                              int n_ball, int n_pass) {
    if (l < 8) {
        mvs_cand* o = rec + node * 8 + l;
        const bool live = l < len;
        const Cand c = list.own(l);
        o->proj_dist = live ? c.pd : 0.0;
        o->proj_len = live ? c.pl : 0.0;
        o->pos[0] = live ? c.x : 0.0; o->pos[1] = live ? c.y : 0.0; o->pos[2] = live ? c.z : 0.0;
        o->index = live ? c.idx : -1;
    }
    if (l == 0) { counts[2 * node] = n_ball; counts[2 * node + 1] = n_pass; }
}

// The node target: means over the list, best first (Deformation.cpp:338-349), the rejection tests — a full radiusSearch result
// and an empty list (:286-297, :315), the mean projection length / distance (:350), the angle of the mean direction (:352-353) —
// and the stores: controls (the node itself when rejected, :271-272), valid, the list's indices (top_idx may be NULL).
// th: LocalMerge or mvs_deform_params (proj_len_err, proj_dist_err, min_cos, max_result); `ball`: the node's ball count
template <class Thresholds, class Ball, class List>
__device__ __forceinline__ void node_verdict(const Thresholds& th, d3 orig, d3 nn, Ball ball, const List& list, int len, int l, int64_t node,
                                             double* __restrict__ controls, uint8_t* __restrict__ valid, int64_t* __restrict__ top_idx) {
    bool ok = ball < (Ball)th.max_result && len > 0;
    d3 mp = orig;
    double m_pl = 0, m_pd = 0;
    d3 acc = mk3(0, 0, 0);
    for (int sidx = 0; sidx < len; ++sidx) {                  // :341-346, best first
        const Cand c = list.at(sidx);
        m_pl += c.pl; m_pd += c.pd;
        acc = acc + mk3(c.x, c.y, c.z);
    }
    if (ok) {
        const double dn = (double)len;
        m_pl /= dn; m_pd /= dn; acc = acc / dn;               // :347-349
        if (m_pl >= th.proj_len_err || m_pd >= th.proj_dist_err) ok = false;          // :350
        if (ok) {
            const d3 dir = acc - orig;                        // :352-353
            if (fabs(dot3(dir, nn) / (norm3(dir) * norm3(nn))) < th.min_cos) ok = false;
        }
        if (ok) mp = acc;
    }
    if (top_idx && l < 8) top_idx[node * 8 + l] = (ball < (Ball)th.max_result && len > 0 && l < len) ? list.own(l).idx : -1;
    if (l == 0) { valid[node] = ok ? 1 : 0; st3(controls + 3 * node, mp); }   // :355-356
}

}  // namespace

#endif
