// grabcut.hip — mvs_grid_mincut and mvs_grabcut_masks (include/mvs.h): the foreground mask Image3D::LoadModel makes with Segment 1
// (R/Image3D/Image3D.cpp:23-51), for all frames of a sequence at once.  OpenCV is not part of the reference tree: the rules are this
// library's definition, stated in include/mvs.h; their per-pixel part is grabcut_rules.h, one body for these kernels and for host code.
//
// The cut (rule G1) — per node an int32 excess e, an int32 height h, eight residual capacities rc, direction-major:
//   k_mc_init     the working copy of excess and capacities (an entry that points outside the grid becomes 0) and the extremes of the
//                 input for the headroom test.
//   k_mc_seed     a relabelling starts: h = 0 where e < 0, INF elsewhere.
//   k_mc_relax    a 16 x 16 tile with a halo ring of heights in LDS: at most MC_SWEEPS min-relaxations h(u) = min(h(u), 1 + min h(v)
//                 over rc(u -> v) > 0), halo values as the launch found them.  Values only fall, every value is the length of a
//                 real residual path, and a launch in which no tile changed anything has found the fixed point: the exact distances.
//                 The last launch of a round counts the nodes it changed and the nodes with e > 0 and a finite h.
//   k_mc_push     the same tile with e and rc in LDS too: at most MC_PUSH_ITERS rounds of (decide, barrier, apply): a node with e > 0
//                 and h < nodes pushes min(e, rc) to its lowest residual neighbour when that is lower, else lifts itself above it.
//                 A push inside the tile is four LDS atomics; across the border the neighbour's e and rc get global atomics at once.
//                 At the end the tile adds what it changed (final - loaded) to global memory with atomics and stores its heights:
//                 e(u) and rc(u -> .) are lowered by u's tile alone, so a tile's copy never exceeds the truth and no push overdraws.
//   k_mc_side     source_side = (h == INF).
// A tile reads the heights of its ring with plain loads while the tiles that own them may store new ones in the same launch, and
// k_mc_push reads e and rc of its own nodes while neighbours add to them: formally data races on aligned 32-bit words.  Either
// value serves: in a relabelling heights only fall and any value read is the length of a real path; in a push a stale height only
// misdirects a push and a stale e or rc is a lower bound.  h is nowhere __restrict__, nor are e and rc in k_mc_push.
// Nothing waits: every loop has a constant bound, the host reads one record of counters per round and decides.  Heights steer the
// pushes but prove nothing; the answer is read off a relabelling that converged on a state no kernel is changing.
//
// The segmentation — one launch per step for all frames (a workgroup works inside one frame):
//   k_gc_half, k_gc_start (beta's integer sum, the luma histograms; LDS-privatised, then 64-bit / 32-bit atomics), k_gc_thresholds,
//   k_gc_label0, k_gc_ncap; per iteration k_gc_assign, k_gc_learn (100 uint32 LDS counters per workgroup: 256 pixels cannot overflow
//   them; then int64 atomics) + k_gc_fit, k_gc_excess, the cut, k_gc_update; k_gc_full.  Every sum is an integer: order-free.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "grabcut_rules.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int MC_T = 16, MC_TPB = MC_T * MC_T, MC_HW = MC_T + 2;     // tile side, threads, tile side with the halo ring
constexpr int MC_HINF = 0x3fffffff;
constexpr int MC_SWEEPS = 32, MC_PUSH_ITERS = 16;                    // bounded work per launch
constexpr int MC_RELAX_BATCH = 8, MC_PUSH_BATCH = 4;                 // launches per round
constexpr int MC_CTR = 2;                                            // of a round's last relax launch: nodes changed | nodes active

__host__ __device__ inline int mc_dx(int d) { return (d == 0 || d == 1 || d == 7) ? -1 : ((d == 2 || d == 6) ? 0 : 1); }
__host__ __device__ inline int mc_dy(int d) { return (d >= 1 && d <= 3) ? -1 : ((d == 0 || d == 4) ? 0 : 1); }

struct McDims { int32_t n, gw, gh, tx, ty; int64_t N; };            // grids, grid size, tiles per row / column, nodes per grid

struct McTile { int g, x, y, lx, ly, c; bool in; int64_t node; };   // a thread's node: grid, position, place in the tile, LDS slot of its height
__device__ inline McTile mc_tile(const McDims& q) {
    McTile t;
    const int per = q.tx * q.ty, tile = blockIdx.x % per;
    t.g = blockIdx.x / per;
    t.lx = threadIdx.x % MC_T; t.ly = threadIdx.x / MC_T;
    t.x = (tile % q.tx) * MC_T + t.lx; t.y = (tile / q.tx) * MC_T + t.ly;
    t.in = t.x < q.gw && t.y < q.gh;
    t.c = (t.ly + 1) * MC_HW + t.lx + 1;
    t.node = (int64_t)t.g * q.N + (int64_t)t.y * q.gw + t.x;
    return t;
}
// heights of the tile and its ring into LDS; outside the grid INF
__device__ inline void mc_load_heights(const McDims& q, const McTile& t, const int32_t* h, int* s_h) {
    const int x0 = t.x - t.lx - 1, y0 = t.y - t.ly - 1;
    for (int i = threadIdx.x; i < MC_HW * MC_HW; i += MC_TPB) {
        const int hx = x0 + i % MC_HW, hy = y0 + i / MC_HW;
        s_h[i] = (hx >= 0 && hx < q.gw && hy >= 0 && hy < q.gh) ? h[(int64_t)t.g * q.N + (int64_t)hy * q.gw + hx] : MC_HINF;
    }
}

__global__ __launch_bounds__(MC_TPB) void k_mc_init(McDims q, const int32_t* __restrict__ excess, const int32_t* __restrict__ cap,
                                                    int32_t* __restrict__ e, int32_t* __restrict__ rc, int32_t* __restrict__ stat) {
    const int64_t at = (int64_t)blockIdx.x * MC_TPB + threadIdx.x;
    if (at >= (int64_t)q.n * q.N) return;
    const int64_t g = at / q.N, i = at % q.N;
    const int x = (int)(i % q.gw), y = (int)(i / q.gw);
    const int32_t ex = excess[at];
    e[at] = ex;
    int amax = ex == INT32_MIN ? INT32_MAX : (ex < 0 ? -ex : ex), cmax = 0, cmin = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int nx = x + mc_dx(d), ny = y + mc_dy(d);
        const int64_t k = (g * 8 + d) * q.N + i;
        int32_t c = 0;
        if (nx >= 0 && nx < q.gw && ny >= 0 && ny < q.gh) {
            c = cap[k];
            cmax = c > cmax ? c : cmax;
            cmin = c < cmin ? c : cmin;
        }
        rc[k] = c > 0 ? c : 0;
    }
    if (stat) {                                                      // the plain read only filters: the words move one way
        if (amax > stat[0]) atomicMax(&stat[0], amax);
        if (cmax > stat[1]) atomicMax(&stat[1], cmax);
        if (cmin < stat[2]) atomicMin(&stat[2], cmin);
    }
}

__global__ __launch_bounds__(MC_TPB) void k_mc_seed(int64_t total, const int32_t* __restrict__ e, int32_t* __restrict__ h) {
    const int64_t at = (int64_t)blockIdx.x * MC_TPB + threadIdx.x;
    if (at < total) h[at] = e[at] < 0 ? 0 : MC_HINF;
}

__global__ __launch_bounds__(MC_TPB) void k_mc_relax(McDims q, const int32_t* __restrict__ e, const int32_t* __restrict__ rc,
                                                     int32_t* h, int32_t* __restrict__ ctr) {
    __shared__ int s_h[MC_HW * MC_HW];
    const McTile t = mc_tile(q);
    mc_load_heights(q, t, h, s_h);
    unsigned open = 0;                                               // directions with residual capacity (0 outside the grid: k_mc_init)
    if (t.in) {
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (rc[((int64_t)t.g * 8 + d) * q.N + (t.node - (int64_t)t.g * q.N)] > 0) open |= 1u << d;
    }
    __syncthreads();
    const int h0 = s_h[t.c];
    int my = h0;
    for (int s = 0; s < MC_SWEEPS; ++s) {
        int best = MC_HINF;
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (open >> d & 1u) { const int v = s_h[t.c + mc_dy(d) * MC_HW + mc_dx(d)]; best = v < best ? v : best; }
        const int nv = best < MC_HINF ? best + 1 : MC_HINF;
        const bool ch = t.in && nv < my;
        __syncthreads();                                             // every read of this sweep is done
        if (ch) { my = nv; s_h[t.c] = nv; }
        if (!__syncthreads_or(ch)) break;
    }
    const bool changed = t.in && my != h0;
    if (changed) h[t.node] = my;
    if (!ctr) return;                                                // only a round's last launch is judged
    const int nch = __syncthreads_count(changed);
    const int nact = __syncthreads_count(t.in && my < MC_HINF && e[t.in ? t.node : 0] > 0);
    if (threadIdx.x == 0) {
        if (nch) atomicAdd(&ctr[0], nch);
        if (nact) atomicAdd(&ctr[1], nact);
    }
}

__global__ __launch_bounds__(MC_TPB) void k_mc_push(McDims q, int32_t* e, int32_t* rc, int32_t* h) {
    __shared__ int s_h[MC_HW * MC_HW];
    __shared__ int s_e[MC_TPB];
    __shared__ int s_c[8][MC_TPB];
    const McTile t = mc_tile(q);
    const int tid = threadIdx.x;
    const int64_t gi = t.node - (int64_t)t.g * q.N, cbase = (int64_t)t.g * 8 * q.N + gi;
    const int hcap = q.N < MC_HINF ? (int)q.N : MC_HINF;             // a height of N or more cannot be a distance
    mc_load_heights(q, t, h, s_h);
    const int e0 = t.in ? e[t.node] : 0;
    int c0[8];
    s_e[tid] = e0;
#pragma unroll
    for (int d = 0; d < 8; ++d) { c0[d] = t.in ? rc[cbase + d * q.N] : 0; s_c[d][tid] = c0[d]; }
    __syncthreads();
    const int h0 = s_h[t.c];
    if (!__syncthreads_or(t.in && e0 > 0 && h0 < hcap)) return;      // nothing to push in this tile
    for (int it = 0; it < MC_PUSH_ITERS; ++it) {
        const int ex = s_e[tid], hu = s_h[t.c];
        const bool act = t.in && ex > 0 && hu < hcap;
        int best = MC_HINF, bd = -1, amount = 0, lift = -1;
        if (act) {
#pragma unroll
            for (int d = 0; d < 8; ++d)
                if (s_c[d][tid] > 0) { const int v = s_h[t.c + mc_dy(d) * MC_HW + mc_dx(d)]; if (v < best) { best = v; bd = d; } }
            if (bd >= 0 && hu > best) { const int c = s_c[bd][tid]; amount = ex < c ? ex : c; }
            else lift = best < MC_HINF ? best + 1 : MC_HINF;         // no residual neighbour: INF, inactive
        }
        __syncthreads();                                             // every decision is made on one picture of the tile
        if (amount > 0) {
            const int rd = bd ^ 4, nlx = t.lx + mc_dx(bd), nly = t.ly + mc_dy(bd);
            atomicSub(&s_c[bd][tid], amount);
            atomicSub(&s_e[tid], amount);
            if (nlx >= 0 && nlx < MC_T && nly >= 0 && nly < MC_T) {
                const int nt = nly * MC_T + nlx;
                atomicAdd(&s_c[rd][nt], amount);
                atomicAdd(&s_e[nt], amount);
            } else {                                                 // rc > 0 only towards a node of the grid (k_mc_init, k_gc_ncap)
                const int nx = t.x + mc_dx(bd), ny = t.y + mc_dy(bd);
                if (nx >= 0 && nx < q.gw && ny >= 0 && ny < q.gh) {
                    const int64_t nn = (int64_t)ny * q.gw + nx;
                    atomicAdd(&rc[((int64_t)t.g * 8 + rd) * q.N + nn], amount);
                    atomicAdd(&e[(int64_t)t.g * q.N + nn], amount);
                }
            }
        } else if (lift >= 0) {
            s_h[t.c] = lift;
        }
        if (!__syncthreads_or(act)) break;
    }
    if (!t.in) return;
    const int de = s_e[tid] - e0;
    if (de) atomicAdd(&e[t.node], de);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int dc = s_c[d][tid] - c0[d];
        if (dc) atomicAdd(&rc[cbase + d * q.N], dc);
    }
    if (s_h[t.c] != h0) h[t.node] = s_h[t.c];
}

__global__ __launch_bounds__(MC_TPB) void k_mc_side(int64_t total, const int32_t* __restrict__ h, uint8_t* __restrict__ side) {
    const int64_t at = (int64_t)blockIdx.x * MC_TPB + threadIdx.x;
    if (at < total) side[at] = h[at] == MC_HINF ? 1 : 0;
}

// ---- the cut on the host ----
int check_mc(const char* fn, int32_t n, int32_t gw, int32_t gh, const void* excess, const void* cap, int32_t max_rounds, const void* side, McDims* q) {
    if (!excess || !cap || !side) return bad(fn, "excess, cap or source_side is NULL");
    if (n < 1 || gw < 1 || gh < 1) return bad(fn, "need n, gw, gh >= 1");
    if ((int64_t)gw * gh > (1LL << 26)) return bad(fn, "gw * gh must not exceed 2^26");
    if ((int64_t)n * gw * gh > 0x7fffffffLL) return bad(fn, "n * gw * gh must not exceed 2^31 - 1");
    if (max_rounds < 1) return bad(fn, "need max_rounds >= 1");
    q->n = n; q->gw = gw; q->gh = gh; q->N = (int64_t)gw * gh;
    q->tx = (gw + MC_T - 1) / MC_T; q->ty = (gh + MC_T - 1) / MC_T;
    if ((int64_t)n * q->tx * q->ty > 0x7fffffffLL) return bad(fn, "too many tiles for one launch");
    return MVS_OK;
}
int headroom(const char* fn, int64_t amax, int64_t cmax, int64_t cmin) {
    if (cmin < 0) return bad(fn, "a capacity is negative");
    if (amax + 8 * cmax > 0x7fffffffLL) return bad(fn, "|excess| + 8 * capacity exceeds int32: a node's excess could overflow");
    return MVS_OK;
}

// The working state of a cut and its rounds.  e, rc and h are the caller's blocks: n*N, 8*n*N and n*N int32.
struct McRun {
    McDims q;
    int32_t *e, *rc, *h;
    hipStream_t s;
    Scratch dctr;
    unsigned nodes_blk() const { return (unsigned)(((int64_t)q.n * q.N + MC_TPB - 1) / MC_TPB); }
    unsigned tiles() const { return (unsigned)(q.n * q.tx * q.ty); }

    // rounds until a converged relabelling leaves no active node; h then holds the exact distances
    int solve(const char* fn, int max_rounds, int32_t* rounds) {
        int rc_;
        if (!dctr.p && (rc_ = dctr.alloc(sizeof(int32_t) * MC_CTR, s))) return rc_;      // once per run: grabcut_dev solves `iters` times
        int32_t hc[MC_CTR];
        bool seed = true, push = false;
        for (int round = 1; round <= max_rounds; ++round) {
            HIPCHK(hipMemsetAsync(dctr.p, 0, sizeof(int32_t) * MC_CTR, s));
            if (push)
                for (int j = 0; j < MC_PUSH_BATCH; ++j) k_mc_push<<<dim3(tiles()), dim3(MC_TPB), 0, s>>>(q, e, rc, h);
            if (seed || push) k_mc_seed<<<dim3(nodes_blk()), dim3(MC_TPB), 0, s>>>((int64_t)q.n * q.N, e, h);
            for (int j = 0; j < MC_RELAX_BATCH; ++j)
                k_mc_relax<<<dim3(tiles()), dim3(MC_TPB), 0, s>>>(q, e, rc, h, j == MC_RELAX_BATCH - 1 ? dctr.as<int32_t>() : nullptr);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hc, dctr.p, sizeof(hc), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            seed = false;
            const int32_t changed = hc[0], active = hc[1];
            push = changed == 0;                                      // a fixed point: the heights are exact
            if (push && active == 0) { if (rounds) *rounds = round; return MVS_OK; }
        }
        if (rounds) *rounds = max_rounds;
        mvs_set_error("%s: the cut was not finished after max_rounds = %d rounds", fn, max_rounds);
        return MVS_E_SOLVER;
    }
};

int mincut_dev(const char* fn, const McDims& q, const int32_t* excess, const int32_t* cap, int32_t max_rounds, uint8_t* side, int32_t* rounds,
               hipStream_t s) {
    int rc;
    const size_t total = (size_t)q.n * (size_t)q.N;
    Scratch de, dc, dh, dstat;
    if ((rc = de.alloc(sizeof(int32_t) * total, s)) || (rc = dc.alloc(sizeof(int32_t) * 8 * total, s)) || (rc = dh.alloc(sizeof(int32_t) * total, s)) ||
        (rc = dstat.alloc(sizeof(int32_t) * 4, s))) return rc;
    McRun run{q, de.as<int32_t>(), dc.as<int32_t>(), dh.as<int32_t>(), s, {}};
    HIPCHK(hipMemsetAsync(dstat.p, 0, sizeof(int32_t) * 4, s));
    k_mc_init<<<dim3(run.nodes_blk()), dim3(MC_TPB), 0, s>>>(q, excess, cap, run.e, run.rc, dstat.as<int32_t>());
    HIPCHK(hipGetLastError());
    int32_t st[4];
    HIPCHK(hipMemcpyAsync(st, dstat.p, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = headroom(fn, st[0], st[1], st[2]))) return rc;
    if ((rc = run.solve(fn, max_rounds, rounds))) return rc;
    k_mc_side<<<dim3(run.nodes_blk()), dim3(MC_TPB), 0, s>>>((int64_t)total, run.h, side);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// ------------------------------------------------------------------ the segmentation ----
constexpr int GC_TPB = 256;
constexpr int GC_SLOTS = 2 * GC_K * GC_SUMS;                         // sums of a frame: [model][component][GC_SUMS], model 0 = foreground

struct GcDims { int32_t n, w, h, hw, hh, bpf; GcRect r; double gamma; };   // bpf: workgroups per frame over the half image

// this thread's half pixel: frame g and index i (i >= hw * hh: none)
__device__ inline void gc_where(const GcDims& q, int* g, int* i) { *g = blockIdx.x / q.bpf; *i = (blockIdx.x % q.bpf) * GC_TPB + threadIdx.x; }

__global__ __launch_bounds__(GC_TPB) void k_gc_half(GcDims q, const uint8_t* __restrict__ imgs, uint32_t* __restrict__ half) {
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (i >= N) return;
    half[(int64_t)g * N + i] = gc_half_px(imgs + (int64_t)g * q.w * q.h * 3, q.w, i % q.hw, i / q.hw);
}

// rules 3, 4 (histograms) and 7 (S)
__global__ __launch_bounds__(GC_TPB) void k_gc_start(GcDims q, const uint32_t* __restrict__ half, uint8_t* __restrict__ fg, int32_t* __restrict__ hist,
                                                     unsigned long long* __restrict__ S) {
    __shared__ int s_hist[2 * GC_LUMA];
    __shared__ int s_part[GC_TPB / 64];
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    for (int k = threadIdx.x; k < 2 * GC_LUMA; k += GC_TPB) s_hist[k] = 0;
    __syncthreads();
    int sum = 0;                                                     // at most 4 * 3 * 255^2 per pixel: a workgroup's sum fits an int
    if (i < N) {
        const int x = i % q.hw, y = i / q.hw;
        const uint32_t* f = half + (int64_t)g * N;
        const uint32_t p = f[i];
        if (x > 0) sum += gc_d2(p, f[i - 1]);
        if (x > 0 && y > 0) sum += gc_d2(p, f[i - q.hw - 1]);
        if (y > 0) sum += gc_d2(p, f[i - q.hw]);
        if (x + 1 < q.hw && y > 0) sum += gc_d2(p, f[i - q.hw + 1]);
        const bool in = gc_inside(q.r, x, y);
        fg[(int64_t)g * N + i] = in ? 1 : 0;
        atomicAdd(&s_hist[(in ? 0 : 1) * GC_LUMA + gc_luma(p)], 1);
    }
    sum = wave_sum_i(sum);
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {                                          // one 64-bit atomic per workgroup
        int tot = 0;
        for (int k = 0; k < GC_TPB / 64; ++k) tot += s_part[k];
        if (tot) atomicAdd(&S[g], (unsigned long long)tot);
    }
    for (int k = threadIdx.x; k < 2 * GC_LUMA; k += GC_TPB)
        if (s_hist[k]) atomicAdd(&hist[(int64_t)g * 2 * GC_LUMA + k], s_hist[k]);
}

// rule 4's thresholds, a wave per (frame, model): a lane owns GC_THR_BINS consecutive bins, a wave scan gives the count in front of
// them, and the one bin where the cumulative count first reaches a target writes that threshold (gc_thresholds, bin for bin)
constexpr int GC_THR_BINS = (GC_LUMA + 63) / 64;
__global__ __launch_bounds__(64) void k_gc_thresholds(const int32_t* __restrict__ hist, int32_t* __restrict__ thr) {
    const int32_t* hs = hist + (int64_t)blockIdx.x * GC_LUMA;       // (frame, model)
    const int lane = threadIdx.x, l0 = lane * GC_THR_BINS;
    int c[GC_THR_BINS], mine = 0;
#pragma unroll
    for (int j = 0; j < GC_THR_BINS; ++j) { c[j] = l0 + j < GC_LUMA ? hs[l0 + j] : 0; mine += c[j]; }
    int incl = mine;                                                 // inclusive scan over the lanes; w * h <= 2^26 fits an int
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    const int64_t m = __shfl(incl, 63, 64);
    int before = incl - mine;
#pragma unroll
    for (int j = 0; j < GC_THR_BINS; ++j) {
        const int after = before + c[j], l = l0 + j;
        if (l < GC_LUMA)
            for (int k = 1; k <= 4; ++k) {
                const int64_t target = (k * m + 4) / 5;
                if (after >= target && (l == 0 || before < target)) thr[4 * blockIdx.x + k - 1] = l;
            }
        before = after;
    }
}

__global__ __launch_bounds__(GC_TPB) void k_gc_label0(GcDims q, const uint32_t* __restrict__ half, const uint8_t* __restrict__ fg,
                                                      const int32_t* __restrict__ thr, uint8_t* __restrict__ label) {
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (i >= N) return;
    const int64_t at = (int64_t)g * N + i;
    label[at] = (uint8_t)gc_luma_component(gc_luma(half[at]), thr + 4 * (2 * g + (fg[at] ? 0 : 1)));
}

__global__ __launch_bounds__(GC_TPB) void k_gc_ncap(GcDims q, const uint32_t* __restrict__ half, const unsigned long long* __restrict__ S,
                                                    int32_t* __restrict__ ncap) {
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (i >= N) return;
    const double beta = gc_beta((int64_t)S[g], q.hw, q.hh);
    const uint32_t* f = half + (int64_t)g * N;
    const int x = i % q.hw, y = i / q.hw;
    const uint32_t p = f[i];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int nx = x + mc_dx(d), ny = y + mc_dy(d);
        int32_t c = 0;
        if (nx >= 0 && nx < q.hw && ny >= 0 && ny < q.hh) c = gc_ncap(beta, q.gamma, gc_d2(p, f[ny * q.hw + nx]), (d & 1) != 0);
        ncap[((int64_t)g * 8 + d) * N + i] = c;
    }
}

__global__ __launch_bounds__(GC_TPB) void k_gc_assign(GcDims q, const uint32_t* __restrict__ half, const uint8_t* __restrict__ fg,
                                                      const GcComp* __restrict__ comps, uint8_t* __restrict__ label) {
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (i >= N) return;
    const int64_t at = (int64_t)g * N + i;
    label[at] = (uint8_t)gc_assign(comps + (2 * g + (fg[at] ? 0 : 1)) * GC_K, half[at]);
}

__global__ __launch_bounds__(GC_TPB) void k_gc_learn(GcDims q, const uint32_t* __restrict__ half, const uint8_t* __restrict__ fg,
                                                     const uint8_t* __restrict__ label, unsigned long long* __restrict__ sums) {
    __shared__ unsigned s_sum[GC_SLOTS];                             // 256 pixels: a product sum stays below 2^25
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (threadIdx.x < GC_SLOTS) s_sum[threadIdx.x] = 0;
    __syncthreads();
    if (i < N) {
        const int64_t at = (int64_t)g * N + i;
        const uint32_t p = half[at];
        const unsigned c0 = gc_ch(p, 0), c1 = gc_ch(p, 1), c2 = gc_ch(p, 2);
        unsigned* s = s_sum + ((fg[at] ? 0 : 1) * GC_K + label[at]) * GC_SUMS;
        atomicAdd(s + 0, 1u); atomicAdd(s + 1, c0); atomicAdd(s + 2, c1); atomicAdd(s + 3, c2);
        atomicAdd(s + 4, c0 * c0); atomicAdd(s + 5, c0 * c1); atomicAdd(s + 6, c0 * c2);
        atomicAdd(s + 7, c1 * c1); atomicAdd(s + 8, c1 * c2); atomicAdd(s + 9, c2 * c2);
    }
    __syncthreads();
    if (threadIdx.x < GC_SLOTS && s_sum[threadIdx.x]) atomicAdd(&sums[(int64_t)g * GC_SLOTS + threadIdx.x], (unsigned long long)s_sum[threadIdx.x]);
}

__global__ void k_gc_fit(int ncomp, const unsigned long long* __restrict__ sums, GcComp* __restrict__ comps) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;             // (frame, model, component)
    if (k >= ncomp) return;
    const int64_t* model = (const int64_t*)sums + (int64_t)(k / GC_K) * GC_K * GC_SUMS;
    int64_t m = 0;
    for (int j = 0; j < GC_K; ++j) m += model[j * GC_SUMS];
    gc_fit(model + (k % GC_K) * GC_SUMS, m, comps + k);
}

__global__ __launch_bounds__(GC_TPB) void k_gc_excess(GcDims q, const uint32_t* __restrict__ half, const GcComp* __restrict__ comps,
                                                      int32_t* __restrict__ e) {
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (i >= N) return;
    const int64_t at = (int64_t)g * N + i;
    const GcComp* m = comps + (int64_t)2 * g * GC_K;
    e[at] = gc_excess(m, m + GC_K, half[at], q.gamma, gc_inside(q.r, i % q.hw, i / q.hw));
}

__global__ __launch_bounds__(GC_TPB) void k_gc_update(GcDims q, const int32_t* __restrict__ h, uint8_t* __restrict__ fg) {
    int g, i;
    gc_where(q, &g, &i);
    const int N = q.hw * q.hh;
    if (i >= N) return;
    const int64_t at = (int64_t)g * N + i;
    fg[at] = (gc_inside(q.r, i % q.hw, i / q.hw) && h[at] == MC_HINF) ? 1 : 0;
}

__global__ __launch_bounds__(GC_TPB) void k_gc_full(GcDims q, const uint8_t* __restrict__ fg, uint8_t* __restrict__ mask) {
    const int64_t npx = (int64_t)q.w * q.h, at = (int64_t)blockIdx.x * GC_TPB + threadIdx.x;
    if (at >= (int64_t)q.n * npx) return;
    const int g = (int)(at / npx), i = (int)(at % npx);
    mask[at] = gc_full_px(fg + (int64_t)g * q.hw * q.hh, q.hw, q.hh, i % q.w, i / q.w);
}

int check_gc(const char* fn, int32_t n, int32_t w, int32_t h, const void* imgs, const mvs_grabcut_params* p, const void* mask, GcDims* q) {
    if (!imgs || !p || !mask) return bad(fn, "imgs, params or mask is NULL");
    if (n < 1) return bad(fn, "need n >= 1");
    if (w < 2 || h < 2) return bad(fn, "need w, h >= 2");
    if ((int64_t)w * h > (1LL << 26)) return bad(fn, "w * h must not exceed 2^26");
    if ((int64_t)n * w * h > 0x7fffffffLL) return bad(fn, "n * w * h must not exceed 2^31 - 1");
    for (double m : {p->hl, p->hr, p->vl, p->vr})
        if (!(m >= 0.0 && m <= 1.0)) return bad(fn, "a margin ratio is outside [0, 1]");
    if (p->iters < 1) return bad(fn, "need iters >= 1");
    if (!std::isfinite(p->gamma) || p->gamma <= 0.0 || p->gamma > 100000.0) return bad(fn, "need 0 < gamma <= 100000");
    if (p->max_rounds < 1) return bad(fn, "need max_rounds >= 1");
    q->n = n; q->w = w; q->h = h; q->hw = w / 2; q->hh = h / 2;
    q->bpf = (q->hw * q->hh + GC_TPB - 1) / GC_TPB;
    q->gamma = p->gamma;
    q->r = gc_rect(q->hw, q->hh, p->hl, p->hr, p->vl, p->vr);
    if (q->r.x0 >= q->r.x1 || q->r.y0 >= q->r.y1) return bad(fn, "the rectangle is empty");
    return MVS_OK;
}

// where mvs_test_grabcut_trace wants the steps (host arrays, each may be NULL)
struct GcTrace {
    uint8_t* labels; int64_t* sums; int32_t* excess; int32_t* ncap; uint8_t* half_mask; int64_t* S; int32_t* rounds;
};

template <class T> int gc_down(T* host, const void* dev, size_t n, hipStream_t s) {
    if (!host) return MVS_OK;
    HIPCHK(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

int grabcut_dev(const char* fn, const GcDims& q, const uint8_t* imgs, const mvs_grabcut_params* p, uint8_t* mask, uint8_t* half_mask, hipStream_t s,
                const GcTrace* tr) {
    int rc;
    const size_t N = (size_t)q.hw * q.hh, total = (size_t)q.n * N;
    const unsigned blk = (unsigned)(q.n * q.bpf), ncomp = (unsigned)(q.n * 2 * GC_K);
    Scratch dhalf, dfg, dlab, dhist, dthr, dsum, dcomp, dS, dncap, de, drc, dh;
    if ((rc = dhalf.alloc(4 * total, s)) || (rc = dfg.alloc(total, s)) || (rc = dlab.alloc(total, s)) ||
        (rc = dhist.alloc(sizeof(int32_t) * 2 * GC_LUMA * q.n, s)) || (rc = dthr.alloc(sizeof(int32_t) * 8 * q.n, s)) ||
        (rc = dsum.alloc(sizeof(int64_t) * GC_SLOTS * q.n, s)) || (rc = dcomp.alloc(sizeof(GcComp) * ncomp, s)) ||
        (rc = dS.alloc(sizeof(int64_t) * q.n, s)) || (rc = dncap.alloc(sizeof(int32_t) * 8 * total, s)) || (rc = de.alloc(sizeof(int32_t) * total, s)) ||
        (rc = drc.alloc(sizeof(int32_t) * 8 * total, s)) || (rc = dh.alloc(sizeof(int32_t) * total, s))) return rc;
    McDims mq;
    mq.n = q.n; mq.gw = q.hw; mq.gh = q.hh; mq.N = (int64_t)N;
    mq.tx = (q.hw + MC_T - 1) / MC_T; mq.ty = (q.hh + MC_T - 1) / MC_T;
    McRun run{mq, de.as<int32_t>(), drc.as<int32_t>(), dh.as<int32_t>(), s, {}};
    uint32_t* half = dhalf.as<uint32_t>();
    uint8_t *fg = dfg.as<uint8_t>(), *lab = dlab.as<uint8_t>();
    unsigned long long* sums = dsum.as<unsigned long long>();

    HIPCHK(hipMemsetAsync(dhist.p, 0, sizeof(int32_t) * 2 * GC_LUMA * q.n, s));
    HIPCHK(hipMemsetAsync(dS.p, 0, sizeof(int64_t) * q.n, s));
    k_gc_half<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, imgs, half);
    k_gc_start<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, half, fg, dhist.as<int32_t>(), dS.as<unsigned long long>());
    k_gc_thresholds<<<dim3(2 * q.n), dim3(64), 0, s>>>(dhist.as<int32_t>(), dthr.as<int32_t>());
    k_gc_label0<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, half, fg, dthr.as<int32_t>(), lab);
    k_gc_ncap<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, half, dS.as<unsigned long long>(), dncap.as<int32_t>());
    HIPCHK(hipGetLastError());
    if (tr && ((rc = gc_down(tr->S, dS.p, (size_t)q.n, s)) || (rc = gc_down(tr->ncap, dncap.p, 8 * total, s)))) return rc;
    for (int it = 0; it <= p->iters; ++it) {                         // it == 0: the learn of rule 11 on the components of rule 4
        if (it > 0) k_gc_assign<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, half, fg, dcomp.as<GcComp>(), lab);
        HIPCHK(hipMemsetAsync(dsum.p, 0, sizeof(int64_t) * GC_SLOTS * q.n, s));
        k_gc_learn<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, half, fg, lab, sums);
        k_gc_fit<<<dim3((ncomp + 63) / 64), dim3(64), 0, s>>>((int)ncomp, sums, dcomp.as<GcComp>());
        HIPCHK(hipGetLastError());
        if (tr && ((rc = gc_down(tr->labels ? tr->labels + (size_t)it * total : nullptr, lab, total, s)) ||
                   (rc = gc_down(tr->sums ? tr->sums + (size_t)it * GC_SLOTS * q.n : nullptr, sums, (size_t)GC_SLOTS * q.n, s)))) return rc;
        if (it == 0) continue;
        k_gc_excess<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, half, dcomp.as<GcComp>(), run.e);
        HIPCHK(hipMemcpyAsync(run.rc, dncap.p, sizeof(int32_t) * 8 * total, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipGetLastError());
        if (tr && (rc = gc_down(tr->excess ? tr->excess + (size_t)(it - 1) * total : nullptr, run.e, total, s))) return rc;
        int32_t rounds = 0;
        rc = run.solve(fn, p->max_rounds, &rounds);
        if (tr && tr->rounds) tr->rounds[it - 1] = rounds;
        if (rc) return rc;
        k_gc_update<<<dim3(blk), dim3(GC_TPB), 0, s>>>(q, run.h, fg);
        HIPCHK(hipGetLastError());
        if (tr && (rc = gc_down(tr->half_mask ? tr->half_mask + (size_t)(it - 1) * total : nullptr, fg, total, s))) return rc;
    }
    k_gc_full<<<dim3((unsigned)(((int64_t)q.n * q.w * q.h + GC_TPB - 1) / GC_TPB)), dim3(GC_TPB), 0, s>>>(q, fg, mask);
    HIPCHK(hipGetLastError());
    if (half_mask) HIPCHK(hipMemcpyAsync(half_mask, fg, total, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// the host form: images up, masks down
int grabcut_host(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const mvs_grabcut_params* p, uint8_t* mask, uint8_t* half_mask,
                 const GcTrace* tr) {
    GcDims q;
    int rc = check_gc(fn, n, w, h, imgs, p, mask, &q);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    const size_t npx = (size_t)n * w * h, nh = (size_t)n * q.hw * q.hh;
    Scratch di, dm, dhm;
    if ((rc = up(di, imgs, 3 * npx)) || (rc = dm.alloc(npx)) || (half_mask && (rc = dhm.alloc(nh)))) return rc;
    if ((rc = grabcut_dev(fn, q, di.as<uint8_t>(), p, dm.as<uint8_t>(), half_mask ? dhm.as<uint8_t>() : nullptr, nullptr, tr))) return rc;
    if ((rc = down(mask, dm, npx))) return rc;
    return half_mask ? down(half_mask, dhm, nh) : MVS_OK;
}

}  // namespace

extern "C" {

int mvs_grid_mincut_dev(int32_t n, int32_t gw, int32_t gh, const int32_t* excess_dev, const int32_t* cap_dev, int32_t max_rounds,
                        uint8_t* source_side_dev, int32_t* rounds, void* hip_stream) {
    MVS_TRACE();
    McDims q;
    int rc = check_mc(__func__, n, gw, gh, excess_dev, cap_dev, max_rounds, source_side_dev, &q);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return mincut_dev(__func__, q, excess_dev, cap_dev, max_rounds, source_side_dev, rounds, (hipStream_t)hip_stream);
}

int mvs_grid_mincut(int32_t n, int32_t gw, int32_t gh, const int32_t* excess, const int32_t* cap, int32_t max_rounds, uint8_t* source_side,
                    int32_t* rounds) {
    MVS_TRACE();
    McDims q;
    int rc = check_mc(__func__, n, gw, gh, excess, cap, max_rounds, source_side, &q);
    if (rc) return rc;
    int64_t amax = 0, cmax = 0, cmin = 0;
    for (int64_t g = 0; g < n; ++g)
        for (int64_t i = 0; i < q.N; ++i) {
            const int64_t a = excess[g * q.N + i];
            amax = std::max(amax, a < 0 ? -a : a);
            const int x = (int)(i % gw), y = (int)(i / gw);
            for (int d = 0; d < 8; ++d) {
                const int nx = x + mc_dx(d), ny = y + mc_dy(d);
                if (nx < 0 || nx >= gw || ny < 0 || ny >= gh) continue;
                const int64_t c = cap[(g * 8 + d) * q.N + i];
                cmax = std::max(cmax, c);
                cmin = std::min(cmin, c);
            }
        }
    if ((rc = headroom(__func__, amax, cmax, cmin))) return rc;
    if ((rc = need_device())) return rc;
    const size_t total = (size_t)n * (size_t)q.N;
    Scratch de, dc, ds;
    if ((rc = up(de, excess, total)) || (rc = up(dc, cap, 8 * total)) || (rc = ds.alloc(total))) return rc;
    if ((rc = mincut_dev(__func__, q, de.as<int32_t>(), dc.as<int32_t>(), max_rounds, ds.as<uint8_t>(), rounds, nullptr))) return rc;
    return down(source_side, ds, total);
}

void mvs_grabcut_default_params(mvs_grabcut_params* p) {
    if (!p) return;
    p->hl = p->hr = p->vl = p->vr = 0.1;
    p->gamma = 50.0; p->iters = 3; p->max_rounds = 4096; p->reserved = 0;
}

int mvs_grabcut_masks_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, const mvs_grabcut_params* p, uint8_t* mask_dev,
                          uint8_t* half_mask_dev, void* hip_stream) {
    MVS_TRACE();
    GcDims q;
    int rc = check_gc(__func__, n, w, h, imgs_dev, p, mask_dev, &q);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return grabcut_dev(__func__, q, imgs_dev, p, mask_dev, half_mask_dev, (hipStream_t)hip_stream, nullptr);
}

int mvs_grabcut_masks(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const mvs_grabcut_params* p, uint8_t* mask, uint8_t* half_mask) {
    MVS_TRACE();
    return grabcut_host(__func__, n, w, h, imgs, p, mask, half_mask, nullptr);
}

int mvs_test_grabcut_trace(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const mvs_grabcut_params* p, uint8_t* mask, int64_t* S,
                           int32_t* ncap, uint8_t* labels, int64_t* sums, int32_t* excess, uint8_t* half_mask, int32_t* rounds) {
    MVS_TRACE();
    const GcTrace tr{labels, sums, excess, ncap, half_mask, S, rounds};
    return grabcut_host(__func__, n, w, h, imgs, p, mask, nullptr, &tr);
}

}  // extern "C"

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device)
const void* mvs_tu_probe_grabcut() { return (const void*)k_mc_relax; }
