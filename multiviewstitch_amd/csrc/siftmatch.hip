// siftmatch.hip — FeatureProc::MatchFeature (R/FeatureProc/FeatureProc.cpp:77-130, call site R/Processor/Processor.cpp:634): the
// SiftMatchGPU descriptor matcher for ALL list pairs of two adjacent sequences at once.  The rules are those of include/mvs.h
// (mvs_sift_match_lists; recalled from SiftMatchGPU, not verified against its source).
//
//   k_sm_quantise : 128 floats -> 128 bytes per descriptor, 16-byte stores.  The i8 MFMA operands are signed and q runs to 255: the
//                   byte stored is q - 128 and the descriptor's sum of q goes next to it, so that
//                   sum_c a b = sum_c (a - 128)(b - 128) + 128 (sum a + sum b) - 2097152, all in int32, exact
//   k_sm_direction: one launch for every list pair in BOTH directions (the same body, the roles swapped).  A workgroup = 128 query
//                   descriptors of one list against every descriptor of the other list; a wave keeps the A fragments of its 32 query
//                   rows for the whole K = 128 in registers (two 16x16x64 k-steps), the waves share 64-descriptor tiles of the other
//                   list, staged through LDS (double-buffered, rows padded to 144 bytes).  The scores never leave the registers: each
//                   lane keeps (best, bestidx, second) per accumulator row (C/D map: col = lane & 15, row = (lane >> 4) * 4 + reg), the
//                   16 column lanes merge at the end under the total order (score descending, index ascending), and the thresholds
//                   are applied there: m(i) = bestidx or -1.  Integer scores: nothing depends on scheduling, no atomics.
//                   A and B fragments are both "16 bytes at 64 * kstep + 16 * (lane >> 4) of row lane & 15": whatever order the
//                   instruction gives the 64 k of a step, both operands meet it with the same bytes, and a dot product does not care.
//   k_sm_pair / CompactTail / k_sm_rows : the mutual-best rule per list pair and an order-preserving compaction (compact.hip, the
//                   scheme of views.hip's cull).  List pairs are numbered p = ((f1 * n2 + f2) * view_count + v1) * view_count + v2, so
//                   the compacted rows ARE the buckets of rule 7 back to back: bucket k owns pairs [k * view_count^2, (k+1) * view_count^2).
//
// The number of launches does not depend on the number of list pairs.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include "../../include/mvs_test.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int SM_TPB = 256;
constexpr int SM_WAVES = SM_TPB / 64;
static_assert(SM_TPB == COMPACT_TPB, "k_sm_pair and k_sm_rows count and place per workgroup of the shared tail");
constexpr int SM_ROWS_WAVE = 32;                          // query rows of a wave: two 16-row MFMA tiles
constexpr int SM_ROWS = SM_WAVES * SM_ROWS_WAVE;          // ... of a workgroup
constexpr int SM_TILE = 64;                               // descriptors of the other list per LDS stage
constexpr int SM_STRIDE = 144;                            // bytes per staged row: 128 + 16, off the 128-byte bank stride
constexpr int32_t SM_NO_COLUMN = (int32_t)0x80000000;     // column term of a staged row behind the list's end
constexpr int64_t SM_MAX_LIST_PAIRS = 1LL << 30;

typedef int v4i __attribute__((ext_vector_type(4)));

// rule 1: q = (int)(512 d + 0.5) in float32; d <= 0 or NaN -> 0; above 255 -> 255 (the deviation mvs.h states)
__device__ inline int sm_quant(float d) {
    if (!(d > 0.0f)) return 0;
    const float t = 512.0f * d + 0.5f;
    return t >= 256.0f ? 255 : (int)t;
}

// 8 threads per descriptor, 16 floats each
__global__ __launch_bounds__(SM_TPB) void k_sm_quantise(const float* __restrict__ descs, int64_t n, uint4* __restrict__ q, int32_t* __restrict__ sum) {
    const int64_t t = (int64_t)blockIdx.x * SM_TPB + threadIdx.x, r = t >> 3;
    const int part = (int)(t & 7);
    int s = 0;
    if (r < n) {
        const float4* src = (const float4*)(descs + 128 * r + 16 * part);
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 f = src[k];
            const int a = sm_quant(f.x), b = sm_quant(f.y), c = sm_quant(f.z), d = sm_quant(f.w);
            s += (a + b) + (c + d);
            w[k] = ((unsigned)(a ^ 0x80)) | ((unsigned)(b ^ 0x80) << 8) | ((unsigned)(c ^ 0x80) << 16) | ((unsigned)(d ^ 0x80) << 24);      // q - 128 as a signed byte
        }
        q[8 * r + part] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    s += __shfl_xor(s, 1, 64);                             // the 8 threads of a descriptor are neighbours in one wave
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (r < n && part == 0) sum[r] = s;
}

// list pair p -> its two lists (the numbering of the file comment)
__host__ __device__ inline void sm_lists_of(int64_t p, int n2, int vc, int* l1, int* l2) {
    const int v2 = (int)(p % vc), v1 = (int)((p / vc) % vc);
    const int64_t k = p / ((int64_t)vc * vc);
    *l1 = (int)(k / n2) * vc + v1;
    *l2 = (int)(k % n2) * vc + v2;
}

struct SmBest { int best, idx, second; };
// the total order: score descending, index ascending; `second` takes the loser's best
__device__ inline SmBest sm_merge(SmBest a, SmBest b) {
    const bool a_wins = a.best > b.best || (a.best == b.best && a.idx < b.idx);
    SmBest r;
    r.best = a_wins ? a.best : b.best;
    r.idx = a_wins ? a.idx : b.idx;
    r.second = max(max(a.second, b.second), a_wins ? b.best : a.best);
    return r;
}

struct SmDev {
    const int8_t *q1, *q2;                 // [total][128] q - 128
    const int32_t *sum1, *sum2;            // [total] sum of q
    const int64_t *off1, *off2;            // [L + 1]
    const int64_t *roff12, *roff21;        // [NP + 1]: where pair p's results of direction 1->2 (2->1) start
    int32_t *m12, *m21;                    // m(i) of every pair and direction, preset to -1
    int32_t *dbg12, *dbg21;                // test hook: [3][T] best, bestidx, second; or NULL
    int64_t T12, T21;
    int n2, vc, max_sift;
    double distmax, ratiomax;
};

__device__ inline void sm_stage_load(const int8_t* __restrict__ O, const int32_t* __restrict__ sumO, int no, int t, int tid, uint4* regs, int32_t* ct) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = tid + SM_TPB * u, j = t * SM_TILE + (c >> 3);
        regs[u] = j < no ? *(const uint4*)(O + (int64_t)j * 128 + 16 * (c & 7)) : make_uint4(0, 0, 0, 0);
    }
    if (tid < SM_TILE) {
        const int j = t * SM_TILE + tid;
        *ct = j < no ? 128 * sumO[j] : SM_NO_COLUMN;
    }
}
__device__ inline void sm_stage_store(int8_t* buf, int32_t* s_ct, int tid, const uint4* regs, int32_t ct) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = tid + SM_TPB * u;
        *(uint4*)(buf + (c >> 3) * SM_STRIDE + 16 * (c & 7)) = regs[u];
    }
    if (tid < SM_TILE) s_ct[tid] = ct;
}

__global__ __launch_bounds__(SM_TPB) void k_sm_direction(const int2* __restrict__ work, SmDev d) {
    __shared__ __attribute__((aligned(16))) int8_t s_tile[2][SM_TILE * SM_STRIDE];
    __shared__ int32_t s_ct[2][SM_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int2 wk = work[blockIdx.x];
    const int64_t p = wk.x;
    const int dir = wk.y & 1, rb = wk.y >> 1;
    int l1, l2;
    sm_lists_of(p, d.n2, d.vc, &l1, &l2);
    const int64_t a0 = d.off1[l1], b0 = d.off2[l2];
    const int na = (int)min((int64_t)d.max_sift, d.off1[l1 + 1] - a0), nb = (int)min((int64_t)d.max_sift, d.off2[l2 + 1] - b0);      // rule 2
    const int8_t* Q = dir ? d.q2 + b0 * 128 : d.q1 + a0 * 128;          // the query list
    const int8_t* O = dir ? d.q1 + a0 * 128 : d.q2 + b0 * 128;          // the other list
    const int32_t* sumQ = dir ? d.sum2 + b0 : d.sum1 + a0;
    const int32_t* sumO = dir ? d.sum1 + a0 : d.sum2 + b0;
    const int nq = dir ? nb : na, no = dir ? na : nb;
    const int64_t res0 = dir ? d.roff21[p] : d.roff12[p];
    const int row0 = rb * SM_ROWS + wv * SM_ROWS_WAVE;
    const bool active = row0 < nq;                                       // (a whole wave: it still stages tiles and meets the barriers)

    v4i a[2][2];
    int rowc[2][4];
    SmBest st[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int row = row0 + 16 * mt + lr;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            a[mt][ks] = row < nq ? *(const v4i*)(Q + (int64_t)row * 128 + 64 * ks + 16 * lg) : (v4i){0, 0, 0, 0};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = row0 + 16 * mt + 4 * lg + reg;
            rowc[mt][reg] = r < nq ? 128 * sumQ[r] - 2097152 : 0;
            st[mt][reg] = SmBest{-1, 0x7fffffff, -1};
        }
    }

    const int nt = (no + SM_TILE - 1) / SM_TILE;                          // the same in every thread of the workgroup
    uint4 regs[2];
    int32_t ct = 0;
    sm_stage_load(O, sumO, no, 0, tid, regs, &ct);
    sm_stage_store(s_tile[0], s_ct[0], tid, regs, ct);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int8_t* buf = s_tile[t & 1];
        const int32_t* cts = s_ct[t & 1];
        if (t + 1 < nt) sm_stage_load(O, sumO, no, t + 1, tid, regs, &ct);
        if (active) {
#pragma unroll
            for (int ns = 0; ns < SM_TILE / 16; ++ns) {
                const int8_t* brow = buf + (16 * ns + lr) * SM_STRIDE + 16 * lg;
                const v4i b0v = *(const v4i*)brow, b1v = *(const v4i*)(brow + 64);
                const int32_t c = cts[16 * ns + lr];
                const int j = t * SM_TILE + 16 * ns + lr;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    v4i acc = {0, 0, 0, 0};
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mt][0], b0v, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mt][1], b1v, acc, 0, 0, 0);
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int s = c == SM_NO_COLUMN ? -1 : acc[reg] + c + rowc[mt][reg];      // rule 3, exact
                        SmBest& q = st[mt][reg];
                        if (s > q.best) { q.second = q.best; q.best = s; q.idx = j; }              // j ascends in a lane: the lowest index keeps a tie
                        else if (s > q.second) q.second = s;
                    }
                }
            }
        }
        if (t + 1 < nt) sm_stage_store(s_tile[(t + 1) & 1], s_ct[(t + 1) & 1], tid, regs, ct);
        __syncthreads();
    }
    if (!active) return;
    // the 16 column lanes of a row (same lane >> 4) merge; afterwards each of them holds the row's result
    SmBest mine = SmBest{-1, 0x7fffffff, -1};
    int my_row = -1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            SmBest q = st[mt][reg];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                SmBest other;
                other.best = __shfl_xor(q.best, o, 64);
                other.idx = __shfl_xor(q.idx, o, 64);
                other.second = __shfl_xor(q.second, o, 64);
                q = sm_merge(q, other);
            }
            if (lr == 4 * mt + reg) { mine = q; my_row = row0 + 16 * mt + 4 * lg + reg; }       // one row per lane for the thresholds
        }
    if (my_row < 0 || my_row >= nq) return;
    const int second = max(mine.second, 0);                              // no other j: 0
    int m = -1;
    if (mine.best > 0) {                                                 // rule 4
        const double dist = acos(fmin((double)mine.best / 262144.0, 1.0)), dist2 = acos(fmin((double)second / 262144.0, 1.0));
        if (dist < d.distmax && dist < d.ratiomax * dist2) m = mine.idx;
    }
    (dir ? d.m21 : d.m12)[res0 + my_row] = m;
    int32_t* dbg = dir ? d.dbg21 : d.dbg12;
    if (dbg) {
        const int64_t T = dir ? d.T21 : d.T12;
        dbg[res0 + my_row] = mine.best;
        dbg[T + res0 + my_row] = mine.idx;
        dbg[2 * T + res0 + my_row] = second;
    }
}

// rule 5 for candidate r of direction 1->2 (query i of pair p): mutual iff m21(m12(i)) == i
__global__ __launch_bounds__(SM_TPB) void k_sm_pair(SmDev d, int64_t npairs, uint8_t* __restrict__ keep, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[SM_WAVES];
    const int64_t r = (int64_t)blockIdx.x * SM_TPB + threadIdx.x;
    bool f = false;
    if (r < d.T12) {
        const int j = d.m12[r];
        if (j >= 0) {
            const int p = segment_of(d.roff12, (int)npairs, r);
            f = (int64_t)d.m21[d.roff21[p] + j] == r - d.roff12[p];
        }
        keep[r] = f ? 1 : 0;
    }
    const WgRank k = wg_rank<SM_WAVES>(f, s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

// rule 6; without keys (mvs_sift_match, the index form) a row is (i, j)
__global__ __launch_bounds__(SM_TPB) void k_sm_rows(SmDev d, int64_t npairs, const uint8_t* __restrict__ keep, const int32_t* __restrict__ base,
                                                    const float* __restrict__ keys1, const float* __restrict__ keys2, int32_t* __restrict__ out) {
    __shared__ int s_wsum[SM_WAVES];
    const int64_t r = (int64_t)blockIdx.x * SM_TPB + threadIdx.x;
    const bool f = r < d.T12 && keep[r];
    const int64_t pos = (int64_t)base[blockIdx.x] + wg_rank<SM_WAVES>(f, s_wsum).rank;
    if (!f) return;
    const int p = segment_of(d.roff12, (int)npairs, r);
    const int i = (int)(r - d.roff12[p]), j = d.m12[r];
    if (!keys1) { out[2 * pos] = i; out[2 * pos + 1] = j; return; }
    int l1, l2;
    sm_lists_of(p, d.n2, d.vc, &l1, &l2);
    const float* k1 = keys1 + 4 * (d.off1[l1] + i);
    const float* k2 = keys2 + 4 * (d.off2[l2] + j);
    int32_t* o = out + 6 * pos;
    o[0] = l1 % d.vc; o[1] = cvt_i32((double)k1[0] + 0.5); o[2] = cvt_i32((double)k1[1] + 0.5);
    o[3] = l2 % d.vc; o[4] = cvt_i32((double)k2[0] + 0.5); o[5] = cvt_i32((double)k2[1] + 0.5);
}

int check_lists(const char* fn, int32_t n1, int32_t n2, const mvs_sift_match_params* p, const int64_t* off1, const void* keys1, const void* descs1,
                const int64_t* off2, const void* keys2, const void* descs2, const int64_t* raw_offsets, int64_t raw_capacity) {
    if (n1 < 1 || n2 < 1 || (int64_t)n1 * n2 > 1000000) return bad(fn, "need n_frames1, n_frames2 >= 1 and n_frames1 * n_frames2 <= 1000000");
    if (!p) return bad(fn, "params is NULL");
    if (p->view_count < 1 || p->max_sift < 1) return bad(fn, "need view_count >= 1 and max_sift >= 1");
    if ((int64_t)n1 * n2 * p->view_count * p->view_count > SM_MAX_LIST_PAIRS) return bad(fn, "more than 2^30 list pairs");
    if (!off1 || !off2 || !raw_offsets) return bad(fn, "key_offsets1 / key_offsets2 / raw_offsets is NULL");
    if (raw_capacity < 0) return bad(fn, "raw_capacity is negative");
    int rc;
    if ((rc = check_offsets(fn, "key_offsets1", off1, (int64_t)n1 * p->view_count, 0x7fffffffLL)) ||
        (rc = check_offsets(fn, "key_offsets2", off2, (int64_t)n2 * p->view_count, 0x7fffffffLL))) return rc;
    if ((off1[(int64_t)n1 * p->view_count] > 0 && (!keys1 || !descs1)) || (off2[(int64_t)n2 * p->view_count] > 0 && (!keys2 || !descs2)))
        return bad(fn, "keys or descs is NULL");
    return MVS_OK;
}

struct SmHook { int32_t *best12, *idx12, *second12, *best21, *idx21, *second21; };

// Keys (NULL: index rows) and descriptors in HBM; offsets and outputs on the host.  pair_off receives the NP + 1 offsets of the list
// pairs in their own numbering; rows (when wanted) the compacted rows.  Returns with s synchronised.
int sm_core(int n1, int n2, const mvs_sift_match_params* prm, const int64_t* off1, const float* keys1, const float* descs1, const int64_t* off2,
            const float* keys2, const float* descs2, std::vector<int64_t>& pair_off, bool want_rows, int64_t row_capacity, int32_t* rows,
            const SmHook* hook, hipStream_t s) {
    const int vc = prm->view_count, L1 = n1 * vc, L2 = n2 * vc;
    const int64_t NP = (int64_t)L1 * L2, tot1 = off1[L1], tot2 = off2[L2];
    const int width = keys1 ? 6 : 2;
    pair_off.assign((size_t)NP + 1, 0);
    std::vector<int64_t> roff12((size_t)NP + 1, 0), roff21((size_t)NP + 1, 0);
    std::vector<int2> work;
    for (int64_t p = 0; p < NP; ++p) {
        int l1, l2;
        sm_lists_of(p, n2, vc, &l1, &l2);
        const int64_t c1 = std::min<int64_t>(prm->max_sift, off1[l1 + 1] - off1[l1]), c2 = std::min<int64_t>(prm->max_sift, off2[l2 + 1] - off2[l2]);
        roff12[(size_t)p + 1] = roff12[(size_t)p] + c1;
        roff21[(size_t)p + 1] = roff21[(size_t)p] + c2;
        if (c1 == 0 || c2 == 0) continue;                                // an empty list contributes no workgroup
        for (int b = 0; b < (c1 + SM_ROWS - 1) / SM_ROWS; ++b) work.push_back(make_int2((int)p, b << 1));
        for (int b = 0; b < (c2 + SM_ROWS - 1) / SM_ROWS; ++b) work.push_back(make_int2((int)p, (b << 1) | 1));
    }
    const int64_t T12 = roff12[(size_t)NP], T21 = roff21[(size_t)NP];
    if (T12 >= 0x7fffffffLL || T21 >= 0x7fffffffLL || work.size() >= 0x7fffffffULL) {
        mvs_set_error("sift match: more than 2^31 - 1 candidate matches or workgroups in one call");
        return MVS_E_INVALID_ARG;
    }
    if (work.empty()) return MVS_OK;                                     // nothing can match
    Scratch q1, q2, s1, s2, doff1, doff2, dr12, dr21, dwork, m12, m21, dbg12, dbg21, keep, drows;
    CompactTail ct;
    const int nb = (int)((T12 + SM_TPB - 1) / SM_TPB);
    int rc;
    if ((rc = q1.alloc(128 * (size_t)tot1, s)) || (rc = q2.alloc(128 * (size_t)tot2, s)) || (rc = s1.alloc(sizeof(int32_t) * (size_t)tot1, s)) ||
        (rc = s2.alloc(sizeof(int32_t) * (size_t)tot2, s)) || (rc = up_async(doff1, off1, (size_t)L1 + 1, s)) || (rc = up_async(doff2, off2, (size_t)L2 + 1, s)) ||
        (rc = up_async(dr12, roff12.data(), roff12.size(), s)) || (rc = up_async(dr21, roff21.data(), roff21.size(), s)) ||
        (rc = up_async(dwork, work.data(), work.size(), s)) || (rc = m12.alloc(sizeof(int32_t) * (size_t)T12, s)) ||
        (rc = m21.alloc(sizeof(int32_t) * (size_t)T21, s)) || (rc = keep.alloc((size_t)T12, s)) || (rc = ct.alloc((size_t)nb, (size_t)NP, s)) ||
        (hook && ((rc = dbg12.alloc(sizeof(int32_t) * 3 * (size_t)T12, s)) || (rc = dbg21.alloc(sizeof(int32_t) * 3 * (size_t)T21, s))))) return rc;
    HIPCHK(hipMemsetAsync(m12.p, 0xff, sizeof(int32_t) * (size_t)T12, s));                    // -1: a query nobody ran (the other list is empty)
    HIPCHK(hipMemsetAsync(m21.p, 0xff, sizeof(int32_t) * (size_t)T21, s));
    if (hook) {
        HIPCHK(hipMemsetAsync(dbg12.p, 0, sizeof(int32_t) * 3 * (size_t)T12, s));
        HIPCHK(hipMemsetAsync(dbg21.p, 0, sizeof(int32_t) * 3 * (size_t)T21, s));
    }
    k_sm_quantise<<<dim3((unsigned)((8 * tot1 + SM_TPB - 1) / SM_TPB)), dim3(SM_TPB), 0, s>>>(descs1, tot1, q1.as<uint4>(), s1.as<int32_t>());
    k_sm_quantise<<<dim3((unsigned)((8 * tot2 + SM_TPB - 1) / SM_TPB)), dim3(SM_TPB), 0, s>>>(descs2, tot2, q2.as<uint4>(), s2.as<int32_t>());
    SmDev d;
    d.q1 = q1.as<int8_t>(); d.q2 = q2.as<int8_t>(); d.sum1 = s1.as<int32_t>(); d.sum2 = s2.as<int32_t>();
    d.off1 = doff1.as<int64_t>(); d.off2 = doff2.as<int64_t>(); d.roff12 = dr12.as<int64_t>(); d.roff21 = dr21.as<int64_t>();
    d.m12 = m12.as<int32_t>(); d.m21 = m21.as<int32_t>(); d.dbg12 = hook ? dbg12.as<int32_t>() : nullptr; d.dbg21 = hook ? dbg21.as<int32_t>() : nullptr;
    d.T12 = T12; d.T21 = T21; d.n2 = n2; d.vc = vc; d.max_sift = prm->max_sift; d.distmax = prm->distmax; d.ratiomax = prm->ratiomax;
    k_sm_direction<<<dim3((unsigned)work.size()), dim3(SM_TPB), 0, s>>>(dwork.as<int2>(), d);
    k_sm_pair<<<dim3((unsigned)nb), dim3(SM_TPB), 0, s>>>(d, NP, keep.as<uint8_t>(), ct.cnt.as<int32_t>());
    ct.segments(nb, d.roff12, NP, T12, keep.as<uint8_t>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pair_off.data(), ct.off.p, sizeof(int64_t) * ((size_t)NP + 1), hipMemcpyDeviceToHost, s));
    if (hook) {
        int32_t* h12[3] = {hook->best12, hook->idx12, hook->second12};
        int32_t* h21[3] = {hook->best21, hook->idx21, hook->second21};
        for (int k = 0; k < 3; ++k) {
            HIPCHK(hipMemcpyAsync(h12[k], dbg12.as<int32_t>() + k * T12, sizeof(int32_t) * (size_t)T12, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(h21[k], dbg21.as<int32_t>() + k * T21, sizeof(int32_t) * (size_t)T21, hipMemcpyDeviceToHost, s));
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    const int64_t total = pair_off[(size_t)NP];
    if (!want_rows || total == 0 || total > row_capacity) return MVS_OK;      // (the caller reports a capacity that is too small)
    if ((rc = drows.alloc(sizeof(int32_t) * width * (size_t)total, s))) return rc;
    k_sm_rows<<<dim3((unsigned)nb), dim3(SM_TPB), 0, s>>>(d, NP, keep.as<uint8_t>(), ct.base.as<int32_t>(), keys1, keys2, drows.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rows, drows.p, sizeof(int32_t) * width * (size_t)total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// the list form behind both public entries: buckets and pair counts from the list pairs' offsets
int lists_core(const char* fn, int n1, int n2, const mvs_sift_match_params* p, const int64_t* off1, const float* keys1, const float* descs1,
               const int64_t* off2, const float* keys2, const float* descs2, int64_t* raw_offsets, int32_t* raw, int64_t raw_capacity,
               int64_t* pair_counts, hipStream_t s) {
    std::vector<int64_t> po;
    int rc = sm_core(n1, n2, p, off1, keys1, descs1, off2, keys2, descs2, po, raw != nullptr, raw_capacity, raw, nullptr, s);
    if (rc) return rc;
    const int vc = p->view_count, L2 = n2 * vc;
    const int64_t v2 = (int64_t)vc * vc, nk = (int64_t)n1 * n2;
    for (int64_t k = 0; k <= nk; ++k) raw_offsets[k] = po[(size_t)(k * v2)];
    if (pair_counts)
        for (int64_t q = 0; q < nk * v2; ++q) {
            int l1, l2;
            sm_lists_of(q, n2, vc, &l1, &l2);
            pair_counts[(int64_t)l1 * L2 + l2] = po[(size_t)q + 1] - po[(size_t)q];
        }
    if (raw && raw_capacity < raw_offsets[nk]) return bad(fn, "raw_capacity is below the number of matches (raw_offsets holds it)");
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_sift_match_lists_dev(int32_t n_frames1, int32_t n_frames2, const mvs_sift_match_params* p, const int64_t* key_offsets1, const float* keys1_dev,
                             const float* descs1_dev, const int64_t* key_offsets2, const float* keys2_dev, const float* descs2_dev,
                             int64_t* raw_offsets, int32_t* raw, int64_t raw_capacity, int64_t* pair_counts, void* hip_stream) {
    MVS_TRACE();
    int rc = check_lists(__func__, n_frames1, n_frames2, p, key_offsets1, keys1_dev, descs1_dev, key_offsets2, keys2_dev, descs2_dev, raw_offsets, raw_capacity);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return lists_core(__func__, n_frames1, n_frames2, p, key_offsets1, keys1_dev, descs1_dev, key_offsets2, keys2_dev, descs2_dev, raw_offsets, raw,
                      raw_capacity, pair_counts, (hipStream_t)hip_stream);
}

int mvs_sift_match_lists(int32_t n_frames1, int32_t n_frames2, const mvs_sift_match_params* p, const int64_t* key_offsets1, const float* keys1,
                         const float* descs1, const int64_t* key_offsets2, const float* keys2, const float* descs2, int64_t* raw_offsets,
                         int32_t* raw, int64_t raw_capacity, int64_t* pair_counts) {
    MVS_TRACE();
    int rc = check_lists(__func__, n_frames1, n_frames2, p, key_offsets1, keys1, descs1, key_offsets2, keys2, descs2, raw_offsets, raw_capacity);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    const size_t t1 = (size_t)key_offsets1[(size_t)n_frames1 * p->view_count], t2 = (size_t)key_offsets2[(size_t)n_frames2 * p->view_count];
    Scratch k1, k2, d1, d2;
    if ((rc = up(k1, keys1, 4 * t1)) || (rc = up(k2, keys2, 4 * t2)) || (rc = up(d1, descs1, 128 * t1)) || (rc = up(d2, descs2, 128 * t2))) return rc;
    return lists_core(__func__, n_frames1, n_frames2, p, key_offsets1, k1.as<float>(), d1.as<float>(), key_offsets2, k2.as<float>(), d2.as<float>(),
                      raw_offsets, raw, raw_capacity, pair_counts, nullptr);
}

// the two lists of the one-pair forms as 1 x 1 sequences of one view
static int one_pair(const char* fn, int64_t n1, const float* descs1, int64_t n2, const float* descs2, const mvs_sift_match_params* p, int32_t* match_buf,
                    int64_t* n_match, const SmHook* hook) {
    if (n1 < 0 || n2 < 0 || n1 >= 0x7fffffffLL || n2 >= 0x7fffffffLL || (n1 && !descs1) || (n2 && !descs2) || !p) return bad(fn, "bad arguments");
    if (p->max_sift < 1) return bad(fn, "need max_sift >= 1");
    int rc = need_device();
    if (rc) return rc;
    mvs_sift_match_params q = *p;
    q.view_count = 1;
    const int64_t off1[2] = {0, n1}, off2[2] = {0, n2};
    Scratch d1, d2;
    if ((rc = up(d1, descs1, 128 * (size_t)n1)) || (rc = up(d2, descs2, 128 * (size_t)n2))) return rc;
    std::vector<int64_t> po;
    if ((rc = sm_core(1, 1, &q, off1, nullptr, d1.as<float>(), off2, nullptr, d2.as<float>(), po, match_buf != nullptr, std::min(n1, n2), match_buf, hook,
                      nullptr))) return rc;
    if (n_match) *n_match = po[1];
    return MVS_OK;
}

int mvs_sift_match(int64_t n1, const float* descs1, int64_t n2, const float* descs2, const mvs_sift_match_params* p, int32_t* match_buf, int64_t* n_match) {
    MVS_TRACE();
    if (!match_buf || !n_match) return bad(__func__, "match_buf or n_match is NULL");
    return one_pair(__func__, n1, descs1, n2, descs2, p, match_buf, n_match, nullptr);
}

int mvs_test_sift_scores(int64_t n1, const float* descs1, int64_t n2, const float* descs2, int32_t max_sift, int32_t* best12, int32_t* idx12,
                         int32_t* second12, int32_t* best21, int32_t* idx21, int32_t* second21) {
    if (!best12 || !idx12 || !second12 || !best21 || !idx21 || !second21) return bad(__func__, "an output is NULL");
    const mvs_sift_match_params p = {1, max_sift, 0.0, 0.0};
    const int64_t c1 = std::min<int64_t>(n1, max_sift), c2 = std::min<int64_t>(n2, max_sift);
    for (int64_t i = 0; i < c1; ++i) { best12[i] = 0; idx12[i] = -1; second12[i] = 0; }       // what an empty other list leaves
    for (int64_t j = 0; j < c2; ++j) { best21[j] = 0; idx21[j] = -1; second21[j] = 0; }
    if (c1 <= 0 || c2 <= 0) return one_pair(__func__, n1, descs1, n2, descs2, &p, nullptr, nullptr, nullptr);
    const SmHook hook = {best12, idx12, second12, best21, idx21, second21};
    return one_pair(__func__, n1, descs1, n2, descs2, &p, nullptr, nullptr, &hook);
}

}  // extern "C"

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_siftmatch() { return (const void*)k_sm_direction; }
