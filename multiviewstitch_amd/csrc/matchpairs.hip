// matchpairs.hip — one turn of the sequence-pair loop of Processor::CalcSimilarityTransformationSeq (R/Processor/Processor.cpp:629-826,
// without the match JPEGs of :767-793) for ALL n1 x n2 frame pairs of two adjacent sequences at once:
//
//   k_mp_map      : one thread per raw match (view1,u1,v1,view2,u2,v2): the stage-1 rule (mp_stage1, frontend_dev.h; :658-662) -> one
//                   64-bit key or MP_NONE
//   k_mp_cascade  : one workgroup per frame pair, the pair's keys in LDS: bitonic sort + unique (:650-680), SSD window (:683-707,
//                   Utils.h:221-241), ordered compaction, greedy gap filter in list order (:713-735)
//   k_mp_pack     : the survivors of every pair back to back (the layout of mvs_match_filter's `out`, pair after pair)
//   k_mp_lift     : one thread per surviving match: Image3D::GetPoint of both endpoints (:806-811) with k_depth_unproject's arithmetic
//
// A pair whose stage-1 input exceeds the LDS capacity (knobs.h MVS_MATCH_PAIRS_LDS_KEYS, lowered by MVS_MATCH_PAIRS_LDS_CAP) runs the
// same kernel body on a slice of a global-memory workspace: the body takes a flat pointer.  Every loop with a barrier in it has a
// trip count that depends only on per-pair sizes every thread of the workgroup reads from the same place; no workgroup waits on
// another one.
//
// mvs_match_filter, the ONE-pair entry (:644-735), is a client of the same cascade: the stage-1 rule runs on the host over the caller's
// arrays (the tex stacks and masks are never uploaded), the keys and the two base images go up and k_mp_cascade runs as the 1 x 1 case.
#include "engine.h"
#include "trace.h"
#include "knobs.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int MP_TPB = 256;
constexpr int MP_WAVES = MP_TPB / 64;
static_assert((MVS_MATCH_PAIRS_LDS_KEYS & (MVS_MATCH_PAIRS_LDS_KEYS - 1)) == 0, "the bitonic sort pads to a power of two");

struct MpMatch { int u1, v1, u2, v2; };
__device__ inline MpMatch mp_unkey(unsigned long long k) {
    MpMatch m = {(int)(k >> 48), (int)((k >> 32) & 0xffff), (int)((k >> 16) & 0xffff), (int)(k & 0xffff)};
    return m;
}

__global__ void k_mp_map(const int32_t* __restrict__ raw, int64_t total, const int64_t* __restrict__ raw_off, int npairs, int n2,
                         const int32_t* __restrict__ tex1, const uint8_t* __restrict__ valid1, const int32_t* __restrict__ tex2,
                         const uint8_t* __restrict__ valid2, int w, int h, int views, unsigned long long* __restrict__ keys,
                         int32_t* __restrict__ bad_view) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= total) return;
    const int k = segment_of(raw_off, npairs, r);
    const int64_t i = k / n2, j = k % n2, npx = (int64_t)w * h;
    unsigned long long key = mp_stage1(raw + 6 * r, tex1 + i * views * npx, valid1 + i * npx, tex2 + j * views * npx, valid2 + j * npx, w, h, views);
    if (key == MP_BAD_VIEW) {
        *bad_view = 1;                                                     // the call returns MVS_E_INVALID_ARG
        key = MP_NONE;
    }
    keys[r] = key;
}

// Ordered in-place compaction of buf[0, n): element i stays iff keep(i, key, key of i - 1).  The predecessor of a chunk's first
// element travels in *s_last, because the chunk before it has already been compacted over.  n is workgroup-uniform.
template <class F>
__device__ inline int mp_compact(unsigned long long* buf, int n, F keep, int* s_wsum, unsigned long long* s_last) {
    const int tid = threadIdx.x;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += MP_TPB) {
        const int i = c0 + tid;
        unsigned long long key = MP_NONE;
        bool f = false;
        if (i < n) {
            key = buf[i];
            const unsigned long long prev = tid > 0 ? buf[i - 1] : (c0 > 0 ? *s_last : MP_NONE);
            f = keep(i, key, prev);
        }
        __syncthreads();                                                    // every read of this chunk (and of *s_last, s_wsum) is done
        if (tid == MP_TPB - 1) *s_last = key;
        const WgRank k = wg_rank<MP_WAVES>(f, s_wsum);                      // (its barrier: the writes of the chunk start behind it)
        if (f) buf[base + k.rank] = key;                                    // base + k.rank <= i, inside chunks already read
        base += k.total;
    }
    __syncthreads();
    return base;
}

__global__ __launch_bounds__(MP_TPB) void k_mp_cascade(const unsigned long long* __restrict__ keys, const int64_t* __restrict__ raw_off, int n2,
                                                       int cap, unsigned long long* ws, const int64_t* __restrict__ ws_off,
                                                       const uint8_t* __restrict__ imgs1, const uint8_t* __restrict__ imgs2, int w, int h,
                                                       int win, double ssd_err, double gap, int32_t* __restrict__ out,
                                                       int32_t* __restrict__ counts) {
    __shared__ unsigned long long lds[MVS_MATCH_PAIRS_LDS_KEYS];
    __shared__ unsigned long long s_last;
    __shared__ int s_cnt, s_wsum[MP_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = raw_off[k];
    const int n = (int)(raw_off[k + 1] - r0);
    if (n == 0) return;                                                     // (counts were cleared by the host)
    // how many raw matches survived the map
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += MP_TPB) mine += keys[r0 + i] != MP_NONE;
    mine = wave_sum_i(mine);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    const int m = s_cnt;
    if (m == 0) return;
    // in LDS when they fit, else in this pair's slice of the workspace (the host gave one to every pair with n > cap >= its m)
    unsigned long long* buf = m <= cap ? lds : ws + ws_off[k];
    int P = 1;
    while (P < m) P <<= 1;
    __syncthreads();
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = tid; i < n; i += MP_TPB) {
        const unsigned long long key = keys[r0 + i];
        if (key != MP_NONE) buf[atomicAdd(&s_cnt, 1)] = key;                // any order: the sort follows
    }
    for (int i = m + tid; i < P; i += MP_TPB) buf[i] = MP_NONE;
    __syncthreads();
    // 1. the ordered set of :650-680: bitonic sort (ascending), then unique
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += MP_TPB) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = buf[i], b = buf[l];
                if ((a > b) == ((i & kk) == 0)) { buf[i] = b; buf[l] = a; }
            }
            __syncthreads();
        }
    const int c1 = mp_compact(buf, m, [](int i, unsigned long long key, unsigned long long prev) { return i == 0 || key != prev; }, s_wsum, &s_last);
    // 2. SSD window (Utils.h:221-241): the sum of squared integer grey differences (exact), the root mean square tested in double
    const int64_t npx = (int64_t)w * h;
    const uint8_t* img1 = imgs1 + 3 * npx * (k / n2);
    const uint8_t* img2 = imgs2 + 3 * npx * (k % n2);
    const int c2 = mp_compact(buf, c1, [=](int, unsigned long long key, unsigned long long) {
        const MpMatch q = mp_unkey(key);
        if (!(q.u1 >= win && q.v1 >= win && q.u2 >= win && q.v2 >= win && q.u1 < w - win && q.v1 < h - win && q.u2 < w - win && q.v2 < h - win))
            return false;                                                   // window outside an image: dropped (:692-693)
        const int len = 2 * win + 1;
        unsigned long long sum = 0;
        for (int a = 0; a < len; ++a) {
            const uint8_t* p1 = img1 + 3 * ((int64_t)(q.v1 - win + a) * w + (q.u1 - win));
            const uint8_t* p2 = img2 + 3 * ((int64_t)(q.v2 - win + a) * w + (q.u2 - win));
            for (int b = 0; b < len; ++b) {
                const int d = grey8(p1 + 3 * b) - grey8(p2 + 3 * b);
                sum += (unsigned long long)(d * d);
            }
        }
        return sqrt((double)sum / (len * len)) <= ssd_err;
    }, s_wsum, &s_last);
    // 3. greedy gap filter in list order: the kept list grows at the front of buf.  Slot q is written and read by thread q % MP_TPB
    // alone, and a candidate is read by everybody before the OR (a barrier) that decides it, so the OR is the only barrier needed.
    int c3 = 0;
    for (int c = 0; c < c2; ++c) {
        const unsigned long long cand = buf[c];
        const MpMatch b = mp_unkey(cand);
        bool close = false;
        for (int q = tid; q < c3; q += MP_TPB) {
            const MpMatch a = mp_unkey(buf[q]);
            const int64_t x0 = a.u1 - b.u1, x1 = a.v1 - b.v1, y0 = a.u2 - b.u2, y1 = a.v2 - b.v2;
            close = close || (double)(x0 * x0 + x1 * x1) <= gap || (double)(y0 * y0 + y1 * y1) <= gap;      // :724
        }
        if (!__syncthreads_or(close)) {
            if (tid == c3 % MP_TPB) buf[c3] = cand;
            ++c3;
        }
    }
    __syncthreads();
    for (int q = tid; q < c3; q += MP_TPB) {
        const MpMatch a = mp_unkey(buf[q]);
        int32_t* o = out + 4 * (r0 + q);
        o[0] = a.u1; o[1] = a.v1; o[2] = a.u2; o[3] = a.v2;
    }
    if (tid == 0) { counts[3 * k] = c1; counts[3 * k + 1] = c2; counts[3 * k + 2] = c3; }
}

__global__ __launch_bounds__(MP_TPB) void k_mp_pack(const int32_t* __restrict__ in, const int64_t* __restrict__ raw_off,
                                                    const int64_t* __restrict__ out_off, int32_t* __restrict__ out) {
    const int k = blockIdx.x;
    const int64_t src = 4 * raw_off[k], dst = 4 * out_off[k], n = 4 * (out_off[k + 1] - out_off[k]);
    for (int64_t i = threadIdx.x; i < n; i += MP_TPB) out[dst + i] = in[src + i];
}

// Image3D::valid as SolveUnProjectionD sets it (Image3D.cpp:98-101, k_depth_unproject)
__global__ void k_mp_valid(const float* __restrict__ dsp, int64_t n, double mn, double mx, uint8_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = (double)dsp[i];
    valid[i] = (d < mn || d > mx) ? 0 : 1;
}

__global__ void k_mp_lift(const int32_t* __restrict__ m, int64_t total, const int64_t* __restrict__ off, int npairs, int n2,
                          const float* __restrict__ dsp1, const float* __restrict__ dsp2, const CamDev* __restrict__ c1,
                          const CamDev* __restrict__ c2, double mn, double mx, double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= total) return;
    const int k = segment_of(off, npairs, r), i = k / n2, j = k % n2;
    const CamDev a = c1[i], b = c2[j];
    const int32_t* q = m + 4 * r;                                           // inside both images: the SSD stage kept it
    st3(out + 6 * r, point_from_raster(dsp1 + (int64_t)i * a.w * a.h, a, q[0], q[1], mn, mx));
    st3(out + 6 * r + 3, point_from_raster(dsp2 + (int64_t)j * b.w * b.h, b, q[2], q[3], mn, mx));
}

int check_pairs(const char* fn, int32_t n1, int32_t n2, const int64_t* raw_off, const int32_t* raw, const mvs_match_filter_params* p) {
    if (n1 <= 0 || n2 <= 0 || (int64_t)n1 * n2 > 1000000) return bad(fn, "need n1, n2 >= 1 and n1 * n2 <= 1000000");
    if (!raw_off || !p) return bad(fn, "raw_offsets / params is NULL");
    if (p->w <= 0 || p->h <= 0 || p->view_count <= 0 || p->ssd_win < 0) return bad(fn, "need w, h, view_count > 0 and ssd_win >= 0");
    if (p->w > 65535 || p->h > 65535) return bad(fn, "w and h must not exceed 65535 (a match is one 64-bit key)");
    if (int rc = check_offsets(fn, "raw_offsets", raw_off, n1 * n2, 0x7fffffffLL)) return rc;
    if (raw_off[n1 * n2] > 0 && !raw) return bad(fn, "raw is NULL");
    return MVS_OK;
}

// what the cascade leaves: the survivors of every pair back to back in HBM, their offsets and the stage sizes on the host
struct PairsOut {
    Scratch packed;                    // int32 [off[np]][4]; not allocated when nothing survived
    std::vector<int64_t> off;          // np + 1
    std::vector<int32_t> counts;       // np x 3
};

// what the two halves of the cascade share in HBM; the blocks go back when the call is over
struct PairsDev {
    Scratch raw, off, keys, cnt;       // raw matches (map only); raw_off [np + 1]; one key per raw match; stage sizes [np][3], then the
                                       // bad-view flag of the map
};

// off uploaded, keys allocated, the stage sizes and the flag cleared (counts of empty pairs are never written by the cascade)
int pairs_begin(PairsDev& d, int np, const int64_t* raw_off, hipStream_t s) {
    int rc;
    if ((rc = up_async(d.off, raw_off, (size_t)np + 1, s)) || (rc = d.keys.alloc(sizeof(unsigned long long) * (size_t)raw_off[np], s)) ||
        (rc = d.cnt.alloc(sizeof(int32_t) * (3 * (size_t)np + 1), s))) return rc;
    HIPCHK(hipMemsetAsync(d.cnt.p, 0, sizeof(int32_t) * (3 * (size_t)np + 1), s));
    return MVS_OK;
}

// stage 1 of every pair: tex / valid stacks in HBM, raw and raw_off on the host; enqueues on s
int pairs_map(int n1, int n2, const int64_t* raw_off, const int32_t* raw, const int32_t* tex1, const uint8_t* valid1, const int32_t* tex2,
              const uint8_t* valid2, const mvs_match_filter_params* p, hipStream_t s, PairsDev& d) {
    const int np = n1 * n2;
    const int64_t total = raw_off[np];
    if (total == 0) return MVS_OK;
    int rc;
    if ((rc = up_async(d.raw, raw, 6 * (size_t)total, s)) || (rc = pairs_begin(d, np, raw_off, s))) return rc;
    k_mp_map<<<dim3((unsigned)((total + MP_TPB - 1) / MP_TPB)), dim3(MP_TPB), 0, s>>>(d.raw.as<int32_t>(), total, d.off.as<int64_t>(), np, n2, tex1, valid1,
                                                                                     tex2, valid2, p->w, p->h, p->view_count,
                                                                                     d.keys.as<unsigned long long>(), d.cnt.as<int32_t>() + 3 * (size_t)np);
    HIPCHK(hipGetLastError());
    return MVS_OK;
}

// stages 1 (sort, unique) to 3 of every pair from the keys in d (pairs_begin, then pairs_map or an upload); images in HBM.  Returns
// with s synchronised.
int pairs_cascade(int n1, int n2, const int64_t* raw_off, const PairsDev& d, const uint8_t* imgs1, const uint8_t* imgs2,
                  const mvs_match_filter_params* p, hipStream_t s, PairsOut& o) {
    const int np = n1 * n2;
    const int64_t total = raw_off[np];
    o.off.assign((size_t)np + 1, 0);
    o.counts.assign((size_t)np * 3, 0);
    if (total == 0) return MVS_OK;
    const int cap = mvs_match_pairs_lds_cap();
    std::vector<int64_t> ws_off((size_t)np, 0);
    int64_t ws_total = 0;
    for (int k = 0; k < np; ++k) {                                          // a pair with more keys than cap MAY need the workspace
        const int64_t n = raw_off[k + 1] - raw_off[k];
        if (n <= cap) continue;
        int64_t P = 1;
        while (P < n) P <<= 1;
        ws_off[k] = ws_total;
        ws_total += P;
    }
    Scratch dwsoff, dws, dout;
    int rc;
    if ((rc = up_async(dwsoff, ws_off.data(), ws_off.size(), s)) || (rc = dws.alloc(sizeof(unsigned long long) * (size_t)ws_total, s)) ||
        (rc = dout.alloc(sizeof(int32_t) * 4 * (size_t)total, s))) return rc;
    const double gap = (double)p->sample_interval * (double)p->sample_interval;         // :713
    k_mp_cascade<<<dim3((unsigned)np), dim3(MP_TPB), 0, s>>>(d.keys.as<unsigned long long>(), d.off.as<int64_t>(), n2, cap, dws.as<unsigned long long>(),
                                                            dwsoff.as<int64_t>(), imgs1, imgs2, p->w, p->h, p->ssd_win, p->ssd_err, gap,
                                                            dout.as<int32_t>(), d.cnt.as<int32_t>());
    HIPCHK(hipGetLastError());
    std::vector<int32_t> hc(3 * (size_t)np + 1);
    HIPCHK(hipMemcpyAsync(hc.data(), d.cnt.p, sizeof(int32_t) * hc.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (hc.back()) { mvs_set_error("match filter: view index out of range"); return MVS_E_INVALID_ARG; }
    hc.pop_back();
    o.counts = hc;
    for (int k = 0; k < np; ++k) o.off[k + 1] = o.off[k] + hc[3 * (size_t)k + 2];
    const int64_t kept = o.off[np];
    if (kept == 0) return MVS_OK;
    Scratch dooff;
    if ((rc = o.packed.alloc(sizeof(int32_t) * 4 * (size_t)kept, s)) || (rc = up_async(dooff, o.off.data(), o.off.size(), s))) return rc;
    k_mp_pack<<<dim3((unsigned)np), dim3(MP_TPB), 0, s>>>(dout.as<int32_t>(), d.off.as<int64_t>(), dooff.as<int64_t>(), o.packed.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// the cascade over every pair; all image / table stacks in HBM, raw and raw_off on the host.  Returns with s synchronised.
int pairs_core(int n1, int n2, const int64_t* raw_off, const int32_t* raw, const int32_t* tex1, const uint8_t* valid1, const int32_t* tex2,
               const uint8_t* valid2, const uint8_t* imgs1, const uint8_t* imgs2, const mvs_match_filter_params* p, hipStream_t s,
               PairsOut& o) {
    PairsDev d;
    int rc = pairs_map(n1, n2, raw_off, raw, tex1, valid1, tex2, valid2, p, s, d);
    return rc ? rc : pairs_cascade(n1, n2, raw_off, d, imgs1, imgs2, p, s, o);
}

void copy_counts(const PairsOut& o, int64_t* stage_counts) {
    if (stage_counts)
        for (size_t i = 0; i < o.counts.size(); ++i) stage_counts[i] = o.counts[i];
}

}  // namespace

extern "C" {

int mvs_match_filter(const int32_t* raw, int64_t n, const int32_t* tex1, const uint8_t* valid1, const int32_t* tex2, const uint8_t* valid2,
                     const uint8_t* img1, const uint8_t* img2, const mvs_match_filter_params* p, int32_t* out, int64_t* n_out,
                     int64_t* stage_counts) {
    if (n < 0 || (n && !raw) || !tex1 || !valid1 || !tex2 || !valid2 || !img1 || !img2 || !p || !out || !n_out || p->w <= 0 || p->h <= 0 ||
        p->view_count <= 0 || p->ssd_win < 0) return bad(__func__, "bad arguments");
    if (p->w > 65535 || p->h > 65535) return bad(__func__, "w and h must not exceed 65535 (a match is one 64-bit key)");
    std::vector<unsigned long long> keys;                                   // stage 1 on the host: the stacks and masks stay where they are
    for (int64_t k = 0; k < n; ++k) {
        const unsigned long long key = mp_stage1(raw + 6 * k, tex1, valid1, tex2, valid2, p->w, p->h, p->view_count);
        if (key == MP_BAD_VIEW) return bad(__func__, "view index out of range");
        if (key != MP_NONE) keys.push_back(key);
    }
    if (keys.size() >= 0x7fffffffULL) return bad(__func__, "more than 2^31 - 1 matches");
    int rc = need_device();
    if (rc) return rc;
    const int64_t off[2] = {0, (int64_t)keys.size()};
    const size_t npx = (size_t)p->w * p->h;
    PairsDev d;
    Scratch i1, i2;
    if (off[1] > 0) {
        if ((rc = pairs_begin(d, 1, off, nullptr)) || (rc = up(i1, img1, npx * 3)) || (rc = up(i2, img2, npx * 3))) return rc;
        HIPCHK(hipMemcpyAsync(d.keys.p, keys.data(), sizeof(unsigned long long) * keys.size(), hipMemcpyHostToDevice, nullptr));
    }
    PairsOut o;
    if ((rc = pairs_cascade(1, 1, off, d, i1.as<uint8_t>(), i2.as<uint8_t>(), p, nullptr, o))) return rc;
    if ((rc = down(out, o.packed, 4 * (size_t)o.off[1]))) return rc;
    *n_out = o.off[1];
    copy_counts(o, stage_counts);
    return MVS_OK;
}

int mvs_match_filter_pairs_dev(int32_t n1, int32_t n2, const int64_t* raw_offsets, const int32_t* raw, const int32_t* tex1_dev,
                               const uint8_t* valid1_dev, const int32_t* tex2_dev, const uint8_t* valid2_dev, const uint8_t* imgs1_dev,
                               const uint8_t* imgs2_dev, const mvs_match_filter_params* p, int32_t* out, int64_t* out_offsets,
                               int64_t* stage_counts, void* hip_stream) {
    MVS_TRACE();
    int rc = check_pairs(__func__, n1, n2, raw_offsets, raw, p);
    if (rc) return rc;
    if (!tex1_dev || !valid1_dev || !tex2_dev || !valid2_dev || !imgs1_dev || !imgs2_dev || !out_offsets || (raw_offsets[n1 * n2] > 0 && !out))
        return bad(__func__, "a stack, out or out_offsets is NULL");
    if ((rc = need_device())) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    PairsOut o;
    if ((rc = pairs_core(n1, n2, raw_offsets, raw, tex1_dev, valid1_dev, tex2_dev, valid2_dev, imgs1_dev, imgs2_dev, p, s, o))) return rc;
    const int64_t kept = o.off.back();
    if (kept > 0) {
        HIPCHK(hipMemcpyAsync(out, o.packed.p, sizeof(int32_t) * 4 * (size_t)kept, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    std::memcpy(out_offsets, o.off.data(), sizeof(int64_t) * o.off.size());
    copy_counts(o, stage_counts);
    return MVS_OK;
}

int mvs_match_filter_pairs(int32_t n1, int32_t n2, const int64_t* raw_offsets, const int32_t* raw, const int32_t* tex1, const uint8_t* valid1,
                           const int32_t* tex2, const uint8_t* valid2, const uint8_t* imgs1, const uint8_t* imgs2,
                           const mvs_match_filter_params* p, int32_t* out, int64_t* out_offsets, int64_t* stage_counts) {
    MVS_TRACE();
    int rc = check_pairs(__func__, n1, n2, raw_offsets, raw, p);
    if (rc) return rc;
    if (!tex1 || !valid1 || !tex2 || !valid2 || !imgs1 || !imgs2 || !out_offsets || (raw_offsets[n1 * n2] > 0 && !out))
        return bad(__func__, "a stack, out or out_offsets is NULL");
    if ((rc = need_device())) return rc;
    const size_t npx = (size_t)p->w * p->h, v = (size_t)p->view_count;
    Scratch t1, t2, v1, v2, i1, i2;                                        // every stack once
    if ((rc = up(t1, tex1, n1 * v * npx)) || (rc = up(t2, tex2, n2 * v * npx)) || (rc = up(v1, valid1, n1 * npx)) || (rc = up(v2, valid2, n2 * npx)) ||
        (rc = up(i1, imgs1, n1 * npx * 3)) || (rc = up(i2, imgs2, n2 * npx * 3))) return rc;
    PairsOut o;
    if ((rc = pairs_core(n1, n2, raw_offsets, raw, t1.as<int32_t>(), v1.as<uint8_t>(), t2.as<int32_t>(), v2.as<uint8_t>(), i1.as<uint8_t>(),
                         i2.as<uint8_t>(), p, nullptr, o))) return rc;
    if ((rc = down(out, o.packed, 4 * (size_t)o.off.back()))) return rc;
    std::memcpy(out_offsets, o.off.data(), sizeof(int64_t) * o.off.size());
    copy_counts(o, stage_counts);
    return MVS_OK;
}

int mvs_sequence_pair_srt(int32_t n1, int32_t n2, const mvs_camera* cams1, const mvs_camera* cams2, const float* depths1, const float* depths2,
                          const int64_t* raw_offsets, const int32_t* raw, const int32_t* tex1, const int32_t* tex2, const uint8_t* imgs1,
                          const uint8_t* imgs2, const mvs_seq_pair_params* p, uint32_t* rand_state, int32_t* frm_idx1, int32_t* frm_idx2,
                          double* scale, double* R, double* t, double* residual, int64_t* stage_counts, int64_t* n_keep, double* pair_err,
                          int64_t* n_sel, double* sel_matches) {
    MVS_TRACE();
    if (!p) return bad(__func__, "params is NULL");
    int rc = check_pairs(__func__, n1, n2, raw_offsets, raw, &p->filter);
    if (rc) return rc;
    if (!cams1 || !cams2 || !depths1 || !depths2 || !tex1 || !tex2 || !imgs1 || !imgs2 || !rand_state || !frm_idx1 || !frm_idx2 || !scale || !R || !t)
        return bad(__func__, "a required pointer is NULL");
    if (p->ransac_iters < 1) return bad(__func__, "ransac_iters must be >= 1");
    const int w = p->filter.w, h = p->filter.h;
    for (int i = 0; i < n1; ++i) if (cams1[i].w != w || cams1[i].h != h) return bad(__func__, "every camera must have the size w x h of the filter parameters");
    for (int j = 0; j < n2; ++j) if (cams2[j].w != w || cams2[j].h != h) return bad(__func__, "every camera must have the size w x h of the filter parameters");
    if ((rc = need_device())) return rc;
    const int np = n1 * n2;
    const size_t npx = (size_t)w * h, v = (size_t)p->filter.view_count;
    Scratch t1, t2, v1, v2, i1, i2, d1, d2;
    if ((rc = up(t1, tex1, n1 * v * npx)) || (rc = up(t2, tex2, n2 * v * npx)) || (rc = up(i1, imgs1, n1 * npx * 3)) || (rc = up(i2, imgs2, n2 * npx * 3)) ||
        (rc = up(d1, depths1, n1 * npx)) || (rc = up(d2, depths2, n2 * npx)) || (rc = v1.alloc(n1 * npx)) || (rc = v2.alloc(n2 * npx))) return rc;
    k_mp_valid<<<dim3((unsigned)((n1 * npx + MP_TPB - 1) / MP_TPB)), dim3(MP_TPB)>>>(d1.as<float>(), (int64_t)(n1 * npx), p->min_dsp, p->max_dsp, v1.as<uint8_t>());
    k_mp_valid<<<dim3((unsigned)((n2 * npx + MP_TPB - 1) / MP_TPB)), dim3(MP_TPB)>>>(d2.as<float>(), (int64_t)(n2 * npx), p->min_dsp, p->max_dsp, v2.as<uint8_t>());
    HIPCHK(hipGetLastError());
    PairsOut o;                                                             // :644-735
    if ((rc = pairs_core(n1, n2, raw_offsets, raw, t1.as<int32_t>(), v1.as<uint8_t>(), t2.as<int32_t>(), v2.as<uint8_t>(), i1.as<uint8_t>(),
                         i2.as<uint8_t>(), &p->filter, nullptr, o))) return rc;
    copy_counts(o, stage_counts);
    const int64_t kept = o.off[np];
    std::vector<double> m3((size_t)kept * 6);                               // every pair's matches lifted (RemoveOutliers lifts them, :177-192)
    if (kept > 0) {
        std::vector<CamDev> c1((size_t)n1), c2((size_t)n2);
        for (int i = 0; i < n1; ++i) c1[i] = make_camdev(cams1 + i);
        for (int j = 0; j < n2; ++j) c2[j] = make_camdev(cams2 + j);
        Scratch dc1, dc2, doff, dm3;
        if ((rc = up(dc1, c1.data(), c1.size())) || (rc = up(dc2, c2.data(), c2.size())) || (rc = up(doff, o.off.data(), o.off.size())) ||
            (rc = dm3.alloc(sizeof(double) * 6 * (size_t)kept))) return rc;
        k_mp_lift<<<dim3((unsigned)((kept + MP_TPB - 1) / MP_TPB)), dim3(MP_TPB)>>>(o.packed.as<int32_t>(), kept, doff.as<int64_t>(), np, n2, d1.as<float>(),
                                                                                   d2.as<float>(), dc1.as<CamDev>(), dc2.as<CamDev>(), p->min_dsp,
                                                                                   p->max_dsp, dm3.as<double>());
        HIPCHK(hipGetLastError());
        if ((rc = down(m3.data(), dm3, m3.size()))) return rc;
    }
    std::vector<uint8_t> keep((size_t)kept + 1);
    std::vector<int64_t> nk((size_t)np);
    double err = HUGE_VAL;                                                  // :746-765, :794-800
    rc = mvs_select_keyframe_pair(n1, n2, cams1, cams2, o.off.data(), m3.data(), p->min_match_count, p->ransac_iters, p->pixel_err, p->adapt_ratio,
                                  rand_state, frm_idx1, frm_idx2, &err, keep.data(), nk.data(), pair_err);
    if (rc != MVS_OK && rc != MVS_E_DEGENERATE) return rc;
    if (n_keep) std::memcpy(n_keep, nk.data(), sizeof(int64_t) * (size_t)np);
    if (rc) return rc;
    const int ks = *frm_idx1 * n2 + *frm_idx2;                              // :806-811: the selected pair's list as RemoveOutliers left it
    std::vector<double> sel;
    for (int64_t i = o.off[ks]; i < o.off[ks + 1]; ++i)
        if (keep[(size_t)i]) sel.insert(sel.end(), m3.begin() + 6 * i, m3.begin() + 6 * i + 6);
    const int64_t ns = (int64_t)sel.size() / 6;
    if (n_sel) *n_sel = ns;
    if (sel_matches && ns) std::memcpy(sel_matches, sel.data(), sizeof(double) * sel.size());
    double res = 0.0;                                                       // :814-818
    if ((rc = mvs_srt_fit(sel.data(), ns, cams1 + *frm_idx1, cams2 + *frm_idx2, MVS_SRT_CLOSED_FORM, nullptr, 0, 0, scale, R, t, &res))) return rc;
    if (residual) *residual = res;
    return MVS_OK;
}

}  // extern "C"

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_matchpairs() { return (const void*)k_mp_cascade; }
