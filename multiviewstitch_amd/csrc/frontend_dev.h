// frontend_dev.h — the small pieces the units of the `main -a 1` front end share: CheckRange, the 8-bit grey conversion, the segment
// look-up of back-to-back lists, the stage-1 rule of the match filter (one body for the kernel and for host code), the workgroup
// ranking of an ordered compaction (every unit's count and scatter kernels) and the two scan steps behind it (compact.hip).
#ifndef MVS_FRONTEND_DEV_H_
#define MVS_FRONTEND_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

// CheckRange, R/Common/Utils.h:20-22
__host__ __device__ inline bool in_range(int u, int v, int w, int h) { return u >= 0 && u < w && v >= 0 && v < h; }

// cv::cvtColor(COLOR_RGB2GRAY) for 8-bit data.  The conversion is OpenCV's (un-vendored; recollection of its 8-bit fixed-point path
// on the channels in memory order) -> unpinned.
__host__ __device__ inline int grey8(const uint8_t* px) { return (4899 * px[0] + 9617 * px[1] + 1868 * px[2] + 8192) >> 14; }

// the segment of item r: the last k with off[k] <= r (off ascends from 0, off[n] > r; empty segments are skipped)
__host__ __device__ inline int segment_of(const int64_t* __restrict__ off, int n, int64_t r) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------ match keys ----
// A match (u1,v1,u2,v2) of base-view pixels is one 64-bit key, 16 bits each with u1 on top: integer order = the order of the
// reference's set, lexicographic in (u1,v1,u2,v2) (Vector.h:57-63).  The two values below are never keys: u1 = 65535 would need
// w > 65535.
constexpr unsigned long long MP_NONE = ~0ull;              // the raw match was dropped
constexpr unsigned long long MP_BAD_VIEW = ~0ull - 1;      // its view index is outside [0, views): the call is invalid

__host__ __device__ inline unsigned long long mp_key(int u1, int v1, int u2, int v2) {
    return ((unsigned long long)(u1 & 0xffff) << 48) | ((unsigned long long)(v1 & 0xffff) << 32) | ((unsigned long long)(u2 & 0xffff) << 16) |
           (unsigned long long)(v2 & 0xffff);
}

// Stage 1 for one raw match q = (view1,u1,v1,view2,u2,v2) between generated views (R/Processor/Processor.cpp:658-662): the range
// test, the texIndex look-up in the frame's own stack tex [views][w*h], the -1 test, the valid read at the GENERATED-view pixel
// (:661) -> the key of the two base-view pixels, MP_NONE or MP_BAD_VIEW
__host__ __device__ inline unsigned long long mp_stage1(const int32_t* q, const int32_t* __restrict__ tex1, const uint8_t* __restrict__ valid1,
                                                        const int32_t* __restrict__ tex2, const uint8_t* __restrict__ valid2, int w, int h,
                                                        int views) {
    const int a1 = q[0], u1 = q[1], v1 = q[2], a2 = q[3], u2 = q[4], v2 = q[5];
    if (a1 < 0 || a1 >= views || a2 < 0 || a2 >= views) return MP_BAD_VIEW;
    if (!in_range(u1, v1, w, h) || !in_range(u2, v2, w, h)) return MP_NONE;
    const int64_t npx = (int64_t)w * h, px1 = (int64_t)v1 * w + u1, px2 = (int64_t)v2 * w + u2;
    const int idx1 = tex1[a1 * npx + px1], idx2 = tex2[a2 * npx + px2];
    if (idx1 == -1 || idx2 == -1 || !valid1[px1] || !valid2[px2]) return MP_NONE;
    return mp_key(idx1 % w, idx1 / w, idx2 % w, idx2 / w);
}

#ifdef __HIPCC__
// ---------------------------------------------------------- ordered compaction ----
// The place of a thread's flag among the set flags of its workgroup of WAVES waves, in thread order, and how many are set: a
// ballot, the popcount below the lane, and the sums of the waves before it from s_wsum[WAVES] (LDS).  Every thread of the workgroup
// calls it; it holds ONE barrier, between the write of s_wsum and its reads — a caller that calls it again puts a barrier of its
// own in between.
struct WgRank { int rank, total; };
template <int WAVES>
__device__ inline WgRank wg_rank(bool flag, int* s_wsum) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) s_wsum[wv] = __popcll(bal);
    __syncthreads();
    WgRank r = {(int)__popcll(bal & ((1ull << lane) - 1ull)), 0};
#pragma unroll
    for (int q = 0; q < WAVES; ++q) { if (q < wv) r.rank += s_wsum[q]; r.total += s_wsum[q]; }
    return r;
}

// The scan over the survivor counts of nb workgroups, run by ONE workgroup of WAVES waves: base[b] = survivors in the workgroups
// before b, base[nb] = all survivors.
template <int WAVES>
__device__ inline void wg_scan_counts(const int32_t* __restrict__ cnt, int nb, int32_t* __restrict__ base) {
    __shared__ int s_wsum[WAVES], s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += WAVES * 64) {
        const int i = c0 + tid, v = i < nb ? cnt[i] : 0;
        int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(x, o, 64);
            if (lane >= o) x += t;
        }
        if (lane == 63) s_wsum[wv] = x;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) { if (q < wv) woff += s_wsum[q]; tot += s_wsum[q]; }
        const int carry = s_carry;
        if (i < nb) base[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == 0) s_carry = carry + tot;
        __syncthreads();
    }
    if (tid == 0) base[nb] = s_carry;
}

// The survivors in front of item r (of `total`, flagged in keep, counted per workgroup of tpb items into base[nb + 1] by the scan
// above): where the compacted segment that starts at r begins
__device__ inline int64_t survivors_before(int64_t r, int64_t total, const uint8_t* __restrict__ keep, const int32_t* __restrict__ base,
                                           int nb, int tpb) {
    if (r >= total) return base[nb];
    const int64_t b = r / tpb;
    int64_t acc = base[b];
    for (int64_t q = b * tpb; q < r; ++q) acc += keep[q];
    return acc;
}
#endif  // __HIPCC__

#endif
