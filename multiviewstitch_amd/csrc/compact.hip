// compact.hip — the tail every ordered compaction of the front end shares (views.hip's key-point cull, siftmatch.hip's pairing,
// sift.hip's candidates, pointsample.hip's rows).  A unit's own count kernel leaves the survivors of each workgroup of COMPACT_TPB
// (engine.h) items in cnt and its own scatter kernel writes survivor r of workgroup b at base[b] + wg_rank; between the two:
//
//   k_ct_scan     : ONE workgroup, base = the exclusive scan of cnt, base[nb] = all survivors (wg_scan_counts)
//   k_ct_segments : off[k] = the survivors in front of item seg[k] (survivors_before): where compacted segment k starts
//   k_ct_strided  : off[k] = base[at(k) * stride]: the same for segments that start on a workgroup boundary
#include "engine.h"
#include "frontend_dev.h"

namespace {

__global__ __launch_bounds__(COMPACT_TPB) void k_ct_scan(const int32_t* __restrict__ cnt, int nb, int32_t* __restrict__ base) {
    wg_scan_counts<COMPACT_TPB / 64>(cnt, nb, base);
}

__global__ void k_ct_segments(const int64_t* __restrict__ seg, int64_t n, int64_t total, const uint8_t* __restrict__ keep,
                              const int32_t* __restrict__ base, int nb, int64_t* __restrict__ off) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n) return;
    off[k] = survivors_before(seg[k], total, keep, base, nb, COMPACT_TPB);
}

__global__ void k_ct_strided(const int32_t* __restrict__ at, int n, int stride, const int32_t* __restrict__ base, int64_t* __restrict__ off) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n) off[k] = base[(int64_t)(at ? at[k] : k) * stride];
}

}  // namespace

int CompactTail::alloc(size_t nb, size_t n, hipStream_t s) {
    int rc;
    if ((rc = cnt.alloc(sizeof(int32_t) * nb, s)) || (rc = base.alloc(sizeof(int32_t) * (nb + 1), s))) return rc;
    return off.alloc(sizeof(int64_t) * (n + 1), s);
}

void CompactTail::segments(int nb, const int64_t* seg_dev, int64_t n, int64_t total, const uint8_t* keep, hipStream_t s) {
    k_ct_scan<<<dim3(1), dim3(COMPACT_TPB), 0, s>>>(cnt.as<int32_t>(), nb, base.as<int32_t>());
    k_ct_segments<<<dim3((unsigned)(n / COMPACT_TPB + 1)), dim3(COMPACT_TPB), 0, s>>>(seg_dev, n, total, keep, base.as<int32_t>(), nb, off.as<int64_t>());
}

void CompactTail::strided(int nb, const int32_t* at_dev, int n, int stride, hipStream_t s) {
    k_ct_scan<<<dim3(1), dim3(COMPACT_TPB), 0, s>>>(cnt.as<int32_t>(), nb, base.as<int32_t>());
    k_ct_strided<<<dim3((unsigned)(n / COMPACT_TPB + 1)), dim3(COMPACT_TPB), 0, s>>>(at_dev, n, stride, base.as<int32_t>(), off.as<int64_t>());
}

// one kernel of this translation unit, for the code-object preload of runtime.cpp
const void* mvs_tu_probe_compact() { return (const void*)k_ct_scan; }
