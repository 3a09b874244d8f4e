// scan_dev.h — the device-wide exclusive scan: three launches over tiles of 1024 items, In the items' type, Acc the sums'.  grid.hip
// instantiates <int32_t, int32_t> (scan_exclusive_i32(_async), engine.h), jpeg_enc.hip <uint32_t, uint64_t>.  DESIGN.md 4o lists the
// scans that stay apart.
#ifndef MVS_SCAN_DEV_H_
#define MVS_SCAN_DEV_H_
#include <hip/hip_runtime.h>

constexpr int SCAN_TPB = 256, SCAN_ELEMS = 1024;

template <class In, class Acc>
__global__ void k_scan_block_sums(const In* __restrict__ in, int64_t n, Acc* __restrict__ bsum) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_ELEMS;
    Acc s = 0;
    for (int k = threadIdx.x; k < SCAN_ELEMS; k += blockDim.x)
        if (base + k < n) s += in[base + k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ Acc sm[SCAN_TPB / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { Acc t = 0; for (int w = 0; w < SCAN_TPB / 64; ++w) t += sm[w]; bsum[blockIdx.x] = t; }
}

// exclusive scan of the nb block sums in place, ONE workgroup of 1024 threads: a thread owns a contiguous run of ceil(nb / 1024)
// sums (a wave walking 64 at a time took 13-43 us for the 2-64 K block sums of a target grid or a 2 M-vertex compaction)
template <class Acc>
__global__ __launch_bounds__(1024) void k_scan_sums_serial(Acc* bsum, int64_t nb) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t per = (nb + 1023) / 1024, lo = (int64_t)t * per, hi = lo + per < nb ? lo + per : nb;
    Acc sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += bsum[i];
    Acc x = sum;
    for (int o = 1; o < 64; o <<= 1) { const Acc y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    __shared__ Acc sm[16];
    if (lane == 63) sm[wv] = x;
    __syncthreads();
    Acc off = 0;
    for (int w = 0; w < wv; ++w) off += sm[w];
    Acc run = off + x - sum;
    for (int64_t i = lo; i < hi; ++i) { const Acc v = bsum[i]; bsum[i] = run; run += v; }
}

template <class In, class Acc>
__global__ void k_scan_apply(const In* __restrict__ in, int64_t n, const Acc* __restrict__ bsum, Acc* __restrict__ out) {
    // each thread owns 4 consecutive elements of the block's 1024
    const int64_t base = (int64_t)blockIdx.x * SCAN_ELEMS + threadIdx.x * 4;
    In v[4];
    Acc t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = (base + k < n) ? in[base + k] : 0; t += v[k]; }
    Acc x = t;
    for (int o = 1; o < 64; o <<= 1) { const Acc y = __shfl_up(x, o, 64); if ((int)(threadIdx.x & 63) >= o) x += y; }
    __shared__ Acc sm[SCAN_TPB / 64];
    if ((threadIdx.x & 63) == 63) sm[threadIdx.x >> 6] = x;
    __syncthreads();
    Acc off = bsum[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += sm[w];
    Acc run = off + x - t;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k <= n) out[base + k] = run; run += v[k]; }   // out has n+1 entries
}

// in: n entries; out: n+1 entries, out[n] = total; bsum: (n + 1 + 1023) / 1024 sums of workspace.  No allocation, no host sync.
template <class In, class Acc>
inline void scan_exclusive_async(const In* in, int64_t n, Acc* out, Acc* bsum, hipStream_t s) {
    const int64_t nb = (n + 1 + SCAN_ELEMS - 1) / SCAN_ELEMS;
    k_scan_block_sums<In, Acc><<<dim3((unsigned)nb), dim3(SCAN_TPB), 0, s>>>(in, n, bsum);
    k_scan_sums_serial<Acc><<<dim3(1), dim3(1024), 0, s>>>(bsum, nb);
    k_scan_apply<In, Acc><<<dim3((unsigned)nb), dim3(SCAN_TPB), 0, s>>>(in, n, bsum, out);
}

#endif
