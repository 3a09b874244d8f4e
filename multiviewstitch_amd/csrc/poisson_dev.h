// poisson_dev.h — the device helpers that poisson.hip and poisson_band.hip share: the fixed-order folds of a workgroup, whose order is
// part of the result's bytes, and what the extraction of rules 10-12 and 30-31 (poisson_surface.h) decides per item.  One workgroup
// size, PN_TPB, for the kernels of both files.
#ifndef MVS_POISSON_DEV_H_
#define MVS_POISSON_DEV_H_
#ifdef __HIPCC__
#include "poisson_rules.h"

constexpr int PN_TPB = 256, PN_WAVES = PN_TPB / 64;

// v folded over the workgroup by op (tid: the thread's linear index; s_part: WAVES entries of LDS that nothing else uses), in a fixed
// order: shuffles inside a wave, then zero op wave 0 op wave 1 ... in thread 0, the only thread the result is valid in
template <int WAVES, class T, class Op>
__device__ inline T wg_fold(T v, T zero, T* s_part, int tid, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o, 64));
    if ((tid & 63) == 0) s_part[tid >> 6] = v;
    __syncthreads();
    T t = zero;
    if (tid == 0)
        for (int q = 0; q < WAVES; ++q) t = op(t, s_part[q]);
    return t;
}
struct FoldAdd { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct FoldMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct FoldMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
// the sum of a double: its order is part of the result's bytes
template <int WAVES>
__device__ inline double wg_sum(double v, double* s_part, int tid) { return wg_fold<WAVES>(v, 0.0, s_part, tid, FoldAdd()); }

// the sum of n partials by a workgroup of PN_TPB threads: thread t takes t, t + 256, ... in ascending order, then wg_sum; valid in thread 0
__device__ inline double wg_sum_partials(const double* __restrict__ part, int n, double* s_part) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += PN_TPB) acc += part[i];
    return wg_sum<PN_WAVES>(acc, s_part, threadIdx.x);
}
// ... and the same number in every thread of the workgroup, through *s_out
__device__ inline double wg_sum_partials_all(const double* __restrict__ part, int n, double* s_part, double* s_out) {
    const double t = wg_sum_partials(part, n, s_part);
    if (threadIdx.x == 0) *s_out = t;
    __syncthreads();
    return *s_out;
}

// the number of the vertex on edge item r (a set flag): the survivors of the workgroups before its own, then popcounts
__device__ inline int32_t pn_vertex_index(const unsigned long long* __restrict__ words, const int32_t* __restrict__ base, int64_t r) {
    const int64_t blk = r >> 8, w = r >> 6;
    int32_t acc = base[blk];
    for (int64_t q = blk * PN_WAVES; q < w; ++q) acc += __popcll(words[q]);
    return acc + __popcll(words[w] & ((1ull << (r & 63)) - 1ull));
}

__device__ inline void pn_node_pos(const PnGrid& g, int ix, int iy, int iz, double* p) {
    p[0] = g.o[0] + g.h * (double)ix; p[1] = g.o[1] + g.h * (double)iy; p[2] = g.o[2] + g.h * (double)iz;
}

// face item r = (cube item * 6 + tetrahedron) * 2 + slot: the inside bits of the tetrahedron's corners, or -1 when the slot is empty
__device__ inline int pn_face_item(const uint8_t* __restrict__ mask, int64_t r, int64_t items) {
    if (r >= items) return -1;
    const int cm = mask[r / 12];
    if (cm == 0 || cm == 255) return -1;
    const int k = (int)(r % 12) >> 1, slot = (int)(r & 1);
    int in = 0;
    for (int i = 0; i < 4; ++i) in |= (cm >> pn_tet_corner(k, i) & 1) << i;
    const int ni = __popc(in);
    return (slot == 0 ? ni >= 1 && ni <= 3 : ni == 2) ? in : -1;
}

#endif
#endif
