// sift.hip — FeatureProc::DetectFeature (R/FeatureProc/FeatureProc.cpp:14-75,103-112, call site R/Processor/Processor.cpp:562): SIFT
// keys and descriptors for ALL lists (frame x view rasters) of a call.  The rules are those of include/mvs.h (mvs_sift_detect;
// recalled from SiftGPU and Lowe's method, not verified against SiftGPU's source).  The list index is a grid dimension of every
// kernel; lists go through in chunks so that the pyramid scratch stays under SIFT_SCRATCH_BYTES.
//
//   k_sift_base   : rules 1-2, bytes -> grey float32 with the margins zeroed, doubled for first_octave = -1
//   k_sift_blur   : rule 3, the hot path.  A workgroup stages one tile of a level with a halo of r on every side in LDS (borders
//                   replicated on the way in), filters its rows into a second LDS array and the columns of that into HBM: a level
//                   is read once and written once.  Taps come from the host (double, rounded to float32), staged in LDS.
//   k_sift_down   : rule 4, level S at the even pixels -> level 0 of the next octave
//   k_sift_detect : rules 5-6 over EVERY (octave, level, pixel) of a list, flattened in the output order of rule 9.  It reads four
//                   Gaussian levels and stores no DoG.  First run: the keep flag of every item and the survivors per workgroup;
//                   CompactTail (compact.hip; the counts are list-major) turns them into places; second run: the survivors refine
//                   again (the same sift_refine body) and write their record at base + wg_rank — no atomic counter anywhere.
//   k_sift_orient : rule 7, a wave per candidate, the 36-bin histogram in LDS as 64-bit integers (a vote is quantised to 2^-24
//                   first, so the sum does not depend on the order of the lanes), smoothing and peaks in registers
//   k_sift_desc   : rule 8, a wave per final key, the 128 bins in LDS the same way
// Between orientation and descriptor the host clips every list to max_features (a few thousand counts) and fills key_offsets.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include "sift_rules.h"
#include "../../include/mvs_test.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int SF_TPB = 256;
constexpr int SF_WAVES = SF_TPB / 64;
static_assert(SF_TPB == COMPACT_TPB, "k_sift_detect counts and places per workgroup of the shared tail");
constexpr size_t SIFT_SCRATCH_BYTES = (size_t)512 << 20;      // pyramid, base, keep flags, workgroup counts of one chunk of lists (mvs.h states it)
constexpr int SF_MAX_CHUNK = 32768;                           // lists per chunk: the list index is blockIdx.y
constexpr float SF_Q = 16777216.0f;                           // votes are accumulated in units of 2^-24
constexpr float SF_2PI = 6.28318530717958647692f;
constexpr float SF_BIN36 = (float)(36.0 / 6.28318530717958647692);
constexpr float SF_BIN8 = (float)(8.0 / 6.28318530717958647692);
constexpr float SF_ORI_STEP = (float)(6.28318530717958647692 / 36.0);
constexpr int SF_SMOOTH = 6;                                  // box-smoothing passes of the orientation histogram

struct SiftDev {
    float* pyr;                               // the chunk's pyramid
    int64_t oct_off[SIFT_MAX_OCT];            // floats in front of octave o; inside: [list][level][H][W]
    int64_t item_off[SIFT_MAX_OCT + 1];       // (octave, level 1..S, y, x) flattened: items in front of octave o
    int32_t W[SIFT_MAX_OCT], H[SIFT_MAX_OCT];
    float step[SIFT_MAX_OCT];
    int32_t n_oct, S, w, h;
    float T, edge, sigma0;
    float left, right, top, bottom;           // the key filter of FeatureProc.cpp:53-57
};

__device__ inline const float* sf_level(const SiftDev& d, int list, int o, int l) {
    const int64_t npx = (int64_t)d.W[o] * d.H[o];
    return d.pyr + d.oct_off[o] + ((int64_t)list * (d.S + 3) + l) * npx;
}

// rules 1-2
struct SfMargins { int32_t left, right, top, bottom; };      // zeroed: x < left, x >= right, y < top, y >= bottom
__device__ inline float sf_grey(const uint8_t* __restrict__ img, int w, int x, int y, const SfMargins& m) {
    if (x < m.left || x >= m.right || y < m.top || y >= m.bottom) return 0.0f;
    return (float)grey8(img + 3 * ((int64_t)y * w + x)) / 255.0f;
}
__device__ inline float sf_rowval(const uint8_t* __restrict__ img, int w, int X, int y, const SfMargins& m) {
    const int x = X >> 1;
    const float a = sf_grey(img, w, x, y, m);
    if (!(X & 1)) return a;
    return 0.5f * (a + sf_grey(img, w, min(x + 1, w - 1), y, m));
}
__global__ __launch_bounds__(SF_TPB) void k_sift_base(const uint8_t* __restrict__ imgs, int w, int h, SfMargins m, int up, float* __restrict__ U) {
    const int W0 = up ? 2 * w : w, H0 = up ? 2 * h : h;
    const int64_t npx = (int64_t)W0 * H0, r = (int64_t)blockIdx.x * SF_TPB + threadIdx.x;
    if (r >= npx) return;
    const uint8_t* img = imgs + (int64_t)blockIdx.y * w * h * 3;
    const int X = (int)(r % W0), Y = (int)(r / W0);
    float v;
    if (!up) v = sf_grey(img, w, X, Y, m);
    else {
        const int y = Y >> 1;
        v = sf_rowval(img, w, X, y, m);
        if (Y & 1) v = 0.5f * (v + sf_rowval(img, w, X, min(y + 1, h - 1), m));
    }
    U[(int64_t)blockIdx.y * npx + r] = v;
}

// rule 3.  Tile T x T outputs, staged (T + 2r)^2 inputs; dynamic LDS: taps[2r + 1 rounded up to 4] | in[(T+2r)^2] | mid[(T+2r) * T]
__global__ __launch_bounds__(SF_TPB) void k_sift_blur(const float* __restrict__ src, int64_t src_stride, float* __restrict__ dst, int64_t dst_stride,
                                                      int W, int H, const float* __restrict__ taps, int r, int T, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int nt = 2 * r + 1, IW = T + 2 * r;
    float* s_k = s_mem;
    float* s_in = s_mem + ((nt + 3) & ~3);
    float* s_mid = s_in + IW * IW;
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % tiles_x) * T, y0 = (int)(blockIdx.x / tiles_x) * T;
    const float* S = src + (int64_t)blockIdx.y * src_stride;
    for (int i = tid; i < nt; i += SF_TPB) s_k[i] = taps[i];
    for (int i = tid; i < IW * IW; i += SF_TPB) {
        const int ty = i / IW, tx = i - ty * IW;
        const int gy = min(max(y0 - r + ty, 0), H - 1), gx = min(max(x0 - r + tx, 0), W - 1);       // replicate
        s_in[i] = S[(int64_t)gy * W + gx];
    }
    __syncthreads();
    for (int i = tid; i < IW * T; i += SF_TPB) {
        const int ty = i / T, tx = i - ty * T;
        const float* p = s_in + ty * IW + tx;
        float acc = s_k[0] * p[0];
        for (int k = 1; k < nt; ++k) acc = acc + s_k[k] * p[k];
        s_mid[i] = acc;
    }
    __syncthreads();
    float* D = dst + (int64_t)blockIdx.y * dst_stride;
    for (int i = tid; i < T * T; i += SF_TPB) {
        const int ty = i / T, tx = i - ty * T;
        if (x0 + tx >= W || y0 + ty >= H) continue;
        const float* p = s_mid + ty * T + tx;
        float acc = s_k[0] * p[0];
        for (int k = 1; k < nt; ++k) acc = acc + s_k[k] * p[k * T];
        D[(int64_t)(y0 + ty) * W + (x0 + tx)] = acc;
    }
}

__global__ __launch_bounds__(SF_TPB) void k_sift_down(const float* __restrict__ src, int64_t src_stride, int Ws, float* __restrict__ dst,
                                                      int64_t dst_stride, int Wd, int Hd) {
    const int64_t r = (int64_t)blockIdx.x * SF_TPB + threadIdx.x;
    if (r >= (int64_t)Wd * Hd) return;
    const int x = (int)(r % Wd), y = (int)(r / Wd);
    dst[(int64_t)blockIdx.y * dst_stride + r] = src[(int64_t)blockIdx.y * src_stride + (int64_t)(2 * y) * Ws + 2 * x];
}

struct SfItem { int o, l, x, y; };
__device__ inline SfItem sf_item(const SiftDev& d, int64_t r) {
    int o = 0;
    while (o + 1 < d.n_oct && r >= d.item_off[o + 1]) ++o;
    const int64_t rem = r - d.item_off[o], npx = (int64_t)d.W[o] * d.H[o];
    const int pix = (int)(rem % npx);
    return SfItem{o, 1 + (int)(rem / npx), pix % d.W[o], pix / d.W[o]};
}

// rules 5-6 for one item -> kept?, the refined offsets
__device__ inline bool sf_test(const SiftDev& d, int list, const SfItem& it, SiftRefined* rf) {
    const int W = d.W[it.o], H = d.H[it.o];
    if (it.x < 1 || it.x > W - 2 || it.y < 1 || it.y > H - 2) return false;
    const int64_t npx = (int64_t)W * H;
    const float* g = sf_level(d, list, it.o, it.l - 1) + (int64_t)it.y * W + it.x;       // levels l-1 .. l+2 follow each other
    const float v = g[2 * npx] - g[npx];
    if (!(fabsf(v) > d.T)) return false;
    float D[3][3][3];
    bool above = true, below = true;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int64_t q = (int64_t)dy * W + dx;
                const float u = g[(s + 1) * npx + q] - g[s * npx + q];
                D[s][dy + 1][dx + 1] = u;
                if (s != 1 || dy != 0 || dx != 0) { above = above && v > u; below = below && v < u; }
            }
    if (!above && !below) return false;
    if (!sift_refine(D, d.T, d.edge, rf)) return false;
    const float x = (((float)it.x + rf->dx) + 0.5f) * d.step[it.o], y = (((float)it.y + rf->dy) + 0.5f) * d.step[it.o];
    return !(x < d.left || x > d.right || y < d.top || y > d.bottom);
}

// candidate record: ci[8] = {octave, level, xi, yi, list, 0, 0, 0}, cf[8] = {x, y, s, sigma_oct, dx, dy, 0, 0}
template <bool WRITE>
__global__ __launch_bounds__(SF_TPB) void k_sift_detect(SiftDev d, int64_t n_items, uint8_t* __restrict__ keep, int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ base, int32_t* __restrict__ ci, float* __restrict__ cf) {
    __shared__ int s_wsum[SF_WAVES];
    const int64_t r = (int64_t)blockIdx.x * SF_TPB + threadIdx.x;
    const int list = blockIdx.y;
    const int64_t slot = (int64_t)list * gridDim.x + blockIdx.x;
    bool f = false;
    SiftRefined rf = {0, 0, 0, 0};
    SfItem it = {0, 0, 0, 0};
    if (r < n_items && (!WRITE || keep[(int64_t)list * n_items + r])) {
        it = sf_item(d, r);
        f = sf_test(d, list, it, &rf);
    }
    if (!WRITE && r < n_items) keep[(int64_t)list * n_items + r] = f ? 1 : 0;
    const WgRank k = wg_rank<SF_WAVES>(f, s_wsum);
    if (!WRITE) { if (threadIdx.x == 0) cnt[slot] = k.total; return; }
    if (!f) return;
    const int64_t pos = (int64_t)base[slot] + k.rank;
    const float step = d.step[it.o];
    const float so = d.sigma0 * exp2f(((float)it.l + rf.ds) / (float)d.S);
    int32_t* I = ci + 8 * pos;
    float* F = cf + 8 * pos;
    I[0] = it.o; I[1] = it.l; I[2] = it.x; I[3] = it.y; I[4] = list; I[5] = 0; I[6] = 0; I[7] = 0;
    F[0] = (((float)it.x + rf.dx) + 0.5f) * step; F[1] = (((float)it.y + rf.dy) + 0.5f) * step; F[2] = so * step; F[3] = so;
    F[4] = rf.dx; F[5] = rf.dy; F[6] = 0.0f; F[7] = 0.0f;
}

__device__ inline unsigned long long sf_quant(float v) { return (unsigned long long)(v * SF_Q + 0.5f); }

// rule 7: a wave per candidate; ori[c][4] and n_or[c]
__global__ __launch_bounds__(SF_TPB) void k_sift_orient(SiftDev d, int n_cand, const int32_t* __restrict__ ci, const float* __restrict__ cf,
                                                        int max_orient, int32_t* __restrict__ n_or, float* __restrict__ ori) {
    __shared__ unsigned long long s_hist[SF_WAVES][36];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * SF_WAVES + wv;
    const bool active = c < n_cand;                           // a whole wave; it still meets the barriers
    if (lane < 36) s_hist[wv][lane] = 0ull;
    __syncthreads();
    if (active) {
        const int32_t* I = ci + 8 * (int64_t)c;
        const float* F = cf + 8 * (int64_t)c;
        const int o = I[0], l = I[1], xi = I[2], yi = I[3], W = d.W[o], H = d.H[o];
        const float sw = 1.5f * F[3], ddx = F[4], ddy = F[5];
        const int R = (int)(3.0f * sw + 0.5f), side = 2 * R + 1;
        const float den = 2.0f * sw * sw;
        const float* g = sf_level(d, I[4], o, l);
        for (int i = lane; i < side * side; i += 64) {
            const int dy = i / side - R, dx = i % side - R, px = xi + dx, py = yi + dy;
            if (px < 1 || px > W - 2 || py < 1 || py > H - 2) continue;
            const float* p = g + (int64_t)py * W + px;
            const float gx = p[1] - p[-1], gy = p[W] - p[-W];
            const float fx = (float)dx - ddx, fy = (float)dy - ddy;
            const float v = expf(-(fx * fx + fy * fy) / den) * sqrtf(gx * gx + gy * gy);
            float ang = atan2f(gy, gx);
            if (ang < 0.0f) ang += SF_2PI;
            const float fb = ang * SF_BIN36 - 0.5f;
            const int b0 = (int)floorf(fb);
            const float rb = fb - (float)b0;
            atomicAdd(&s_hist[wv][(b0 + 36) % 36], sf_quant((1.0f - rb) * v));
            atomicAdd(&s_hist[wv][(b0 + 37) % 36], sf_quant(rb * v));
        }
    }
    __syncthreads();
    if (!active) return;
    const int b = lane < 36 ? lane : 0;
    float hcur = (float)s_hist[wv][b] / SF_Q;
    const int bm = (b + 35) % 36, bp = (b + 1) % 36;
    for (int k = 0; k < SF_SMOOTH; ++k) {
        const float hm = __shfl(hcur, bm, 64), hp = __shfl(hcur, bp, 64);
        hcur = ((hm + hcur) + hp) / 3.0f;
    }
    const float hm = __shfl(hcur, bm, 64), hp = __shfl(hcur, bp, 64);
    float mx = lane < 36 ? hcur : 0.0f;
#pragma unroll
    for (int q = 1; q < 64; q <<= 1) mx = fmaxf(mx, __shfl_xor(mx, q, 64));
    bool peak = lane < 36 && mx > 0.0f && hcur > hm && hcur > hp && hcur >= 0.8f * mx;
    int n = 0;
    for (int j = 0; j < max_orient; ++j) {
        // the largest remaining peak, the lowest bin among equals
        float bv = peak ? hcur : -1.0f;
        int bb = peak ? lane : 64;
#pragma unroll
        for (int q = 1; q < 64; q <<= 1) {
            const float ov = __shfl_xor(bv, q, 64);
            const int ob = __shfl_xor(bb, q, 64);
            if (ov > bv || (ov == bv && ob < bb)) { bv = ov; bb = ob; }
        }
        if (bb >= 36) break;
        if (lane == bb) {
            const float dd = 0.5f * (hm - hp) / ((hm - 2.0f * hcur) + hp);
            float th = (((float)lane + dd) + 0.5f) * SF_ORI_STEP;
            if (th < 0.0f) th += SF_2PI;
            if (th >= SF_2PI) th -= SF_2PI;
            ori[4 * (int64_t)c + j] = th;
            peak = false;
        }
        ++n;
    }
    if (lane == 0) n_or[c] = n;
}

// rule 8: a wave per final key k = (candidate, orientation index) of kmap; keys / descs row out0 + k
__global__ __launch_bounds__(SF_TPB) void k_sift_desc(SiftDev d, int n_keys, const int2* __restrict__ kmap, const int32_t* __restrict__ ci,
                                                      const float* __restrict__ cf, const float* __restrict__ ori, float* __restrict__ keys,
                                                      float* __restrict__ descs) {
    __shared__ unsigned long long s_q[SF_WAVES][128];
    __shared__ float s_f[SF_WAVES][128];
    __shared__ float s_n[SF_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.x * SF_WAVES + wv;
    const bool active = k < n_keys;
    s_q[wv][lane] = 0ull;
    s_q[wv][lane + 64] = 0ull;
    __syncthreads();
    float th = 0.0f;
    int c = 0;
    if (active) {
        c = kmap[k].x;
        th = ori[4 * (int64_t)c + kmap[k].y];
        const int32_t* I = ci + 8 * (int64_t)c;
        const float* F = cf + 8 * (int64_t)c;
        const int o = I[0], l = I[1], xi = I[2], yi = I[3], W = d.W[o], H = d.H[o];
        const float m = 3.0f * F[3], kdx = F[4], kdy = F[5];
        const float ct = cosf(th), st = sinf(th);
        const int R = (int)(m * 3.5355339f) + 2, side = 2 * R + 1;
        const float* g = sf_level(d, I[4], o, l);
        for (int i = lane; i < side * side; i += 64) {
            const int dy = i / side - R, dx = i % side - R, px = xi + dx, py = yi + dy;
            if (px < 1 || px > W - 2 || py < 1 || py > H - 2) continue;
            const float ddx = (float)dx - kdx, ddy = (float)dy - kdy;
            const float nx = (ct * ddx + st * ddy) / m, ny = (ct * ddy - st * ddx) / m;
            const float fx = nx + 1.5f, fy = ny + 1.5f;
            if (!(fx > -1.0f && fx < 4.0f && fy > -1.0f && fy < 4.0f)) continue;
            const float* p = g + (int64_t)py * W + px;
            const float gx = 0.5f * (p[1] - p[-1]), gy = 0.5f * (p[W] - p[-W]);
            const float v = sqrtf(gx * gx + gy * gy) * expf(-(nx * nx + ny * ny) / 8.0f);
            float dth = atan2f(gy, gx) - th;
            if (dth < 0.0f) dth += SF_2PI;
            if (dth < 0.0f) dth += SF_2PI;
            if (dth >= SF_2PI) dth -= SF_2PI;
            const float ft = dth * SF_BIN8;
            const int ix = (int)floorf(fx), iy = (int)floorf(fy), it = (int)ft;
            const float rx = fx - (float)ix, ry = fy - (float)iy, rt = ft - (float)it;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int cx = ix + a, cy = iy + b;
                    if (cx < 0 || cx > 3 || cy < 0 || cy > 3) continue;
                    const float wxy = (v * (a ? rx : 1.0f - rx)) * (b ? ry : 1.0f - ry);
                    atomicAdd(&s_q[wv][(cy * 4 + cx) * 8 + (it & 7)], sf_quant(wxy * (1.0f - rt)));
                    atomicAdd(&s_q[wv][(cy * 4 + cx) * 8 + ((it + 1) & 7)], sf_quant(wxy * rt));
                }
        }
    }
    __syncthreads();
    float d0 = (float)s_q[wv][lane] / SF_Q, d1 = (float)s_q[wv][lane + 64] / SF_Q;
    for (int pass = 0; pass < 2; ++pass) {                    // L2 normalise, clamp at 0.2, normalise again
        s_f[wv][lane] = d0;
        s_f[wv][lane + 64] = d1;
        __syncthreads();
        if (lane == 0) {
            double sum = 0.0;
            for (int i = 0; i < 128; ++i) sum += (double)s_f[wv][i] * (double)s_f[wv][i];
            s_n[wv] = (float)sqrt(sum);
        }
        __syncthreads();
        const float nrm = s_n[wv];
        if (nrm > 0.0f) { d0 = d0 / nrm; d1 = d1 / nrm; }
        if (pass == 0) { d0 = fminf(d0, 0.2f); d1 = fminf(d1, 0.2f); }
    }
    if (!active) return;
    descs[128 * (int64_t)k + lane] = d0;
    descs[128 * (int64_t)k + lane + 64] = d1;
    if (lane == 0) {
        const float* F = cf + 8 * (int64_t)c;
        *(float4*)(keys + 4 * (int64_t)k) = make_float4(F[0], F[1], F[2], th);
    }
}

// ------------------------------------------------------------------ host ----
struct SiftPlan {
    SiftDev d;
    int W0, H0, up, r[SIFT_MAX_LEVELS], tap_off[SIFT_MAX_LEVELS];
    std::vector<float> taps;                  // level l's taps at tap_off[l]; level 0's = the base blur of the first octave
    SfMargins zero;
    int64_t n_items, pyr_floats_per_list;
    size_t bytes_per_list;
};

bool finite_f(float x) { return std::isfinite(x); }

int check_sift(const char* fn, int32_t n_lists, int32_t w, int32_t h, const void* imgs, const mvs_sift_params* p, const int64_t* key_offsets,
               const void* keys, const void* descs, int64_t capacity, SiftPlan* pl) {
    if (!imgs || !p || !key_offsets || !keys || !descs) return bad(fn, "a pointer is NULL");
    if (n_lists < 1) return bad(fn, "need n_lists >= 1");
    if (w < 8 || h < 8 || w > 65535 || h > 65535) return bad(fn, "need 8 <= w, h <= 65535");
    if (p->first_octave != -1 && p->first_octave != 0) return bad(fn, "first_octave must be -1 or 0");
    if (p->dog_levels < 1 || p->dog_levels > 5) return bad(fn, "dog_levels must be in 1..5");
    if (p->max_orient < 1 || p->max_orient > 4) return bad(fn, "max_orient must be in 1..4");
    if (p->max_features < 1) return bad(fn, "need max_features >= 1");
    if (capacity < 0) return bad(fn, "capacity is negative");
    if (!finite_f(p->dog_threshold) || !finite_f(p->edge_threshold) || !finite_f(p->sigma0) || !finite_f(p->sigma_in))
        return bad(fn, "a float parameter is not finite");
    const double mr[4] = {p->hl, p->hr, p->vl, p->vr};
    for (double m : mr)
        if (!(m >= 0.0 && m < 1.0)) return bad(fn, "a margin ratio is outside [0, 1)");
    if (!(p->hl + p->hr < 1.0) || !(p->vl + p->vr < 1.0)) return bad(fn, "hl + hr and vl + vr must stay below 1");
    if (p->dog_threshold < 0.0f || !(p->edge_threshold > 0.0f) || !(p->sigma0 > 0.0f) || p->sigma_in < 0.0f)
        return bad(fn, "need dog_threshold >= 0, edge_threshold > 0, sigma0 > 0, sigma_in >= 0");
    const int S = p->dog_levels;
    SiftDev& d = pl->d;
    std::memset(&d, 0, sizeof d);
    pl->up = p->first_octave < 0;
    pl->W0 = pl->up ? 2 * w : w;
    pl->H0 = pl->up ? 2 * h : h;
    pl->taps.clear();
    for (int l = 0; l < S + 3; ++l) {
        std::vector<float> t;
        const int r = sift_taps(sift_level_sigma(l, S, p->sigma0, p->sigma_in, p->first_octave), t);
        if (r < 1 || r > SIFT_RMAX) return bad(fn, "sigma0 / sigma_in / dog_levels give a blur that is not positive or whose radius exceeds 51");
        pl->r[l] = r;
        pl->tap_off[l] = (int)pl->taps.size();
        pl->taps.insert(pl->taps.end(), t.begin(), t.end());
    }
    d.n_oct = sift_octaves(pl->W0, pl->H0);
    d.S = S; d.w = w; d.h = h;
    d.T = p->dog_threshold / (float)S;
    d.edge = p->edge_threshold;
    d.sigma0 = p->sigma0;
    const int left = cvt_i32((double)w * p->hl), right = cvt_i32((double)w * p->hr), top = cvt_i32((double)h * p->vl), bottom = cvt_i32((double)h * p->vr);
    pl->zero = SfMargins{left, w - right, top, h - bottom};
    d.left = (float)left; d.right = (float)(w - right); d.top = (float)top; d.bottom = (float)(h - bottom);
    int W = pl->W0, H = pl->H0;
    int64_t items = 0, floats = 0;
    for (int o = 0; o < d.n_oct; ++o) {
        d.W[o] = W; d.H[o] = H;
        d.step[o] = pl->up ? (o == 0 ? 0.5f : (float)(1 << (o - 1))) : (float)(1 << o);
        d.item_off[o] = items;
        items += (int64_t)S * W * H;
        floats += (int64_t)(S + 3) * W * H;
        W /= 2; H /= 2;
    }
    d.item_off[d.n_oct] = items;
    if (items >= 0x7fffffffLL) return bad(fn, "the image is too large: 2^31 - 1 or more (octave, level, pixel) items per list");
    pl->n_items = items;
    pl->pyr_floats_per_list = floats;
    // pyramid, base image, one keep flag per item, and the count and place of every workgroup of the compaction
    pl->bytes_per_list = sizeof(float) * ((size_t)floats + (size_t)pl->W0 * pl->H0) + (size_t)items + 2 * sizeof(int32_t) * (size_t)((items + SF_TPB - 1) / SF_TPB);
    return MVS_OK;
}

struct SiftHook {
    int oct = -1, level = -1;                 // >= 0: copy this Gaussian level of list 0 to level_out
    float* level_out = nullptr;
    int64_t* cand_off = nullptr;              // != NULL: the stage-6 candidates of every list
    int32_t* ci = nullptr; float* cf = nullptr;
    int64_t cand_cap = 0;
};

void launch_blur(const SiftPlan& pl, int l, const float* src, int64_t sstride, float* dst, int64_t dstride, int W, int H, const float* taps_dev, int nl,
                 hipStream_t s) {
    const int r = pl.r[l], T = r <= 40 ? 32 : 16, IW = T + 2 * r, nt = 2 * r + 1;
    const int tx = (W + T - 1) / T, ty = (H + T - 1) / T;
    const size_t lds = sizeof(float) * ((size_t)((nt + 3) & ~3) + (size_t)IW * IW + (size_t)IW * T);       // <= 64 KiB for r <= 51
    k_sift_blur<<<dim3((unsigned)(tx * ty), (unsigned)nl), dim3(SF_TPB), lds, s>>>(src, sstride, dst, dstride, W, H, taps_dev + pl.tap_off[l], r, T, tx);
}

// imgs, keys and descs in HBM; key_offsets on the host.  Returns with s synchronised.
int sift_core(const char* fn, int n_lists, int w, int h, const uint8_t* imgs, const mvs_sift_params* p, SiftPlan& pl, int64_t* key_offsets, float* keys,
              float* descs, int64_t capacity, const SiftHook* hook, hipStream_t s) {
    const int S = pl.d.S, n_oct = pl.d.n_oct;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_lists, (size_t)SF_MAX_CHUNK, SIFT_SCRATCH_BYTES / pl.bytes_per_list}));
    const int64_t npx0 = (int64_t)pl.W0 * pl.H0, n_items = pl.n_items;
    const int nb = (int)((n_items + SF_TPB - 1) / SF_TPB);
    if ((int64_t)nb * chunk >= 0x7fffffffLL) return bad(fn, "too many workgroups in one chunk");
    Scratch pyr, U, keep, taps;
    CompactTail ct;
    int rc;
    if ((rc = pyr.alloc(sizeof(float) * (size_t)pl.pyr_floats_per_list * chunk, s)) || (rc = U.alloc(sizeof(float) * (size_t)npx0 * chunk, s)) ||
        (rc = keep.alloc((size_t)n_items * chunk, s)) || (rc = ct.alloc((size_t)nb * chunk, (size_t)chunk, s)) ||
        (rc = up_async(taps, pl.taps.data(), pl.taps.size(), s))) return rc;
    SiftDev d = pl.d;
    d.pyr = pyr.as<float>();
    int64_t off = 0;
    for (int o = 0; o < n_oct; ++o) {
        d.oct_off[o] = off;
        off += (int64_t)chunk * (S + 3) * d.W[o] * d.H[o];
    }
    key_offsets[0] = 0;
    if (hook && hook->cand_off) hook->cand_off[0] = 0;
    int64_t total = 0, cand_total = 0;
    bool fits = true;
    for (int l0 = 0; l0 < n_lists; l0 += chunk) {
        const int nl = std::min(chunk, n_lists - l0);
        k_sift_base<<<dim3((unsigned)((npx0 + SF_TPB - 1) / SF_TPB), (unsigned)nl), dim3(SF_TPB), 0, s>>>(imgs + (int64_t)l0 * w * h * 3, w, h, pl.zero, pl.up,
                                                                                                       U.as<float>());
        for (int o = 0; o < n_oct; ++o) {
            const int W = d.W[o], H = d.H[o];
            const int64_t npx = (int64_t)W * H, lstride = (int64_t)(S + 3) * npx;
            float* lv = d.pyr + d.oct_off[o];
            if (o == 0) launch_blur(pl, 0, U.as<float>(), npx0, lv, lstride, W, H, taps.as<float>(), nl, s);
            else {
                const int64_t pstride = (int64_t)(S + 3) * d.W[o - 1] * d.H[o - 1];
                k_sift_down<<<dim3((unsigned)((npx + SF_TPB - 1) / SF_TPB), (unsigned)nl), dim3(SF_TPB), 0, s>>>(
                    d.pyr + d.oct_off[o - 1] + (int64_t)S * d.W[o - 1] * d.H[o - 1], pstride, d.W[o - 1], lv, lstride, W, H);
            }
            for (int l = 1; l < S + 3; ++l) launch_blur(pl, l, lv + (l - 1) * npx, lstride, lv + l * npx, lstride, W, H, taps.as<float>(), nl, s);
        }
        HIPCHK(hipGetLastError());
        if (hook && hook->level_out && l0 == 0) {
            const int64_t npx = (int64_t)d.W[hook->oct] * d.H[hook->oct];
            HIPCHK(hipMemcpyAsync(hook->level_out, d.pyr + d.oct_off[hook->oct] + hook->level * npx, sizeof(float) * (size_t)npx, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            return MVS_OK;
        }
        k_sift_detect<false><<<dim3((unsigned)nb, (unsigned)nl), dim3(SF_TPB), 0, s>>>(d, n_items, keep.as<uint8_t>(), ct.cnt.as<int32_t>(), nullptr, nullptr, nullptr);
        ct.strided(nb * nl, nullptr, nl, nb, s);                  // where every list's candidates start: list l's workgroups start at l * nb
        HIPCHK(hipGetLastError());
        std::vector<int64_t> coff((size_t)nl + 1);
        HIPCHK(hipMemcpyAsync(coff.data(), ct.off.p, sizeof(int64_t) * ((size_t)nl + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int n_cand = (int)coff[(size_t)nl];
        std::vector<int32_t> n_or((size_t)n_cand);
        Scratch ci, cf, dn_or, dori, dkmap;
        if (n_cand > 0) {
            if ((rc = ci.alloc(sizeof(int32_t) * 8 * (size_t)n_cand, s)) || (rc = cf.alloc(sizeof(float) * 8 * (size_t)n_cand, s)) ||
                (rc = dn_or.alloc(sizeof(int32_t) * (size_t)n_cand, s)) || (rc = dori.alloc(sizeof(float) * 4 * (size_t)n_cand, s))) return rc;
            k_sift_detect<true><<<dim3((unsigned)nb, (unsigned)nl), dim3(SF_TPB), 0, s>>>(d, n_items, keep.as<uint8_t>(), nullptr, ct.base.as<int32_t>(), ci.as<int32_t>(),
                                                                                          cf.as<float>());
            HIPCHK(hipGetLastError());
        }
        if (hook && hook->cand_off) {
            for (int l = 0; l < nl; ++l) hook->cand_off[l0 + l + 1] = cand_total + coff[(size_t)l + 1];
            if (cand_total + n_cand <= hook->cand_cap && n_cand > 0) {
                std::vector<int32_t> hi(8 * (size_t)n_cand);
                std::vector<float> hf(8 * (size_t)n_cand);
                HIPCHK(hipMemcpyAsync(hi.data(), ci.p, sizeof(int32_t) * hi.size(), hipMemcpyDeviceToHost, s));
                HIPCHK(hipMemcpyAsync(hf.data(), cf.p, sizeof(float) * hf.size(), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                for (int c = 0; c < n_cand; ++c) {
                    std::memcpy(hook->ci + 4 * (cand_total + c), &hi[8 * (size_t)c], 4 * sizeof(int32_t));
                    std::memcpy(hook->cf + 3 * (cand_total + c), &hf[8 * (size_t)c], 3 * sizeof(float));
                }
            }
            cand_total += n_cand;
            continue;
        }
        if (n_cand > 0) {
            k_sift_orient<<<dim3((unsigned)((n_cand + SF_WAVES - 1) / SF_WAVES)), dim3(SF_TPB), 0, s>>>(d, n_cand, ci.as<int32_t>(), cf.as<float>(), p->max_orient,
                                                                                                       dn_or.as<int32_t>(), dori.as<float>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(n_or.data(), dn_or.p, sizeof(int32_t) * (size_t)n_cand, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        // rule 9: the first max_features keys of every list, candidates in order, a candidate's orientations in theirs
        std::vector<int2> kmap;
        for (int l = 0; l < nl; ++l) {
            int64_t nk = 0;
            for (int c = (int)coff[(size_t)l]; c < coff[(size_t)l + 1] && nk < p->max_features; ++c)
                for (int j = 0; j < n_or[(size_t)c] && nk < p->max_features; ++j, ++nk) kmap.push_back(make_int2(c, j));
            key_offsets[l0 + l + 1] = key_offsets[l0 + l] + nk;
        }
        const int64_t nk = (int64_t)kmap.size();
        if (nk >= 0x7fffffffLL) return bad(fn, "2^31 - 1 or more keys in one chunk");
        fits = fits && total + nk <= capacity;
        if (fits && nk > 0) {
            if ((rc = up_async(dkmap, kmap.data(), (size_t)nk, s))) return rc;
            k_sift_desc<<<dim3((unsigned)((nk + SF_WAVES - 1) / SF_WAVES)), dim3(SF_TPB), 0, s>>>(d, (int)nk, dkmap.as<int2>(), ci.as<int32_t>(), cf.as<float>(),
                                                                                                 dori.as<float>(), keys + 4 * total, descs + 128 * total);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));          // kmap and this chunk's tables are released below
        }
        total += nk;
    }
    HIPCHK(hipStreamSynchronize(s));
    if (!fits) return bad(fn, "capacity is below the number of keys (key_offsets holds it)");
    return MVS_OK;
}

}  // namespace

extern "C" {

void mvs_sift_default_params(mvs_sift_params* p) {
    if (!p) return;
    p->first_octave = -1; p->dog_levels = 3; p->max_orient = 2; p->max_features = 0x7fffffff;
    p->dog_threshold = 0.02f; p->edge_threshold = 10.0f; p->sigma0 = 1.6f; p->sigma_in = 0.5f;
    p->hl = p->hr = p->vl = p->vr = 0.0;
}

int mvs_sift_detect_dev(int32_t n_lists, int32_t w, int32_t h, const uint8_t* imgs_dev, const mvs_sift_params* p, int64_t* key_offsets, float* keys_dev,
                        float* descs_dev, int64_t capacity, void* hip_stream) {
    MVS_TRACE();
    SiftPlan pl;
    int rc = check_sift(__func__, n_lists, w, h, imgs_dev, p, key_offsets, keys_dev, descs_dev, capacity, &pl);
    if (rc) return rc;
    if (((uintptr_t)keys_dev & 15) || ((uintptr_t)descs_dev & 15)) return bad(__func__, "keys_dev and descs_dev must be 16-byte aligned");
    if ((rc = need_device())) return rc;
    return sift_core(__func__, n_lists, w, h, imgs_dev, p, pl, key_offsets, keys_dev, descs_dev, capacity, nullptr, (hipStream_t)hip_stream);
}

int mvs_sift_detect(int32_t n_lists, int32_t w, int32_t h, const uint8_t* imgs, const mvs_sift_params* p, int64_t* key_offsets, float* keys, float* descs,
                    int64_t capacity) {
    MVS_TRACE();
    SiftPlan pl;
    int rc = check_sift(__func__, n_lists, w, h, imgs, p, key_offsets, keys, descs, capacity, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    Scratch di, dk, dd;
    if ((rc = up(di, imgs, (size_t)n_lists * w * h * 3)) || (rc = dk.alloc(sizeof(float) * 4 * (size_t)capacity)) ||
        (rc = dd.alloc(sizeof(float) * 128 * (size_t)capacity))) return rc;
    rc = sift_core(__func__, n_lists, w, h, di.as<uint8_t>(), p, pl, key_offsets, dk.as<float>(), dd.as<float>(), capacity, nullptr, nullptr);
    if (rc) return rc;
    const size_t total = (size_t)key_offsets[n_lists];
    if ((rc = down(keys, dk, 4 * total)) || (rc = down(descs, dd, 128 * total))) return rc;
    return MVS_OK;
}

int mvs_test_sift_level(int32_t w, int32_t h, const uint8_t* img, const mvs_sift_params* p, int32_t octave, int32_t level, float* out, int64_t out_floats,
                        int32_t* ow, int32_t* oh) {
    SiftPlan pl;
    int64_t koff[2];
    float dummy;
    int rc = check_sift(__func__, 1, w, h, img, p, koff, &dummy, &dummy, 0, &pl);
    if (rc) return rc;
    if (!out || !ow || !oh) return bad(__func__, "an output is NULL");
    if (octave < 0 || octave >= pl.d.n_oct || level < 0 || level >= pl.d.S + 3) return bad(__func__, "no such octave or level");
    *ow = pl.d.W[octave]; *oh = pl.d.H[octave];
    if (out_floats < (int64_t)*ow * *oh) return bad(__func__, "out is too small (ow, oh hold the size)");
    if ((rc = need_device())) return rc;
    Scratch di;
    if ((rc = up(di, img, (size_t)w * h * 3))) return rc;
    SiftHook hook;
    hook.oct = octave; hook.level = level; hook.level_out = out;
    return sift_core(__func__, 1, w, h, di.as<uint8_t>(), p, pl, koff, nullptr, nullptr, 0, &hook, nullptr);
}

int mvs_test_sift_candidates(int32_t n_lists, int32_t w, int32_t h, const uint8_t* imgs, const mvs_sift_params* p, int64_t* cand_offsets, int32_t* ci,
                             float* cf, int64_t capacity) {
    SiftPlan pl;
    int rc = check_sift(__func__, n_lists, w, h, imgs, p, cand_offsets, ci, cf, capacity, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    Scratch di;
    if ((rc = up(di, imgs, (size_t)n_lists * w * h * 3))) return rc;
    std::vector<int64_t> koff((size_t)n_lists + 1);
    SiftHook hook;
    hook.cand_off = cand_offsets; hook.ci = ci; hook.cf = cf; hook.cand_cap = capacity;
    if ((rc = sift_core(__func__, n_lists, w, h, di.as<uint8_t>(), p, pl, koff.data(), nullptr, nullptr, 0, &hook, nullptr))) return rc;
    if (cand_offsets[n_lists] > capacity) return bad(__func__, "capacity is below the number of candidates (cand_offsets holds it)");
    return MVS_OK;
}

}  // extern "C"

const void* mvs_tu_probe_sift() { return (const void*)k_sift_blur; }
