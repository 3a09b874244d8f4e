// views.hip — the head of Processor::CalcSimilarityTransformationSeq (R/Processor/Processor.cpp:524-600):
//
//   Image3D::GenNewViews (R/Image3D/Image3D.cpp:109-222) for ALL frames of a sequence at once
//     host          : the homography H = K (R_ K_) of every (frame, view) in double — the only place sin / cos are called
//     k_gv_bbox     : pass A (:146-167), the bounding box of the source pixels whose (uf, vf) is in range: integer min / max of
//                     i % w2 and i / w2, combined per wave, per workgroup in LDS, then one atomicMin per workgroup and bound
//     k_gv_paint    : pass B (:170-216) as a GATHER: one thread per destination pixel enumerates the source pixels that map to it
//                     in descending i and paints from the first one that passes :178 — the reference's ascending scatter, in which
//                     a later i overwrites an earlier one, without racing stores and without the xy array
//   the background cull of the key points (Processor.cpp:567-600) for all view_count * n_frames lists of a sequence
//     k_kc_decide   : one thread per key point, the cameras staged in LDS once per workgroup
//     CompactTail / k_kc_scatter : order-preserving compaction (compact.hip).  The lists lie back to back and so do the compacted
//                     lists, so ONE exclusive scan of `keep` over all keys gives every survivor's place, and out_offsets are that
//                     scan read at key_offsets; a wave copies each surviving 512-byte descriptor row
//
// Every double -> int conversion is cvt_i32 (camera_dev.h).  The library is built with -ffp-contract=off: (uf, vf) recomputed in
// pass B are the values pass A saw.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int VW_TPB = 256;
constexpr int VW_WAVES = VW_TPB / 64;
static_assert(VW_TPB == COMPACT_TPB, "k_kc_decide and k_kc_scatter count and place per workgroup of the shared tail");
constexpr int32_t GV_NONE = 0x7f7f7f7f;                  // what hipMemset(0x7f) leaves: no source pixel was in range
constexpr int KC_CAMS = 64;                               // cameras staged in LDS at a time
static_assert(sizeof(CamDev) % 8 == 0, "the cameras are staged as 8-byte words");

// :151-155 for the source pixel (x, y) = (i % w2, i / w2); qx = w2 * 0.25, qy = h2 * 0.25
__device__ inline void gv_source(const double* H, int x, int y, double qx, double qy, double* uf, double* vf) {
    const int u = cvt_i32((double)x - qx), v = cvt_i32((double)y - qy);
    const double wf = (H[6] * u + H[7] * v) + H[8];
    *uf = ((H[0] * u + H[1] * v) + H[2]) / wf;
    *vf = ((H[3] * u + H[4] * v) + H[5]) / wf;
}
// `u + w * scale2_` of :157-160 for the source column (row) x: monotone in x, so min / max commute with it
__device__ inline double gv_back(int x, double q) { return (double)cvt_i32((double)x - q) + q; }

__device__ inline int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// bbox[fv] = {min x, -max x, min y, -max y}, all combined with min; preset to GV_NONE
__global__ __launch_bounds__(VW_TPB) void k_gv_bbox(const double* __restrict__ Hs, int w, int h, int w2, int h2, int bpv,
                                                    int32_t* __restrict__ bbox) {
    __shared__ int s_bb[4];
    const int fv = blockIdx.x / bpv, b = blockIdx.x % bpv, tid = threadIdx.x;
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = Hs[9 * (int64_t)fv + k];
    if (tid < 4) s_bb[tid] = GV_NONE;
    __syncthreads();
    const double qx = w2 * 0.25, qy = h2 * 0.25;
    int bb[4] = {GV_NONE, GV_NONE, GV_NONE, GV_NONE};
    for (int y = b; y < h2; y += bpv)
        for (int x = tid; x < w2; x += VW_TPB) {
            double uf, vf;
            gv_source(H, x, y, qx, qy, &uf, &vf);
            if (in_range(cvt_i32(uf), cvt_i32(vf), w, h)) {                  // :156
                bb[0] = min(bb[0], x); bb[1] = min(bb[1], -x);
                bb[2] = min(bb[2], y); bb[3] = min(bb[3], -y);
            }
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int m = wave_min_i(bb[k]);
        if ((tid & 63) == 0 && m != GV_NONE) atomicMin(&s_bb[k], m);
    }
    __syncthreads();
    if (tid < 4 && s_bb[tid] != GV_NONE) atomicMin(&bbox[4 * (int64_t)fv + tid], s_bb[tid]);
}

// the source columns (rows) x of [0, n2) with (int)(x - off + 0.5) == d, descending; at most two exist, four neighbours are tried
__device__ inline int gv_sources(int d, double off, int n2, int* out) {
    const int x0 = cvt_i32(floor(((double)d + off) - 0.5));
    int n = 0;
    for (int x = x0 + 2; x >= x0 - 1; --x)
        if (x >= 0 && x < n2 && cvt_i32(((double)x - off) + 0.5) == d && n < 2) out[n++] = x;
    return n;
}

__global__ __launch_bounds__(VW_TPB) void k_gv_paint(const double* __restrict__ Hs, const int32_t* __restrict__ bbox,
                                                     const uint8_t* __restrict__ imgs, int w, int h, int w2, int h2, int view_count, int bpv,
                                                     uint8_t* __restrict__ views, int32_t* __restrict__ tex) {
    const int fv = blockIdx.x / bpv, b = blockIdx.x % bpv;
    const int64_t npx = (int64_t)w * h, p = (int64_t)b * VW_TPB + threadIdx.x;
    if (p >= npx) return;
    const int ud = (int)(p % w), vd = (int)(p / w);
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = Hs[9 * (int64_t)fv + k];
    const double qx = w2 * 0.25, qy = h2 * 0.25;
    double minu = 1000000000.0, minv = 1000000000.0, maxu = -1000000000.0, maxv = -1000000000.0;      // :148-149
    const int32_t* bb = bbox + 4 * (int64_t)fv;
    if (bb[0] != GV_NONE) { minu = gv_back(bb[0], qx); maxu = gv_back(-bb[1], qx); minv = gv_back(bb[2], qy); maxv = gv_back(-bb[3], qy); }
    const double offx = (maxu + minu) * 0.5 - qx, offy = (maxv + minv) * 0.5 - qy;                    // :164-167
    int xs[2], ys[2];
    const int nx = gv_sources(ud, offx, w2, xs), ny = gv_sources(vd, offy, h2, ys);
    const uint8_t* img = imgs + 3 * npx * (fv / view_count);
    uint8_t rgb[3] = {0, 0, 0};
    int32_t t = -1;
    bool found = false;
    for (int a = 0; a < ny && !found; ++a)                                   // descending i = y * w2 + x: the last writer of :170
        for (int c = 0; c < nx && !found; ++c) {
            double uf, vf;
            gv_source(H, xs[c], ys[a], qx, qy, &uf, &vf);
            const double u11 = floor(uf), v11 = floor(vf), u22 = ceil(uf), v22 = ceil(vf);
            const int iu1 = cvt_i32(u11), iv1 = cvt_i32(v11), iu2 = cvt_i32(u22), iv2 = cvt_i32(v22);
            if (!in_range(iu1, iv1, w, h) || !in_range(iu2, iv2, w, h)) continue;                     // :178 (the destination is in range)
            found = true;
            const uint8_t* p11 = img + 3 * ((int64_t)iv1 * w + iu1);
            const uint8_t* p12 = img + 3 * ((int64_t)iv2 * w + iu1);
            const uint8_t* p21 = img + 3 * ((int64_t)iv1 * w + iu2);
            const uint8_t* p22 = img + 3 * ((int64_t)iv2 * w + iu2);
            const bool ueq = fabs(u11 - u22) <= 1e-9, veq = fabs(v11 - v22) <= 1e-9;
            if (ueq && veq) {
                for (int k = 0; k < 3; ++k) rgb[k] = p11[k];
                t = cvt_i32(v11 * w + u11);
                break;
            }
            if (ueq) {
                const double s1 = (vf - v11) / (v22 - v11), s2 = 1 - s1;
                for (int k = 0; k < 3; ++k) rgb[k] = (uint8_t)(int)(p11[k] * s2 + p12[k] * s1);
            } else if (veq) {
                const double s1 = (uf - u11) / (u22 - u11), s2 = 1 - s1;
                for (int k = 0; k < 3; ++k) rgb[k] = (uint8_t)(int)(p11[k] * s2 + p21[k] * s1);
            } else {
                const double s1 = (u22 - uf) * (v22 - vf), s2 = (uf - u11) * (v22 - vf), s3 = (u22 - uf) * (vf - v11), s4 = (uf - u11) * (vf - v11);
                for (int k = 0; k < 3; ++k) rgb[k] = (uint8_t)(int)(((p11[k] * s1 + p21[k] * s2) + p12[k] * s3) + p22[k] * s4);
            }
            t = cvt_i32(vf + 0.5) * w + cvt_i32(uf + 0.5);
        }
    uint8_t* o = views + 3 * (npx * fv + p);
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
    tex[npx * fv + p] = t;
}

// RotationMatrix (R/Common/Utils.h:124-138), K_ (Image3D.cpp:123-125) and H = K (R_ K_) (:144); every 3 x 3 product is
// a0 b0 + a1 b1 + a2 b2, left to right
void mul33(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
void gv_homography(const mvs_camera& c, int axis, double angle_deg, double* H) {
    const double u[3] = {c.R[3 * axis], c.R[3 * axis + 1], c.R[3 * axis + 2]};
    const double angle = angle_deg / 180 * M_PI;
    const double cosine = cos(angle), sine = sin(angle);
    const double R_[9] = {cosine + u[0] * u[0] * (1 - cosine),         u[0] * u[1] * (1 - cosine) - u[2] * sine,  u[1] * sine + u[0] * u[2] * (1 - cosine),
                          u[2] * sine + u[0] * u[1] * (1 - cosine),    cosine + u[1] * u[1] * (1 - cosine),       -u[0] * sine + u[1] * u[2] * (1 - cosine),
                          -u[1] * sine + u[0] * u[2] * (1 - cosine),   u[0] * sine + u[1] * u[2] * (1 - cosine),  cosine + u[2] * u[2] * (1 - cosine)};
    const double K[9] = {c.fx, 0.0, c.cx, 0.0, c.fy, c.cy, 0.0, 0.0, 1.0};
    const double K_[9] = {1.0 / c.fx, 0.0, -c.cx / c.fx, 0.0, 1.0 / c.fy, -c.cy / c.fy, 0.0, 0.0, 1.0};
    double T[9];
    mul33(R_, K_, T);
    mul33(K, T, H);
}

int check_views(const char* fn, int32_t n_frames, const mvs_camera* cams, const void* imgs, int32_t view_count, int32_t axis, const void* views,
                const void* tex) {
    if (view_count < 1) return bad(fn, "need view_count >= 1");
    if (axis < 0 || axis > 2) return bad(fn, "axis must be 0, 1 or 2");
    int rc = check_cams(fn, n_frames, cams);
    if (rc) return rc;
    if (!imgs || !views || !tex) return bad(fn, "imgs, views or tex is NULL");
    const int64_t npx = (int64_t)cams[0].w * cams[0].h, nfv = (int64_t)n_frames * view_count;
    if (nfv * ((npx + VW_TPB - 1) / VW_TPB) > 0x7fffffffLL) return bad(fn, "n_frames * view_count * w * h is too large for one launch");
    return MVS_OK;
}

// images and outputs in HBM; returns with s synchronised
int views_core(int n, const mvs_camera* cams, const uint8_t* imgs, int view_count, int axis, double rot, uint8_t* views, int32_t* tex,
               hipStream_t s) {
    std::vector<double> angle;                                              // :131-133
    for (int i = view_count / 2; i > 0; --i) angle.push_back(-rot * i);
    for (int i = 0; i <= view_count / 2; ++i) angle.push_back(rot * i);
    const int nfv = n * view_count, w = cams[0].w, h = cams[0].h;
    const int w2 = (int)(w * 2.0), h2 = (int)(h * 2.0);                     // :120-121
    std::vector<double> H(9 * (size_t)nfv);
    for (int f = 0; f < n; ++f)
        for (int k = 0; k < view_count; ++k) gv_homography(cams[f], axis, angle[(size_t)k], &H[9 * ((size_t)f * view_count + k)]);
    Scratch dH, dbb;
    int rc;
    if ((rc = up_async(dH, H.data(), H.size(), s)) || (rc = dbb.alloc(sizeof(int32_t) * 4 * (size_t)nfv, s))) return rc;
    HIPCHK(hipMemsetAsync(dbb.p, 0x7f, sizeof(int32_t) * 4 * (size_t)nfv, s));
    const int bpa = h2 < 512 ? h2 : 512;
    const int bpb = (int)(((int64_t)w * h + VW_TPB - 1) / VW_TPB);
    k_gv_bbox<<<dim3((unsigned)(nfv * bpa)), dim3(VW_TPB), 0, s>>>(dH.as<double>(), w, h, w2, h2, bpa, dbb.as<int32_t>());
    k_gv_paint<<<dim3((unsigned)((int64_t)nfv * bpb)), dim3(VW_TPB), 0, s>>>(dH.as<double>(), dbb.as<int32_t>(), imgs, w, h, w2, h2, view_count, bpb,
                                                                           views, tex);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// ------------------------------------------------------------------ key-point cull ----
__global__ __launch_bounds__(VW_TPB) void k_kc_decide(const float* __restrict__ keys, int64_t total, const int64_t* __restrict__ off, int nlists,
                                                      int view_count, int n_frames, const CamDev* __restrict__ cams,
                                                      const int32_t* __restrict__ tex, const float* __restrict__ dsp,
                                                      const uint8_t* __restrict__ mask, double mn, double mx, uint8_t* __restrict__ keep,
                                                      int32_t* __restrict__ cnt) {
    __shared__ CamDev s_cam[KC_CAMS];
    __shared__ int s_wsum[VW_WAVES];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * VW_TPB + tid;
    const int w = cams[0].w, h = cams[0].h;
    const int64_t npx = (int64_t)w * h;
    bool ok = false;
    int frame = -1;
    d3 p = mk3(0, 0, 0);
    if (r < total) {
        const int l = segment_of(off, nlists, r);                       // the list of key r
        frame = l / view_count;
        const int x = cvt_i32((double)keys[4 * r]), y = cvt_i32((double)keys[4 * r + 1]);          // GetTexIndex's int parameters (:575)
        if (in_range(x, y, w, h)) {
            const int32_t idx = tex[(int64_t)l * npx + (int64_t)y * w + x];
            if (idx >= 0 && idx < npx) {                                                             // -1: unmapped
                const double d = (double)dsp[frame * npx + idx];
                if (!(d < mn || d > mx) && (!mask || mask[frame * npx + idx])) {                    // IsValid, InMask (:576)
                    ok = true;
                    p = world_from_img(cams[frame], idx % w, idx / w, 1.0 / d);                       // GetPoint (:578)
                }
            }
        }
    }
    for (int c0 = 0; c0 < n_frames; c0 += KC_CAMS) {                         // n_frames is uniform: every thread meets the barriers
        const int m = n_frames - c0 < KC_CAMS ? n_frames - c0 : KC_CAMS;
        __syncthreads();
        const unsigned long long* src = (const unsigned long long*)(cams + c0);
        for (int i = tid; i < m * (int)(sizeof(CamDev) / 8); i += VW_TPB) ((unsigned long long*)s_cam)[i] = src[i];
        __syncthreads();
        if (ok)
            for (int j = 0; j < m; ++j) {
                if (c0 + j == frame) continue;
                int32_t u, v;
                img_from_world(s_cam[j], p, &u, &v);                         // :583
                if (!in_range(u, v, w, h)) { ok = false; break; }
            }
    }
    if (r < total) keep[r] = ok ? 1 : 0;
    const WgRank k = wg_rank<VW_WAVES>(ok, s_wsum);
    if (tid == 0) cnt[blockIdx.x] = k.total;
}

__global__ __launch_bounds__(VW_TPB) void k_kc_scatter(const float* __restrict__ keys, const float* __restrict__ descs, int64_t total,
                                                       const uint8_t* __restrict__ keep, const int32_t* __restrict__ base,
                                                       float* __restrict__ out_keys, float* __restrict__ out_descs) {
    __shared__ int s_wsum[VW_WAVES], s_pos[VW_TPB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * VW_TPB, r = r0 + tid;
    const bool f = r < total && keep[r];
    const int pos = base[blockIdx.x] + wg_rank<VW_WAVES>(f, s_wsum).rank;
    s_pos[tid] = f ? pos : -1;
    if (f) {
        const float* a = keys + 4 * r;
        float* o = out_keys + 4 * (int64_t)pos;
        o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
    }
    if (!descs) return;
    __syncthreads();
    for (int q = wv; q < VW_TPB; q += VW_WAVES) {                            // a wave per 512-byte row
        const int pp = s_pos[q];
        if (pp < 0) continue;
        const float* a = descs + 128 * (r0 + q);
        float* o = out_descs + 128 * (int64_t)pp;
        o[lane] = a[lane];
        o[lane + 64] = a[lane + 64];
    }
}

int check_cull(const char* fn, int32_t n_frames, int32_t view_count, const mvs_camera* cams, const int64_t* off, const void* keys,
               const void* descs, const void* tex, const void* depths, const void* out_off, const void* out_keys, const void* out_descs) {
    if (view_count < 1) return bad(fn, "need view_count >= 1");
    int rc = check_cams(fn, n_frames, cams);
    if (rc) return rc;
    if ((int64_t)n_frames * view_count > 0x7ffffffeLL) return bad(fn, "too many lists");
    if (!off || !out_off) return bad(fn, "key_offsets / out_offsets is NULL");
    if (!tex || !depths) return bad(fn, "tex or depths is NULL");
    const int nl = n_frames * view_count;
    if ((rc = check_offsets(fn, "key_offsets", off, nl, 0x7fffffffLL))) return rc;
    if (off[nl] > 0 && (!keys || !out_keys)) return bad(fn, "keys / out_keys is NULL");
    if (descs && !out_descs) return bad(fn, "descs given without out_descs");
    return MVS_OK;
}

// everything but the offsets in HBM; keep may be NULL; returns with s synchronised
int cull_core(int n, int view_count, const mvs_camera* cams, const int64_t* off, const float* keys, const float* descs, const int32_t* tex,
              const float* depths, double mn, double mx, const uint8_t* mask, uint8_t* keep, int64_t* out_off, float* out_keys, float* out_descs,
              hipStream_t s) {
    const int nl = n * view_count;
    const int64_t total = off[nl];
    if (total == 0) { std::memset(out_off, 0, sizeof(int64_t) * ((size_t)nl + 1)); return MVS_OK; }
    const int nb = (int)((total + VW_TPB - 1) / VW_TPB);
    std::vector<CamDev> hc;
    Scratch dcam, doff, dkeep;
    CompactTail ct;
    int rc;
    if ((rc = up_cams(dcam, hc, cams, (size_t)n, s)) || (rc = up_async(doff, off, (size_t)nl + 1, s)) || (rc = ct.alloc((size_t)nb, (size_t)nl, s)) ||
        (!keep && (rc = dkeep.alloc((size_t)total, s)))) return rc;
    if (!keep) keep = dkeep.as<uint8_t>();
    k_kc_decide<<<dim3((unsigned)nb), dim3(VW_TPB), 0, s>>>(keys, total, doff.as<int64_t>(), nl, view_count, n, dcam.as<CamDev>(), tex, depths, mask, mn, mx,
                                                           keep, ct.cnt.as<int32_t>());
    ct.segments(nb, doff.as<int64_t>(), nl, total, keep, s);
    k_kc_scatter<<<dim3((unsigned)nb), dim3(VW_TPB), 0, s>>>(keys, descs, total, keep, ct.base.as<int32_t>(), out_keys, out_descs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_off, ct.off.p, sizeof(int64_t) * ((size_t)nl + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_gen_new_views_dev(int32_t n_frames, const mvs_camera* cams, const uint8_t* imgs_dev, int32_t view_count, int32_t axis, double rot_angle,
                          uint8_t* views_dev, int32_t* tex_dev, void* hip_stream) {
    MVS_TRACE();
    int rc = check_views(__func__, n_frames, cams, imgs_dev, view_count, axis, views_dev, tex_dev);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return views_core(n_frames, cams, imgs_dev, view_count, axis, rot_angle, views_dev, tex_dev, (hipStream_t)hip_stream);
}

int mvs_gen_new_views(int32_t n_frames, const mvs_camera* cams, const uint8_t* imgs, int32_t view_count, int32_t axis, double rot_angle,
                      uint8_t* views, int32_t* tex) {
    MVS_TRACE();
    int rc = check_views(__func__, n_frames, cams, imgs, view_count, axis, views, tex);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    const size_t npx = (size_t)cams[0].w * cams[0].h, nfv = (size_t)n_frames * view_count;
    Scratch di, dv, dt;
    if ((rc = up(di, imgs, n_frames * npx * 3)) || (rc = dv.alloc(nfv * npx * 3)) || (rc = dt.alloc(sizeof(int32_t) * nfv * npx))) return rc;
    if ((rc = views_core(n_frames, cams, di.as<uint8_t>(), view_count, axis, rot_angle, dv.as<uint8_t>(), dt.as<int32_t>(), nullptr))) return rc;
    if ((rc = down(views, dv, nfv * npx * 3))) return rc;
    return down(tex, dt, nfv * npx);
}

int mvs_keypoint_cull_dev(int32_t n_frames, int32_t view_count, const mvs_camera* cams, const int64_t* key_offsets, const float* keys_dev,
                          const float* descs_dev, const int32_t* tex_dev, const float* depths_dev, double min_dsp, double max_dsp,
                          const uint8_t* mask_dev, uint8_t* keep_dev, int64_t* out_offsets, float* out_keys_dev, float* out_descs_dev,
                          void* hip_stream) {
    MVS_TRACE();
    int rc = check_cull(__func__, n_frames, view_count, cams, key_offsets, keys_dev, descs_dev, tex_dev, depths_dev, out_offsets, out_keys_dev, out_descs_dev);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return cull_core(n_frames, view_count, cams, key_offsets, keys_dev, descs_dev, tex_dev, depths_dev, min_dsp, max_dsp, mask_dev, keep_dev, out_offsets,
                     out_keys_dev, out_descs_dev, (hipStream_t)hip_stream);
}

int mvs_keypoint_cull(int32_t n_frames, int32_t view_count, const mvs_camera* cams, const int64_t* key_offsets, const float* keys, const float* descs,
                      const int32_t* tex, const float* depths, double min_dsp, double max_dsp, const uint8_t* mask, uint8_t* keep,
                      int64_t* out_offsets, float* out_keys, float* out_descs) {
    MVS_TRACE();
    int rc = check_cull(__func__, n_frames, view_count, cams, key_offsets, keys, descs, tex, depths, out_offsets, out_keys, out_descs);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    const size_t npx = (size_t)cams[0].w * cams[0].h, nl = (size_t)n_frames * view_count, total = (size_t)key_offsets[nl];
    Scratch dk, dd, dt, dz, dm, dkeep, dok, dod;
    if ((rc = up(dk, keys, 4 * total)) || (rc = up(dt, tex, nl * npx)) || (rc = up(dz, depths, n_frames * npx)) || (rc = dkeep.alloc(total)) ||
        (rc = dok.alloc(sizeof(float) * 4 * total)) || (descs && ((rc = up(dd, descs, 128 * total)) || (rc = dod.alloc(sizeof(float) * 128 * total)))) ||
        (mask && (rc = up(dm, mask, n_frames * npx)))) return rc;
    if ((rc = cull_core(n_frames, view_count, cams, key_offsets, dk.as<float>(), descs ? dd.as<float>() : nullptr, dt.as<int32_t>(), dz.as<float>(),
                        min_dsp, max_dsp, mask ? dm.as<uint8_t>() : nullptr, dkeep.as<uint8_t>(), out_offsets, dok.as<float>(),
                        descs ? dod.as<float>() : nullptr, nullptr))) return rc;
    const size_t kept = (size_t)out_offsets[nl];
    if (keep && (rc = down(keep, dkeep, total))) return rc;
    if ((rc = down(out_keys, dok, 4 * kept))) return rc;
    return descs ? down(out_descs, dod, 128 * kept) : MVS_OK;
}

}  // extern "C"

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_views() { return (const void*)k_gv_paint; }
