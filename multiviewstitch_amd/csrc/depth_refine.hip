// depth_refine.hip — mvs_refine_depth_maps (include/mvs.h): the rendered inverse-depth rasters of every sequence taken back to the
// images, the stage DepthRecovery/DepthOptimizer names (RefineAllDepthMaps, DepthOptimizer.cpp:20-43; the frame window of
// RefineDepthMap, :45-63) and leaves without a body (DepthRefineCore is declared and never defined).  The rules are this library's
// definition, stated in include/mvs.h; their per-pixel part is depth_refine_rules.h, one body for this kernel and for host code.
//
//   k_dr_grey    ONE launch turns every image of the call into its 8-bit grey raster (grey8, frontend_dev.h).
//   k_dr_squares ONE launch: the sum of G^2 over the window of every interior pixel of every image.
//   k_dr_refine  ONE launch for all frames of all sequences: a workgroup per DR_TILE x DR_TILE tile of the current frame, a thread per
//                pixel.  Rule 5's sum is evaluated as sum a^2 + sum b^2 - 2 sum a b, exact in uint32: the squares come from
//                k_dr_squares, the products from v_dot4_u32_u8 on four packed bytes.  The current grey tile and its halo of N pixels
//                go to LDS once, as four copies moved by 0..3 bytes, so that every thread reads the rows of its window as aligned
//                dwords ((DR_TILE + 2 N) rows of 3 + ceil((2 N + 1) / 4) dwords per copy, 8096 bytes at N = 15); the rows of a
//                reference window are read from global memory as aligned dwords and moved into place by v_alignbyte_b32:
//                neighbouring pixels land on neighbouring windows.  Frame and sequence come from blockIdx alone, so the cameras stay
//                in scalar registers.  Every thread writes its own pixel of every output and nothing else: no atomic, two runs give
//                the same bytes.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "geom.h"
#include "stitch.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include "depth_refine_rules.h"
#include <cmath>

namespace {

constexpr int DR_TILE = 16, DR_TPB = DR_TILE * DR_TILE, DR_NMAX = 15, DR_SPAN = DR_TILE + 2 * DR_NMAX;
constexpr int DR_ROWW = 3 + (2 * DR_NMAX + 1 + 3) / 4;        // dwords per row of a moved copy: the widest word index (DR_TILE - 1) / 4 plus a window row
constexpr int DR_GREY_PAD = 16;                              // bytes behind the grey rasters: a window row is read as whole aligned dwords

struct DrSeq {                        // one sequence: its cameras cams[cam0 .. cam0 + n), all w x h, cut into tw x th tiles
    int32_t cam0, n, w, h, tw, th;
    int64_t px_off;                   // pixels in front of its first frame
};

__global__ __launch_bounds__(256) void k_dr_grey(const uint8_t* __restrict__ imgs, int64_t npx, uint8_t* __restrict__ grey) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npx) grey[i] = (uint8_t)grey8(imgs + 3 * i);
    else if (i < npx + DR_GREY_PAD) grey[i] = 0;
}

__global__ __launch_bounds__(DR_TPB) void k_dr_squares(const uint8_t* __restrict__ grey, const DrSeq* __restrict__ seqs,
                                                       const int32_t* __restrict__ seq_of, int maxblk, int N, uint32_t* __restrict__ sq) {
    const int cam = blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const DrSeq s = seqs[seq_of[cam]];
    if (b >= s.tw * s.th) return;
    const int u = (b % s.tw) * DR_TILE + threadIdx.x % DR_TILE, v = (b / s.tw) * DR_TILE + threadIdx.x / DR_TILE;
    if (u >= s.w || v >= s.h) return;
    const int64_t at = s.px_off + (int64_t)(cam - s.cam0) * s.w * s.h + (int64_t)v * s.w + u;
    uint32_t acc = 0;
    if (dr_interior(u, v, s.w, s.h, N))
        for (int a = -N; a <= N; ++a)
            for (int c = -N; c <= N; ++c) {
                const uint32_t x = grey[at + (int64_t)a * s.w + c];
                acc += x * x;
            }
    sq[at] = acc;
}

// rule 5's sum from packed bytes: sum a^2 + sum b^2 - 2 sum a b
struct DotSsd {
    const uint32_t* cur;              // LDS: the first dword of the top row of the thread's window in its moved copy; rows are roww apart
    const uint32_t* grey32;           // the grey rasters of the call as dwords (the block is dword aligned and padded)
    const uint32_t* sq;
    int64_t seq_px, npx;              // pixels in front of the sequence; pixels per frame
    int w, N, nw, roww;               // nw: dwords per window row
    uint32_t last_mask, sq_cur;       // the bytes of the last dword that belong to the window; sum a^2
    __device__ int32_t operator()(int g, int u2, int v2) const {
        const int64_t centre = seq_px + g * npx + (int64_t)v2 * w + u2;
        uint32_t dot = 0;
        for (int r = 0; r <= 2 * N; ++r) {
            const int64_t off = centre + (int64_t)(r - N) * w - N;       // the first byte of the reference row
            const uint32_t* p = grey32 + (off >> 2);
            const uint32_t sh = (uint32_t)off & 3u;
            const uint32_t* c = cur + r * roww;
            uint32_t lo = p[0];
            for (int j = 0; j < nw; ++j) {
                const uint32_t hi = p[j + 1];
                const uint32_t bb = __builtin_amdgcn_alignbyte(hi, lo, sh);
                const uint32_t aa = j == nw - 1 ? c[j] & last_mask : c[j];
                dot = __builtin_amdgcn_udot4(aa, bb, dot, false);
                lo = hi;
            }
        }
        return (int32_t)(sq_cur + sq[centre] - 2u * dot);
    }
};

__global__ __launch_bounds__(DR_TPB) void k_dr_refine(const float* __restrict__ depths, const uint8_t* __restrict__ grey, const uint32_t* __restrict__ sq,
                                                      const CamDev* __restrict__ cams, const DrSeq* __restrict__ seqs,
                                                      const int32_t* __restrict__ seq_of, int maxblk, DrRules q, float* __restrict__ out,
                                                      int8_t* __restrict__ k_out, int32_t* __restrict__ sum_out, uint8_t* __restrict__ cnt_out) {
    __shared__ uint8_t s_tile[DR_SPAN * DR_SPAN];
    __shared__ uint32_t s_moved[4 * DR_SPAN * DR_ROWW];
    const int cam = blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const DrSeq s = seqs[seq_of[cam]];
    if (b >= s.tw * s.th) return;                                        // the whole workgroup: no barrier is skipped by a part of it
    const int f = cam - s.cam0, N = q.N, span = DR_TILE + 2 * N;
    const int u0 = (b % s.tw) * DR_TILE, v0 = (b / s.tw) * DR_TILE;
    const int64_t npx = (int64_t)s.w * s.h;
    const uint8_t* gf = grey + s.px_off + f * npx;
    for (int i = threadIdx.x; i < span * span; i += DR_TPB) {            // tile and halo; what lies outside the raster is never used
        const int y = v0 - N + i / span, x = u0 - N + i % span;
        s_tile[i] = (x >= 0 && x < s.w && y >= 0 && y < s.h) ? gf[(int64_t)y * s.w + x] : 0;
    }
    __syncthreads();
    const int nw = (2 * N + 1 + 3) / 4, roww = 3 + nw;
    for (int i = threadIdx.x; i < 4 * span * roww; i += DR_TPB) {        // copy m, row y, dword j: the tile's bytes 4 j + m .. 4 j + m + 3 of row y
        const int m = i / (span * roww), y = i / roww % span, x = i % roww * 4 + m;
        uint32_t word = 0;
        for (int k = 0; k < 4; ++k)
            if (x + k < span) word |= (uint32_t)s_tile[y * span + x + k] << (8 * k);
        s_moved[i] = word;
    }
    __syncthreads();
    const int tx = threadIdx.x % DR_TILE, ty = threadIdx.x / DR_TILE, u = u0 + tx, v = v0 + ty;
    if (u >= s.w || v >= s.h) return;
    const int64_t at = s.px_off + f * npx + (int64_t)v * s.w + u;
    const float d0 = depths[at];
    const int rem = 2 * N + 1 - 4 * (nw - 1);                            // 1 or 3 bytes of the last dword: the window is odd
    const DotSsd ssd = {s_moved + ((tx & 3) * span + ty) * roww + (tx >> 2), (const uint32_t*)grey, sq, s.px_off, npx, s.w, N, nw, roww,
                        (1u << (8 * rem)) - 1u, sq[at]};
    const DrPixel r = dr_pixel(cams + s.cam0, s.n, f, u, v, d0, q, ssd);
    if (r.accepted) out[at] = (float)r.d;
    else ((uint32_t*)out)[at] = ((const uint32_t*)depths)[at];          // bit for bit, a NaN's payload included
    if (k_out) k_out[at] = (int8_t)r.k;
    if (sum_out) sum_out[at] = r.sum;
    if (cnt_out) cnt_out[at] = (uint8_t)r.cnt;
}

// what a call is made of, built by the argument checks on the host
struct DrPlan {
    std::vector<DrSeq> seqs;
    std::vector<int32_t> seq_of;
    DrRules q;
    int ncam = 0, maxblk = 0;
    int64_t px = 0;
};

int check_dr(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const void* imgs, const void* depths,
             const mvs_depth_refine_params* p, const void* out, DrPlan* pl) {
    if (!cam_off || !cams || !imgs || !depths || !p || !out) return bad(fn, "cam_off, cams, imgs, depths, params or out is NULL");
    if (n_seq < 1) return bad(fn, "need n_seq >= 1");
    int rc = check_offsets(fn, "cam_off", cam_off, n_seq);
    if (rc) return rc;
    if (!std::isfinite(p->dsp_min) || !std::isfinite(p->dsp_max) || !std::isfinite(p->rel_range) || !std::isfinite(p->ssd_err))
        return bad(fn, "a parameter is not finite");
    if (p->dsp_min <= 0.0 || p->dsp_min > p->dsp_max) return bad(fn, "need 0 < dsp_min <= dsp_max");
    if (p->rel_range <= 0.0 || p->rel_range >= 1.0) return bad(fn, "need 0 < rel_range < 1");
    if (p->ssd_err < 0.0) return bad(fn, "ssd_err is negative");
    if (p->ssd_win < 0 || p->ssd_win > DR_NMAX) return bad(fn, "ssd_win must lie in [0, 15]");
    if (p->ref_frm_count < 1 || p->ref_frm_count > DR_MAX_REFS + 1 || p->ref_frm_count % 2 == 0) return bad(fn, "ref_frm_count must be odd and lie in [1, 9]");
    if (p->steps < 1 || p->steps > 63) return bad(fn, "steps must lie in [1, 63]");
    if (p->flags & ~(int32_t)MVS_REFINE_SUBSTEP) return bad(fn, "unknown flag bits");
    if (out == depths) return bad(fn, "out must not alias depths");
    pl->q = DrRules{p->dsp_min, p->dsp_max, p->rel_range, p->ssd_err, p->ssd_win, p->ref_frm_count, p->steps, p->flags};
    pl->ncam = cam_off[n_seq];
    pl->seqs.resize((size_t)n_seq);
    pl->seq_of.resize((size_t)pl->ncam);
    for (int k = 0; k < n_seq; ++k) {
        DrSeq& s = pl->seqs[(size_t)k];
        s = DrSeq{cam_off[k], cam_off[k + 1] - cam_off[k], 0, 0, 0, 0, pl->px};
        if (!s.n) continue;
        const mvs_camera* c = cams + s.cam0;
        for (int f = 0; f < s.n; ++f) {
            if (!cam_fine(c + f)) return bad(fn, "a camera needs w, h > 0 and fx, fy != 0");
            if (c[f].w != c[0].w || c[f].h != c[0].h) return bad(fn, "the frames of a sequence must share one raster size");
            pl->seq_of[(size_t)(s.cam0 + f)] = k;
        }
        if ((int64_t)c[0].w * c[0].h > 0x7fffffffLL) return bad(fn, "w * h of a frame must fit an int32 pixel index");
        s.w = c[0].w; s.h = c[0].h;
        s.tw = (int)(((int64_t)s.w + DR_TILE - 1) / DR_TILE); s.th = (int)(((int64_t)s.h + DR_TILE - 1) / DR_TILE);
        const int64_t tiles = (int64_t)s.tw * s.th;
        if (tiles > 0x7fffffffLL) return bad(fn, "too many tiles in a frame");
        if (tiles > pl->maxblk) pl->maxblk = (int)tiles;
        pl->px += (int64_t)s.n * s.w * s.h;
    }
    if ((int64_t)pl->ncam * pl->maxblk > 0x7fffffffLL || (pl->px + DR_GREY_PAD + 255) / 256 > 0x7fffffffLL)
        return bad(fn, "cameras * w * h is too large for one launch");
    return MVS_OK;
}

// grey pass, squares and refinement on device arrays, enqueued on s; the tables stay alive in the object until the caller has synchronised
struct DrRun {
    std::vector<CamDev> hc;
    Scratch dcam, dseq, dsof, dgrey, dsq;
    int launch(const DrPlan& pl, const mvs_camera* cams, const uint8_t* imgs, const float* depths, float* out, int8_t* k_out, int32_t* sum_out,
               uint8_t* cnt_out, hipStream_t s) {
        int rc;
        if ((rc = up_cams(dcam, hc, cams, (size_t)pl.ncam, s)) || (rc = up_async(dseq, pl.seqs.data(), pl.seqs.size(), s)) ||
            (rc = up_async(dsof, pl.seq_of.data(), pl.seq_of.size(), s)) || (rc = dgrey.alloc((size_t)pl.px + DR_GREY_PAD, s)) ||
            (rc = dsq.alloc(sizeof(uint32_t) * (size_t)pl.px, s))) return rc;
        const dim3 tiles((unsigned)(pl.ncam * pl.maxblk));
        k_dr_grey<<<dim3((unsigned)((pl.px + DR_GREY_PAD + 255) / 256)), dim3(256), 0, s>>>(imgs, pl.px, dgrey.as<uint8_t>());
        k_dr_squares<<<tiles, dim3(DR_TPB), 0, s>>>(dgrey.as<uint8_t>(), dseq.as<DrSeq>(), dsof.as<int32_t>(), pl.maxblk, pl.q.N, dsq.as<uint32_t>());
        k_dr_refine<<<tiles, dim3(DR_TPB), 0, s>>>(depths, dgrey.as<uint8_t>(), dsq.as<uint32_t>(), dcam.as<CamDev>(), dseq.as<DrSeq>(), dsof.as<int32_t>(),
                                                   pl.maxblk, pl.q, out, k_out, sum_out, cnt_out);
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }
};

}  // namespace

// the host form under the name fn (mvs_refine_depth_maps, mvs_processor_refine_depths)
int refine_depth_maps_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                           const mvs_depth_refine_params* p, float* out, int8_t* k_out, int32_t* sum_out, uint8_t* cnt_out) {
    DrPlan pl;
    int rc = check_dr(fn, n_seq, cam_off, cams, imgs, depths, p, out, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    const size_t n = (size_t)pl.px;
    Scratch di, dd, dout, dk, dsum, dcnt;
    if ((rc = up(di, imgs, 3 * n)) || (rc = up(dd, depths, n)) || (rc = dout.alloc(sizeof(float) * n)) || (k_out && (rc = dk.alloc(n))) ||
        (sum_out && (rc = dsum.alloc(sizeof(int32_t) * n))) || (cnt_out && (rc = dcnt.alloc(n)))) return rc;
    DrRun run;
    if ((rc = run.launch(pl, cams, di.as<uint8_t>(), dd.as<float>(), dout.as<float>(), k_out ? dk.as<int8_t>() : nullptr,
                         sum_out ? dsum.as<int32_t>() : nullptr, cnt_out ? dcnt.as<uint8_t>() : nullptr, nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    if ((rc = down(out, dout, n))) return rc;
    if (k_out && (rc = down(k_out, dk, n))) return rc;
    if (sum_out && (rc = down(sum_out, dsum, n))) return rc;
    return cnt_out ? down(cnt_out, dcnt, n) : MVS_OK;
}

extern "C" {

void mvs_depth_refine_default_params(mvs_depth_refine_params* p) {
    if (!p) return;
    p->dsp_min = 0.0025; p->dsp_max = 0.3; p->rel_range = 0.04; p->ssd_err = 40.0;
    p->ssd_win = 7; p->ref_frm_count = 5; p->steps = 8; p->flags = MVS_REFINE_SUBSTEP;
}

int mvs_refine_depth_maps(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                          const mvs_depth_refine_params* p, float* out, int8_t* k_out, int32_t* sum_out, uint8_t* cnt_out) {
    MVS_TRACE();
    return refine_depth_maps_host(__func__, n_seq, cam_off, cams, imgs, depths, p, out, k_out, sum_out, cnt_out);
}

int mvs_refine_depth_maps_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev, const float* depths_dev,
                              const mvs_depth_refine_params* p, float* out_dev, int8_t* k_out_dev, int32_t* sum_out_dev, uint8_t* cnt_out_dev,
                              void* hip_stream) {
    MVS_TRACE();
    DrPlan pl;
    int rc = check_dr(__func__, n_seq, cam_off, cams, imgs_dev, depths_dev, p, out_dev, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.px == 0) return MVS_OK;
    DrRun run;
    if ((rc = run.launch(pl, cams, imgs_dev, depths_dev, out_dev, k_out_dev, sum_out_dev, cnt_out_dev, (hipStream_t)hip_stream))) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    return MVS_OK;
}

}  // extern "C"
