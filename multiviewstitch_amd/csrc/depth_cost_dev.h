// depth_cost_dev.h — the one statement of rule 5's window cost on the device, shared by depth_refine.hip (mvs_refine_depth_maps) and
// depth_recover.hip (mvs_recover_depth_maps): the plan of a call (its sequences cut into DR_TILE x DR_TILE tiles), the grey launch, the
// squares launch, the current tile as four moved copies in LDS, and DotSsd, the exact integer sum on v_dot4_u32_u8.
//
//   k_dr_grey    ONE launch turns every image of the call into its 8-bit grey raster (grey8, frontend_dev.h).
//   k_dr_squares ONE launch: the sum of G^2 over the window of every interior pixel of every image.
//   DrTile       The current grey tile and its halo of N pixels go to LDS once, as four copies moved by 0..3 bytes, so that every thread
//                reads the rows of its window as aligned dwords ((DR_TILE + 2 N) rows of 3 + ceil((2 N + 1) / 4) dwords per copy, 8096
//                bytes at N = 15).
//   DotSsd       Rule 5's sum as sum a^2 + sum b^2 - 2 sum a b, exact in uint32: the squares come from k_dr_squares, the products from
//                v_dot4_u32_u8 on four packed bytes; the rows of a reference window are read from global memory as aligned dwords and
//                moved into place by v_alignbyte_b32: neighbouring pixels land on neighbouring windows.
// Everything here has internal linkage: each of the two files compiles its own copy of the two small kernels.
#ifndef MVS_DEPTH_COST_DEV_H_
#define MVS_DEPTH_COST_DEV_H_
#include "engine.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include "depth_refine_rules.h"

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

// the LDS of a workgroup of DR_TPB threads that evaluates DotSsd on one tile
struct DrTile {
    uint8_t tile[DR_SPAN * DR_SPAN];
    uint32_t moved[4 * DR_SPAN * DR_ROWW];
    // Called by the whole workgroup: the tile at (u0, v0) of the grey frame gf (w x h) with its halo of N pixels, then the four moved
    // copies.  Two barriers; the copies are complete on return.
    __device__ void load(const uint8_t* __restrict__ gf, int w, int h, int u0, int v0, int N) {
        const int span = DR_TILE + 2 * N;
        for (int i = threadIdx.x; i < span * span; i += DR_TPB) {            // tile and halo; what lies outside the raster is never used
            const int y = v0 - N + i / span, x = u0 - N + i % span;
            tile[i] = (x >= 0 && x < w && y >= 0 && y < h) ? gf[(int64_t)y * w + x] : 0;
        }
        __syncthreads();
        const int nw = (2 * N + 1 + 3) / 4, roww = 3 + nw;
        for (int i = threadIdx.x; i < 4 * span * roww; i += DR_TPB) {        // copy m, row y, dword j: the tile's bytes 4 j + m .. 4 j + m + 3 of row y
            const int m = i / (span * roww), y = i / roww % span, x = i % roww * 4 + m;
            uint32_t word = 0;
            for (int k = 0; k < 4; ++k)
                if (x + k < span) word |= (uint32_t)tile[y * span + x + k] << (8 * k);
            moved[i] = word;
        }
        __syncthreads();
    }
    // rule 5's sum for the thread's pixel (tx, ty) of the tile, raster index `at`, in sequence s
    __device__ DotSsd ssd(const uint8_t* grey, const uint32_t* sq, const DrSeq& s, int64_t at, int tx, int ty, int N) const {
        const int span = DR_TILE + 2 * N, nw = (2 * N + 1 + 3) / 4, roww = 3 + nw;
        const int rem = 2 * N + 1 - 4 * (nw - 1);                            // 1 or 3 bytes of the last dword: the window is odd
        return DotSsd{moved + ((tx & 3) * span + ty) * roww + (tx >> 2), (const uint32_t*)grey, sq, s.px_off, (int64_t)s.w * s.h, s.w, N, nw, roww,
                      (1u << (8 * rem)) - 1u, sq[at]};
    }
};

// the sequences of a call, built by the argument checks on the host
struct DrSeqPlan {
    std::vector<DrSeq> seqs;
    std::vector<int32_t> seq_of;
    int ncam = 0, maxblk = 0;
    int64_t px = 0;
};

// the checks of the cameras of a call (cam_off is known to ascend from 0) and its cut into tiles
inline int dr_plan_seqs(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, DrSeqPlan* pl) {
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

// the tables of a call on the device and its grey pass and squares, enqueued on s; the tables stay alive in the object until the caller
// has synchronised
struct DrCost {
    std::vector<CamDev> hc;
    Scratch dcam, dseq, dsof, dgrey, dsq;
    int launch(const DrSeqPlan& pl, int N, const mvs_camera* cams, const uint8_t* imgs, hipStream_t s) {
        int rc;
        if ((rc = up_cams(dcam, hc, cams, (size_t)pl.ncam, s)) || (rc = up_async(dseq, pl.seqs.data(), pl.seqs.size(), s)) ||
            (rc = up_async(dsof, pl.seq_of.data(), pl.seq_of.size(), s)) || (rc = dgrey.alloc((size_t)pl.px + DR_GREY_PAD, s)) ||
            (rc = dsq.alloc(sizeof(uint32_t) * (size_t)pl.px, s))) return rc;
        k_dr_grey<<<dim3((unsigned)((pl.px + DR_GREY_PAD + 255) / 256)), dim3(256), 0, s>>>(imgs, pl.px, dgrey.as<uint8_t>());
        k_dr_squares<<<tiles(pl), dim3(DR_TPB), 0, s>>>(dgrey.as<uint8_t>(), dseq.as<DrSeq>(), dsof.as<int32_t>(), pl.maxblk, N, dsq.as<uint32_t>());
        return MVS_OK;
    }
    static dim3 tiles(const DrSeqPlan& pl) { return dim3((unsigned)(pl.ncam * pl.maxblk)); }
};

}  // namespace

#endif
