// jpeg.hip — mvs_jpeg_info, mvs_jpeg_decode(_dev) (include/mvs.h): the batched baseline JPEG decoder, rules J1-J8.  The header walk is
// host code (jpeg_rules.h: jpeg_parse) on the fan-out of host_parts.h; the rest is three launch sets, each over all images of the call.
// Which block a wave or a lane is at comes from the walks of jpeg_rules.h, which the encoder shares; the last two launch sets are
// jpeg_pixels_tail, which the encoder's round trip runs too; the timed hook's stage times come from the StageClock of engine.h.
//
//   k_jpeg_entropy ONE launch, a workgroup of one wave per entry of the segment table (a restart interval, or a whole scan).  The wave
//                  copies the Huffman tables of its image into LDS and stages the segment's bytes through a ring of 2048 bytes in LDS,
//                  1024 bytes per refill, as aligned dwords.  Lane 0 decodes one block at a time into 64 int16 of LDS (J3 is serial);
//                  the 64 lanes then write the block, de-zigzagged, as one 128-byte row.  Every block of the segment's MCU range is
//                  written, as zeros behind an error, so the coefficient array needs no memset.  An error goes into the image's error
//                  word with atomicOr: the only atomic, and not on data.
//   k_jpeg_idct    ONE launch: J4.  One lane per block: the lane runs pass 1 on the eight columns with the workspace in registers, then
//                  pass 2 on the eight rows, and writes each row of eight samples as one 8-byte store into the component plane (padded
//                  to whole MCUs).  Eight lanes per block with the workspace in LDS were measured against it and were slower.
//   k_jpeg_pixels  ONE launch, a thread per output pixel: J5-J7, three bytes per thread, neighbouring threads neighbouring bytes.
//
// No thread writes a byte another thread writes: two runs give the same bytes.
#include "engine.h"
#include "trace.h"
#include "jpeg_rules.h"
#include "../../include/mvs_test.h"
#include "stitch.h"
#include <algorithm>

namespace {

constexpr int JPEG_RING = 2048, JPEG_HALF = JPEG_RING / 2;     // a block takes at most 64 x 31 bits, 496 bytes with every byte stuffed
constexpr int HUFF_DWORDS = (int)(sizeof(JpegHuff) / 4);

struct JpegImg {                       // one image of the call
    JpegLayout L;
    int32_t q[3];                      // the component's quantisers: 64 uint16 at quant + 64 * q[c]
    int32_t ntab, tab[6];              // the distinct Huffman tables of the image, as indices of the call's table array
    int32_t dcs[3], acs[3];            // the component's tables among those
    int32_t pad;
};

struct RingBytes {
    const uint8_t* ring;
    __device__ uint32_t operator()(int64_t pos) const { return ring[pos & (JPEG_RING - 1)]; }
};

__global__ __launch_bounds__(64) void k_jpeg_entropy(const JpegSeg* __restrict__ segs, const JpegImg* __restrict__ imgs,
                                                     const JpegHuff* __restrict__ huffs, const uint32_t* __restrict__ data32,
                                                     int16_t* __restrict__ coef, int32_t* __restrict__ errw) {
    __shared__ JpegHuff s_tab[6];
    __shared__ uint32_t s_ring[JPEG_RING / 4];
    __shared__ int16_t s_blk[64];
    __shared__ int32_t s_pred[3];
    __shared__ int64_t s_pos;
    __shared__ int32_t s_err;
    const int lane = threadIdx.x;
    const JpegSeg sg = segs[blockIdx.x];
    const JpegImg* im = imgs + sg.image;
    __shared__ JpegLayout s_lay;                                     // indexed by the component: LDS, not registers
    for (int i = lane; i < (int)(sizeof(JpegLayout) / 4); i += 64) ((uint32_t*)&s_lay)[i] = ((const uint32_t*)&im->L)[i];
    const JpegLayout& L = s_lay;
    const int ntab = im->ntab;
    for (int i = lane; i < ntab * HUFF_DWORDS; i += 64)
        ((uint32_t*)s_tab)[i] = ((const uint32_t*)(huffs + im->tab[i / HUFF_DWORDS]))[i % HUFF_DWORDS];
    int64_t win = sg.first & ~(int64_t)3;                            // the ring holds bytes [win, win + JPEG_RING) of the call's data
    for (int i = lane; i < JPEG_RING / 4; i += 64) {
        const int64_t off = win + 4 * i;
        s_ring[(off >> 2) & (JPEG_RING / 4 - 1)] = off < sg.end ? data32[off >> 2] : 0u;
    }
    if (lane < 3) s_pred[lane] = 0;
    if (lane == 0) { s_pos = sg.first; s_err = 0; }
    __syncthreads();
    JpegBits<RingBytes> bits{RingBytes{(const uint8_t*)s_ring}, sg.first, sg.end, 0u, 0};     // lane 0's
    int err = 0;
    const int bpm = jpeg_blocks_per_mcu(L), nblk = sg.nmcu * bpm;
    for (int blk = 0; blk < nblk; ++blk) {
        int c, bx, by, m;
        jpeg_scan_block(L, sg.mcu0 * bpm + blk, &c, &bx, &by, &m);
        const int64_t at = jpeg_block_at(L, c, bx, by);
        s_blk[lane] = 0;
        __syncthreads();
        if (lane == 0 && !err) {
            int32_t pred = s_pred[c];
            err = jpeg_decode_block(bits, s_tab[im->dcs[c]], s_tab[im->acs[c]], &pred, s_blk);
            s_pred[c] = pred;
            if (err) s_err = err;
            else s_pos = bits.pos;
        }
        __syncthreads();
        coef[at + lane] = s_err ? (int16_t)0 : s_blk[lane];
        const int64_t pos = s_pos;
        if (pos - win >= JPEG_HALF) {                                 // uniform: the half behind the reader is replaced
            win += JPEG_HALF;
            for (int i = lane; i < JPEG_HALF / 4; i += 64) {
                const int64_t off = win + JPEG_HALF + 4 * i;
                s_ring[(off >> 2) & (JPEG_RING / 4 - 1)] = off < sg.end ? data32[off >> 2] : 0u;
            }
        }
        __syncthreads();
    }
    if (lane == 0 && err) atomicOr(errw + sg.image, 1 << (err - 1));
}

__global__ __launch_bounds__(64) void k_jpeg_idct(const JpegImg* __restrict__ imgs, const uint16_t* __restrict__ quant,
                                                  const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
    const JpegImg* im = imgs + blockIdx.y;
    const JpegLayout& L = im->L;
    int c, bx, by;
    int64_t k;
    if (!jpeg_plane_find(L, (int64_t)blockIdx.x * 64 + threadIdx.x, &c, &k)) return;
    uint32_t ws[8][8];
    for (int x = 0; x < 8; ++x) {
        uint32_t col[8];
        jpeg_idct_column(coef + L.coef[c] + 64 * k, quant + 64 * im->q[c], x, col);
        for (int v = 0; v < 8; ++v) ws[v][x] = col[v];
    }
    jpeg_plane_place(L, c, k, &bx, &by);
    for (int y = 0; y < 8; ++y) {
        union { uint8_t b8[8]; uint2 u; } px;
        jpeg_idct_row(ws[y], px.b8);
        *(uint2*)(planes + L.plane[c] + ((int64_t)(by * 8 + y) * L.bw[c] + bx) * 8) = px.u;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_pixels(const JpegImg* __restrict__ imgs, const uint8_t* __restrict__ planes, int rgb,
                                                     uint8_t* __restrict__ out) {
    const JpegLayout& L = imgs[blockIdx.y].L;
    const int64_t npx = (int64_t)L.w * L.h, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    uint8_t px[3];
    jpeg_pixel(L, planes, (int)(i % L.w), (int)(i / L.w), rgb, px);
    uint8_t* o = out + 3 * ((int64_t)blockIdx.y * npx + i);
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
}

// what a call is made of: the header walk of every image and the tables the kernels read
struct JpegPlan {
    std::vector<JpegImg> imgs;
    std::vector<JpegHuff> huffs;
    std::vector<uint16_t> quant;
    std::vector<JpegSeg> segs;
    int64_t n_coef = 0, n_plane = 0, max_blocks = 0;
    int w = 0, h = 0;
};

// J1, J2, J8 for the n streams of a call
int jpeg_plan(const char* fn, int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, JpegPlan* pl) {
    if (n < 1) return bad(fn, "need n >= 1");
    if (!offsets || !data) return bad(fn, "offsets or data is NULL");
    if (flags & ~(uint32_t)MVS_JPEG_RGB) return bad(fn, "unknown flag bits");
    int rc = check_offsets(fn, "offsets", offsets, n);
    if (rc) return rc;
    std::vector<JpegHeader> hd((size_t)n);
    std::vector<char> ok((size_t)n, 0);
    const int nt = io_threads(n, offsets[n]);
    parallel_parts(nt, [&](int t) {
        for (int i = t; i < n; i += nt) ok[(size_t)i] = jpeg_parse(data + offsets[i], offsets[i + 1] - offsets[i], &hd[(size_t)i]);
    });
    for (int i = 0; i < n; ++i)
        if (!ok[(size_t)i]) { mvs_set_error("%s: image %d: %s", fn, i, hd[(size_t)i].why.c_str()); return MVS_E_IO; }
    pl->w = hd[0].w; pl->h = hd[0].h;
    for (int i = 1; i < n; ++i)
        if (hd[(size_t)i].w != pl->w || hd[(size_t)i].h != pl->h) {
            mvs_set_error("%s: image %d is %d x %d, image 0 is %d x %d: the images of a call must share one size", fn, i, hd[(size_t)i].w,
                          hd[(size_t)i].h, pl->w, pl->h);
            return MVS_E_INVALID_ARG;
        }
    pl->imgs.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const JpegHeader& H = hd[(size_t)i];
        JpegImg& im = pl->imgs[(size_t)i];
        memset(&im, 0, sizeof im);
        int64_t nc = 0, np = 0;
        im.L = jpeg_layout(H, pl->n_coef, pl->n_plane, &nc, &np);
        pl->n_coef += nc; pl->n_plane += np;
        pl->max_blocks = std::max(pl->max_blocks, nc / 64);
        int cls[6], ids[6];
        for (int c = 0; c < H.ncomp; ++c) {
            im.q[c] = (int32_t)(pl->quant.size() / 64);
            pl->quant.insert(pl->quant.end(), H.quant[c], H.quant[c] + 64);
            for (int k = 0; k < 2; ++k) {                             // k = 0: the DC table, 1: the AC table
                const int id = k ? H.ac_id[c] : H.dc_id[c];
                int s = 0;
                while (s < im.ntab && !(cls[s] == k && ids[s] == id)) ++s;
                if (s == im.ntab) {
                    cls[s] = k; ids[s] = id;
                    im.tab[s] = (int32_t)pl->huffs.size();
                    pl->huffs.push_back(k ? H.ac[c] : H.dc[c]);
                    ++im.ntab;
                }
                (k ? im.acs : im.dcs)[c] = s;
            }
        }
        for (JpegSeg s : H.segs) {
            s.image = i; s.first += offsets[i]; s.end += offsets[i];
            pl->segs.push_back(s);
        }
    }
    if (pl->segs.size() > 0x7fffffffu || (pl->max_blocks + 63) / 64 > 0x7fffffffLL || n > 65535)
        return bad(fn, "too many images or restart intervals for one launch (n <= 65535)");
    return MVS_OK;
}

// J4-J7, the one coefficients-to-pixels tail (jpeg_run; the round trip through jpeg_coef_to_pixels_dev): the dequantise / IDCT launch and
// the pixel launch on n images of w x h, max_blocks the largest block count of one.  planes: a byte per padded sample, allocated by the
// caller in front of its first launch (allocating here put the pool's fence on s between the entropy launch and these two: 0.041 ->
// 0.046 ms on the IDCT stage of the timed hook).  clk gets a mark behind each launch
int jpeg_pixels_tail(const JpegImg* imgs, const uint16_t* quant, const int16_t* coef, int32_t n, int64_t max_blocks, int w, int h, int rgb,
                     uint8_t* planes, uint8_t* out, StageClock& clk, hipStream_t s) {
    k_jpeg_idct<<<dim3((unsigned)((max_blocks + 63) / 64), (unsigned)n), dim3(64), 0, s>>>(imgs, quant, coef, planes);
    if (int rc = clk.mark(s)) return rc;
    k_jpeg_pixels<<<dim3((unsigned)(((int64_t)w * h + 255) / 256), (unsigned)n), dim3(256), 0, s>>>(imgs, planes, rgb, out);
    return clk.mark(s);
}

// upload, the three launch sets and the error words, complete on return; ms (may be NULL): upload, entropy, idct, pixels in milliseconds
int jpeg_run(const char* fn, const JpegPlan& pl, int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs_dev,
             hipStream_t s, double* ms) {
    const size_t bytes = (size_t)offsets[n], padded = (bytes + 3) / 4 * 4 + 4;
    Scratch ddata, dimg, dhuff, dquant, dseg, dcoef, dplane, derr;
    StageClock clk(ms != nullptr);
    int rc;
    const double t0 = now_ms();
    if ((rc = ddata.alloc(padded, s))) return rc;
    HIPCHK(hipMemsetAsync(ddata.as<uint8_t>() + padded - 8, 0, 8, s));
    HIPCHK(hipMemcpyAsync(ddata.p, data, bytes, hipMemcpyHostToDevice, s));
    if ((rc = up_async(dimg, pl.imgs.data(), pl.imgs.size(), s)) || (rc = up_async(dhuff, pl.huffs.data(), pl.huffs.size(), s)) ||
        (rc = up_async(dquant, pl.quant.data(), pl.quant.size(), s)) || (rc = up_async(dseg, pl.segs.data(), pl.segs.size(), s)) ||
        (rc = dcoef.alloc(sizeof(int16_t) * (size_t)pl.n_coef, s)) || (rc = dplane.alloc((size_t)pl.n_plane, s)) ||
        (rc = derr.alloc(sizeof(int32_t) * (size_t)n, s))) return rc;
    HIPCHK(hipMemsetAsync(derr.p, 0, sizeof(int32_t) * (size_t)n, s));
    if (ms) {
        HIPCHK(hipStreamSynchronize(s));
        ms[0] = now_ms() - t0;
    }
    if ((rc = clk.mark(s))) return rc;
    k_jpeg_entropy<<<dim3((unsigned)pl.segs.size()), dim3(64), 0, s>>>(dseg.as<JpegSeg>(), dimg.as<JpegImg>(), dhuff.as<JpegHuff>(),
                                                                        ddata.as<uint32_t>(), dcoef.as<int16_t>(), derr.as<int32_t>());
    if ((rc = clk.mark(s)) || (rc = jpeg_pixels_tail(dimg.as<JpegImg>(), dquant.as<uint16_t>(), dcoef.as<int16_t>(), n, pl.max_blocks, pl.w, pl.h,
                                                     (int)(flags & MVS_JPEG_RGB), dplane.as<uint8_t>(), imgs_dev, clk, s))) return rc;
    HIPCHK(hipGetLastError());
    std::vector<int32_t> err((size_t)n);
    HIPCHK(hipMemcpyAsync(err.data(), derr.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ms && (rc = clk.read(ms + 1))) return rc;
    for (int i = 0; i < n; ++i)
        if (err[(size_t)i]) {
            int e = 1;
            while (!(err[(size_t)i] >> (e - 1) & 1)) ++e;
            mvs_set_error("%s: image %d: %s", fn, i, jpeg_scan_error(e));
            return MVS_E_IO;
        }
    return MVS_OK;
}

}  // namespace

// mvs_jpeg_decode under the name fn; w / h (may be NULL) receive the size; imgs == NULL: the walk and the checks only
int jpeg_decode_host(const char* fn, int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs, int32_t* w, int32_t* h) {
    JpegPlan pl;
    int rc = jpeg_plan(fn, n, offsets, data, flags, &pl);
    if (rc) return rc;
    if (w) *w = pl.w;
    if (h) *h = pl.h;
    if (!imgs) return MVS_OK;
    if ((rc = need_device())) return rc;
    const size_t nb = (size_t)n * (size_t)pl.w * (size_t)pl.h * 3;
    Scratch dout;
    if ((rc = dout.alloc(nb)) || (rc = jpeg_run(fn, pl, n, offsets, data, flags, dout.as<uint8_t>(), nullptr, nullptr))) return rc;
    return down(imgs, dout, nb);
}

// the round trip of jpeg_enc.hip: the table of n images of layout L (blocks and planes from 0), image i's blocks at i * n_coef, then
// jpeg_pixels_tail.  Synchronises s
int jpeg_coef_to_pixels_dev(int32_t n, const JpegLayout& L, int64_t n_coef, const uint16_t* q_luma, const uint16_t* q_chroma, const int16_t* coef_dev,
                            int rgb, uint8_t* imgs_dev, hipStream_t s) {
    std::vector<JpegImg> imgs((size_t)n);
    for (int i = 0; i < n; ++i) {
        JpegImg& im = imgs[(size_t)i];
        memset(&im, 0, sizeof im);
        im.L = L;
        for (int c = 0; c < 3; ++c) { im.L.coef[c] += i * n_coef; im.L.plane[c] += i * n_coef; im.q[c] = c ? 1 : 0; }
    }
    std::vector<uint16_t> quant(q_luma, q_luma + 64);
    quant.insert(quant.end(), q_chroma, q_chroma + 64);
    Scratch dimg, dquant, dplane;
    StageClock off(false);
    int rc;
    if ((rc = up_async(dimg, imgs.data(), imgs.size(), s)) || (rc = up_async(dquant, quant.data(), quant.size(), s)) ||
        (rc = dplane.alloc((size_t)n_coef * (size_t)n, s)) ||
        (rc = jpeg_pixels_tail(dimg.as<JpegImg>(), dquant.as<uint16_t>(), coef_dev, n, n_coef / 64, L.w, L.h, rgb, dplane.as<uint8_t>(), imgs_dev, off, s))) return rc;
    HIPCHK(hipGetLastError());
    return mvs_check_hip(hipStreamSynchronize(s), "jpeg_coef_to_pixels_dev");
}

// mvs_jpeg_decode_dev under the name fn; ms (NULL: not timed): the header walk, then jpeg_run's four, in milliseconds
static int jpeg_decode_dev(const char* fn, int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs_dev, void* hip_stream,
                           double* ms) {
    JpegPlan pl;
    const double t0 = now_ms();
    int rc = jpeg_plan(fn, n, offsets, data, flags, &pl);
    if (ms) ms[0] = now_ms() - t0;
    if (rc || (rc = need_device())) return rc;
    return jpeg_run(fn, pl, n, offsets, data, flags, imgs_dev, (hipStream_t)hip_stream, ms ? ms + 1 : nullptr);
}

extern "C" {

int mvs_jpeg_info(const uint8_t* data, int64_t len, mvs_jpeg_info_t* out) {
    MVS_TRACE();
    if (!data || !out || len < 0) return bad(__func__, "data or out is NULL, or len is negative");
    JpegHeader H;
    if (!jpeg_parse(data, len, &H)) { mvs_set_error("%s: image 0: %s", __func__, H.why.c_str()); return MVS_E_IO; }
    *out = mvs_jpeg_info_t{H.w, H.h, H.ncomp, H.hs[0], H.vs[0], H.restart, (int32_t)H.segs.size(), H.sof};
    return MVS_OK;
}

int mvs_jpeg_decode(int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs) {
    MVS_TRACE();
    if (!imgs) return bad(__func__, "imgs is NULL");
    return jpeg_decode_host(__func__, n, offsets, data, flags, imgs, nullptr, nullptr);
}

int mvs_jpeg_decode_dev(int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs_dev, void* hip_stream) {
    MVS_TRACE();
    if (!imgs_dev) return bad(__func__, "imgs_dev is NULL");
    return jpeg_decode_dev(__func__, n, offsets, data, flags, imgs_dev, hip_stream, nullptr);
}

int mvs_test_jpeg_decode_timed(int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs_dev, void* hip_stream,
                               double* ms) {
    if (!ms || !imgs_dev) return bad(__func__, "ms or imgs_dev is NULL");
    return jpeg_decode_dev(__func__, n, offsets, data, flags, imgs_dev, hip_stream, ms);
}

}  // extern "C"
