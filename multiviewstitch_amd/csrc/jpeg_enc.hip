// jpeg_enc.hip — mvs_jpeg_encode(_dev), mvs_jpeg_roundtrip(_dev), mvs_depth_preview(_dev) (include/mvs.h): the batched baseline JPEG
// encoder, rules E1-E9 (jpeg_enc_rules.h).  The headers are host code, identical within a call.  Every launch covers all images:
//
//   k_je_transform ONE launch, a lane per coefficient block of the padded planes (JpegLayout, as the decoder's): E2-E5.  The lane
//                  gathers its 64 samples (colour, edge repeat and downsampling on the way), runs the row and the column pass of E4 with
//                  the workspace in registers and writes the quantised block as eight 16-byte stores.  Dummy blocks (E6) are zeros.
//   entropy        k_je_bits: a lane per scan block, its bit count; the DC predecessor is read from the coefficient array.  A scan over
//                  all blocks of the call.  k_je_intervals: bytes per restart interval (or whole scan); a scan over the intervals gives
//                  each one a byte-aligned start in the unstuffed buffer.  k_je_write: a lane per scan block puts its bits at their bit
//                  offset, whole 32-bit words with atomicOr into the zeroed buffer (an OR commutes: the bytes do not depend on the
//                  order), the interval's last lane fills the last byte with 1 bits.  A scan without restart markers is one interval and
//                  goes through the same lanes: nothing is serial in it.
//   stuffing       k_je_ffcount: FF bytes per chunk of 1024 unstuffed bytes; a scan; k_je_offsets: a wave per image, the stream
//                  offsets (E9) — the host reads them and checks the capacity before anything is written to the output;
//                  k_je_stuff: a lane per four unstuffed bytes writes them at their final place, FF followed by 00; the lane that holds
//                  an interval's last byte writes RSTn or EOI behind it.  k_je_headers copies the header in front of every scan.
//   k_dp_range / k_dp_write: mvs_depth_preview, min / max of the valid depths by atomicMin / atomicMax on the bits of the non-negative
//                  floats (order-free), then a lane per pixel.
//
// mvs_test_jpeg_encode_coef (include/mvs_test.h) uploads coefficient blocks of its caller's choice in place of k_je_transform's output and
// runs everything behind it (je_entropy), which the production entries run after their transform launch.
//
// Stream positions come from scans only; two runs give the same bytes.  The scans are scan_dev.h's, as grid.hip's; which block a lane
// is at comes from the walks of jpeg_rules.h, as in the decoder; the round trip ends in the decoder's jpeg_pixels_tail (jpeg.hip).
#include "engine.h"
#include "trace.h"
#include "jpeg_enc_rules.h"
#include "frontend_dev.h"
#include "scan_dev.h"
#include "../../include/mvs_test.h"
#include "stitch.h"

namespace {

constexpr int JE_TPB = 256, JE_TILE = JE_TPB * 4;   // the stuffing chunk in bytes: four per lane

struct JeCall {                        // what every kernel of a call reads
    JpegLayout L;                      // of one image; image i's blocks start at i * n_coef
    JpegEncPixels px;                  // px.px: image 0; image i at + i * img_bytes
    int64_t n_coef, img_bytes, nblk, n_int;   // int16 and bytes per image, scan blocks per image, intervals of the call
    int32_t n, per, nint, hdr;         // images, MCUs per interval, intervals per image, header bytes
};

// exclusive scan of 256 values, one per thread; *total: their sum.  Not scan_dev.h's: k_je_ffcount and k_je_stuff scan the FF counts of
// one chunk inside the workgroup that holds the chunk and never leave it
__device__ inline uint64_t wg_excl_scan(uint64_t v, uint64_t* s_buf /*[JE_TPB]*/, uint64_t* total) {
    const int t = threadIdx.x;
    s_buf[t] = v;
    __syncthreads();
    for (int o = 1; o < JE_TPB; o <<= 1) {
        const uint64_t add = t >= o ? s_buf[t - o] : 0;
        __syncthreads();
        s_buf[t] += add;
        __syncthreads();
    }
    const uint64_t incl = s_buf[t];
    *total = s_buf[JE_TPB - 1];
    __syncthreads();
    return incl - v;
}


// ------------------------------------------------------------------ transform ----
__global__ __launch_bounds__(64) void k_je_transform(JeCall cl, const uint16_t* __restrict__ quant /*[2][64]*/, int16_t* __restrict__ coef) {
    const JpegLayout& L = cl.L;
    int c, bx, by;
    int64_t k;
    if (!jpeg_plane_block(L, (int64_t)blockIdx.x * 64 + threadIdx.x, &c, &bx, &by, &k)) return;
    union { int16_t v[64]; uint4 q[8]; } blk;
    if (jpeg_enc_dummy(L, c, bx, by)) {
        for (int k = 0; k < 8; ++k) blk.q[k] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        JpegEncPixels px = cl.px;
        px.px += (int64_t)blockIdx.y * cl.img_bytes;
        jpeg_enc_block(L, px, c, bx, by, quant + (c ? 64 : 0), blk.v);
    }
    uint4* o = (uint4*)(coef + (int64_t)blockIdx.y * cl.n_coef + L.coef[c] + 64 * k);
    for (int k = 0; k < 8; ++k) o[k] = blk.q[k];
}

// ------------------------------------------------------------------ entropy ----
// scan block j of the call -> its image, and through blk / pred / c what jpeg_enc_block_bits takes
struct JeBlock { const int16_t* blk; int32_t pred; int c; int jj; };
__device__ inline JeBlock je_block(const JeCall& cl, const int16_t* __restrict__ coef, int64_t j) {
    const int64_t img = j / cl.nblk;
    const int jj = (int)(j % cl.nblk);
    const int16_t* ic = coef + img * cl.n_coef;
    int c, bx, by, m;
    jpeg_scan_block(cl.L, jj, &c, &bx, &by, &m);
    if (jpeg_enc_dummy(cl.L, c, bx, by)) return JeBlock{nullptr, 0, c, jj};
    return JeBlock{ic + jpeg_block_at(cl.L, c, bx, by), jpeg_enc_pred(cl.L, ic, jj, c, cl.per), c, jj};
}

__global__ __launch_bounds__(JE_TPB) void k_je_bits(JeCall cl, const JpegEncTables* __restrict__ T, const int16_t* __restrict__ coef,
                                                    uint32_t* __restrict__ bits) {
    const int64_t j = (int64_t)blockIdx.x * JE_TPB + threadIdx.x;
    if (j >= cl.nblk * cl.n) return;
    const JeBlock B = je_block(cl, coef, j);
    JpegEncCount cnt;
    jpeg_enc_block_bits(B.blk, B.pred, T->dc[B.c ? 1 : 0], T->ac[B.c ? 1 : 0], cnt);
    bits[j] = cnt.bits;
}

// first and one-past-last scan block (of the call) of interval t (of the call)
__device__ inline void je_interval(const JeCall& cl, int64_t t, int64_t* a, int64_t* b) {
    const int64_t img = t / cl.nint, tl = t % cl.nint;
    const int64_t bpm = jpeg_blocks_per_mcu(cl.L);
    const int64_t first = tl * cl.per * bpm, end = first + (int64_t)cl.per * bpm;
    *a = img * cl.nblk + first;
    *b = img * cl.nblk + (end < cl.nblk ? end : cl.nblk);
}

__global__ __launch_bounds__(JE_TPB) void k_je_intervals(JeCall cl, const uint64_t* __restrict__ bit_at, uint32_t* __restrict__ ibytes) {
    const int64_t t = (int64_t)blockIdx.x * JE_TPB + threadIdx.x;
    if (t >= cl.n_int) return;
    int64_t a, b;
    je_interval(cl, t, &a, &b);
    ibytes[t] = (uint32_t)((bit_at[b] - bit_at[a] + 7) / 8);
}

struct JeBitWriter {                   // the sink that writes: bits MSB first into the bytes behind `words`
    uint32_t* words;
    uint64_t pos;                      // bit position in the buffer
    uint32_t cur;                      // the bits of word pos / 32 this lane has produced, the first bit on top
    __device__ void flush() {
        if (cur) atomicOr(words + (pos >> 5), __builtin_bswap32(cur));
        cur = 0u;
    }
    __device__ void put(uint32_t v, int n) {
        const int room = 32 - (int)(pos & 31);
        if (n < room) cur |= v << (room - n);
        else {
            cur |= v >> (n - room);
            flush();
            if (n > room) cur = v << (32 - (n - room));
        }
        pos += (uint64_t)n;
    }
};

__global__ __launch_bounds__(JE_TPB) void k_je_write(JeCall cl, const JpegEncTables* __restrict__ T, const int16_t* __restrict__ coef,
                                                     const uint64_t* __restrict__ bit_at, const uint64_t* __restrict__ ibyte_at,
                                                     uint32_t* __restrict__ raw) {
    const int64_t j = (int64_t)blockIdx.x * JE_TPB + threadIdx.x;
    if (j >= cl.nblk * cl.n) return;
    const JeBlock B = je_block(cl, coef, j);
    const int64_t t = j / cl.nblk * cl.nint + B.jj / ((int64_t)cl.per * jpeg_blocks_per_mcu(cl.L));
    int64_t a, b;
    je_interval(cl, t, &a, &b);
    JeBitWriter w{raw, 8u * ibyte_at[t] + (bit_at[j] - bit_at[a]), 0u};
    jpeg_enc_block_bits(B.blk, B.pred, T->dc[B.c ? 1 : 0], T->ac[B.c ? 1 : 0], w);
    if (j == b - 1 && (w.pos & 7)) {                                  // E7: the interval's last byte is filled with 1 bits
        const int k = 8 - (int)(w.pos & 7);
        w.put((1u << k) - 1u, k);
    }
    w.flush();
}

// ------------------------------------------------------------------ stuffing ----
__device__ inline int ff_in_word(uint32_t w, int nbytes) {
    int c = 0;
    for (int k = 0; k < nbytes; ++k) c += ((w >> (8 * k)) & 255u) == 255u;
    return c;
}
__global__ __launch_bounds__(JE_TPB) void k_je_ffcount(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ ibyte_at, int64_t n_int,
                                                       uint32_t* __restrict__ cnt) {
    __shared__ uint64_t s_buf[JE_TPB];
    const int64_t total = (int64_t)ibyte_at[n_int], p = ((int64_t)blockIdx.x * JE_TPB + threadIdx.x) * 4;
    const int nb = p >= total ? 0 : total - p < 4 ? (int)(total - p) : 4;
    uint64_t sum;
    wg_excl_scan((uint64_t)(nb ? ff_in_word(raw[p >> 2], nb) : 0), s_buf, &sum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = (uint32_t)sum;
}
// bytes the stream of image `img` holds in front of the unstuffed bytes of its interval tl, beyond those and their stuffing: the headers
// up to its own, the EOIs of the images before it and the RSTn markers before the interval
__device__ inline int64_t je_extra(const JeCall& cl, int64_t img, int64_t tl) {
    return (img + 1) * cl.hdr + 2 * img + 2 * (img * (cl.nint - 1) + tl);
}
// a wave per image: offsets[img + 1]; lane 0 of image 0 also offsets[0]
__global__ __launch_bounds__(64) void k_je_offsets(JeCall cl, const uint8_t* __restrict__ raw, const uint64_t* __restrict__ ibyte_at,
                                                   const uint64_t* __restrict__ ff_at, int64_t* __restrict__ offsets) {
    const int64_t img = blockIdx.x, x = (int64_t)ibyte_at[(img + 1) * cl.nint], chunk = x / JE_TILE;
    int c = 0;
    for (int64_t p = chunk * JE_TILE + threadIdx.x; p < x; p += 64) c += raw[p] == 255;
    for (int o = 32; o; o >>= 1) c += __shfl_down(c, o, 64);
    if (threadIdx.x == 0) {
        const int64_t ff = (int64_t)ff_at[chunk] + c;                 // chunk <= the chunk count: ff_at has one entry more
        offsets[img + 1] = x + ff + je_extra(cl, img, cl.nint - 1) + 2;
        if (img == 0) offsets[0] = 0;
    }
}
__global__ __launch_bounds__(JE_TPB) void k_je_stuff(JeCall cl, const uint32_t* __restrict__ raw, const uint64_t* __restrict__ ibyte_at,
                                                     const uint64_t* __restrict__ ff_at, uint8_t* __restrict__ out) {
    __shared__ uint64_t s_buf[JE_TPB];
    const int64_t total = (int64_t)ibyte_at[cl.n_int], p0 = ((int64_t)blockIdx.x * JE_TPB + threadIdx.x) * 4;
    const int nb = p0 >= total ? 0 : total - p0 < 4 ? (int)(total - p0) : 4;
    const uint32_t w = nb ? raw[p0 >> 2] : 0u;
    uint64_t sum;
    int64_t ff = (int64_t)(ff_at[blockIdx.x] + wg_excl_scan((uint64_t)(nb ? ff_in_word(w, nb) : 0), s_buf, &sum));
    if (!nb) return;
    int64_t t = segment_of((const int64_t*)ibyte_at, (int)cl.n_int, p0);
    for (int k = 0; k < nb; ++k) {
        const int64_t p = p0 + k;
        while (p >= (int64_t)ibyte_at[t + 1]) ++t;
        const int64_t img = t / cl.nint, tl = t % cl.nint;
        const uint32_t b = (w >> (8 * k)) & 255u;
        int64_t at = p + ff + je_extra(cl, img, tl);
        out[at++] = (uint8_t)b;
        if (b == 255u) { out[at++] = 0; ++ff; }
        if (p + 1 == (int64_t)ibyte_at[t + 1]) {                      // the interval's last byte: RSTn, or EOI behind the image's last
            out[at] = 0xFF;
            out[at + 1] = (uint8_t)(tl + 1 < cl.nint ? 0xD0 + (tl & 7) : 0xD9);
        }
    }
}
__global__ __launch_bounds__(JE_TPB) void k_je_headers(const uint8_t* __restrict__ hdr, int n_hdr, const int64_t* __restrict__ offsets,
                                                       uint8_t* __restrict__ out) {
    for (int i = threadIdx.x; i < n_hdr; i += JE_TPB) out[offsets[blockIdx.x] + i] = hdr[i];
}

// ------------------------------------------------------------------ depth preview ----
__device__ inline bool dp_valid(float d) { return d >= 0.f && d < INFINITY; }
__global__ __launch_bounds__(JE_TPB) void k_dp_range(const float* __restrict__ depths, int64_t npx, uint32_t* __restrict__ range /*[n][2]*/) {
    const float* d = depths + (int64_t)blockIdx.y * npx;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * JE_TPB + threadIdx.x; i < npx; i += (int64_t)gridDim.x * JE_TPB)
        if (dp_valid(d[i])) {
            const uint32_t u = __float_as_uint(fabsf(d[i]));        // -0 counts as 0; the bits of non-negative floats order as the floats do
            lo = u < lo ? u : lo;
            hi = u > hi ? u : hi;
        }
    for (int o = 32; o; o >>= 1) {
        const uint32_t l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo != 0xFFFFFFFFu) {
        atomicMin(range + 2 * blockIdx.y, lo);
        atomicMax(range + 2 * blockIdx.y + 1, hi);
    }
}
__global__ __launch_bounds__(JE_TPB) void k_dp_write(const float* __restrict__ depths, int64_t npx, const uint32_t* __restrict__ range,
                                                     uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * JE_TPB + threadIdx.x;
    if (i >= npx) return;
    const float d = depths[(int64_t)blockIdx.y * npx + i];
    const double lo = (double)__uint_as_float(range[2 * blockIdx.y]), hi = (double)__uint_as_float(range[2 * blockIdx.y + 1]);
    uint8_t v = 255;
    if (dp_valid(d)) v = hi == lo ? (uint8_t)0 : (uint8_t)(int32_t)(255.0 * ((double)d - lo) / (hi - lo));
    out[(int64_t)blockIdx.y * npx + i] = v;
}

// ------------------------------------------------------------------ host ----
struct JePlan {
    JpegEncShape S;
    JpegEncTables T;
    JeCall cl;
    std::vector<uint8_t> hdr;
    uint32_t flags;
};

// E1
int je_plan(const char* fn, int32_t n, int32_t w, int32_t h, uint32_t flags, const mvs_jpeg_encode_params* p, JePlan* pl) {
    if (n < 1 || n > 65535) return bad(fn, "need n in 1 .. 65535");
    if (flags & ~(uint32_t)(MVS_JPEG_RGB | MVS_JPEG_GREY)) return bad(fn, "unknown flag bits");
    mvs_jpeg_encode_params d;
    mvs_jpeg_encode_default_params(&d);
    if (!p) p = &d;
    const bool grey = flags & MVS_JPEG_GREY;
    if (const char* why = jpeg_enc_shape(w, h, grey, p->quality, p->sampling, p->restart_interval, &pl->S)) return bad(fn, why);
    const JpegEncShape& S = pl->S;
    if (S.nblk * n > 0x7fffffffLL * 64 || (int64_t)S.nint * n > 0x7fffffffLL)          // a launch of 256 lanes per workgroup covers the blocks
        return bad(fn, "too many blocks or restart intervals for one call");
    jpeg_enc_make_tables(S.quality, &pl->T);
    pl->hdr = jpeg_enc_header(w, h, S.ncomp, S.hmax, S.vmax, pl->T, S.restart);
    pl->flags = flags;
    JeCall& cl = pl->cl;
    memset(&cl, 0, sizeof cl);
    cl.L = jpeg_enc_layout(w, h, S.ncomp, S.hmax, S.vmax, &cl.n_coef);
    cl.px = JpegEncPixels{nullptr, w, h, grey ? 1 : 3, (int32_t)(flags & MVS_JPEG_RGB)};
    cl.img_bytes = (int64_t)w * h * cl.px.chan;
    cl.nblk = S.nblk; cl.n = n; cl.per = S.per; cl.nint = S.nint; cl.n_int = (int64_t)S.nint * n; cl.hdr = (int32_t)pl->hdr.size();
    return MVS_OK;
}

// E9: the streams of a call against the caller's capacity
int je_fits(const char* fn, int64_t total, int64_t capacity) {
    if (total <= capacity) return MVS_OK;
    mvs_set_error("%s: the streams take %lld bytes, capacity is %lld (offsets is written)", fn, (long long)total, (long long)capacity);
    return MVS_E_INVALID_ARG;
}

struct JeCoef { Scratch tab, coef; };
// the tables of the call in HBM and room for its coefficient blocks
int je_coef_alloc(JePlan& pl, JeCoef* c, hipStream_t s) {
    int rc = up_async(c->tab, &pl.T, 1, s);
    return rc ? rc : c->coef.alloc(sizeof(int16_t) * (size_t)pl.cl.n_coef * (size_t)pl.cl.n, s);
}
// the transform launch on the pixels at imgs_dev
int je_transform(JePlan& pl, const uint8_t* imgs_dev, JeCoef* c, hipStream_t s) {
    int rc;
    if ((rc = je_coef_alloc(pl, c, s))) return rc;
    pl.cl.px.px = imgs_dev;
    const int64_t nb = pl.cl.n_coef / 64;
    k_je_transform<<<dim3((unsigned)((nb + 63) / 64), (unsigned)pl.cl.n), dim3(64), 0, s>>>(pl.cl, &c->tab.as<JpegEncTables>()->quant[0][0],
                                                                                           c->coef.as<int16_t>());
    return mvs_check_hip(hipGetLastError(), "k_je_transform");
}

// Everything behind the transform, on the coefficient blocks c its caller made (k_je_transform's, or mvs_test_jpeg_encode_coef's upload):
// bits, scans, intervals, write, FF count, offsets, stuffing, headers.  clk: the caller's clock with the marks around the transform set;
// the other arguments are je_run's.  Complete on return
int je_entropy(const char* fn, const JePlan& pl, const JeCoef& c, StageClock& clk, int64_t* offsets, uint8_t* data_dev, int64_t capacity, Scratch* own,
               hipStream_t s, double* ms) {
    const JeCall& cl = pl.cl;
    const int64_t N = cl.nblk * cl.n, NI = cl.n_int;
    Scratch dbits, dbit_at, dpart, dpart2, dibytes, dibyte_at, draw, dcnt, dff_at, doff, dhdr;
    int rc;
    if ((rc = dbits.alloc(4 * (size_t)N, s)) || (rc = dbit_at.alloc(8 * (size_t)(N + 1), s)) ||
        (rc = dpart.alloc(8 * (size_t)((N + JE_TILE - 1) / JE_TILE + 2), s)) || (rc = dibytes.alloc(4 * (size_t)NI, s)) ||
        (rc = dibyte_at.alloc(8 * (size_t)(NI + 1), s)) || (rc = doff.alloc(8 * (size_t)(cl.n + 1), s)) ||
        (rc = up_async(dhdr, pl.hdr.data(), pl.hdr.size(), s))) return rc;
    const JpegEncTables* T = c.tab.as<JpegEncTables>();
    k_je_bits<<<dim3((unsigned)((N + JE_TPB - 1) / JE_TPB)), dim3(JE_TPB), 0, s>>>(cl, T, c.coef.as<int16_t>(), dbits.as<uint32_t>());
    scan_exclusive_async(dbits.as<uint32_t>(), N, dbit_at.as<uint64_t>(), dpart.as<uint64_t>(), s);
    k_je_intervals<<<dim3((unsigned)((NI + JE_TPB - 1) / JE_TPB)), dim3(JE_TPB), 0, s>>>(cl, dbit_at.as<uint64_t>(), dibytes.as<uint32_t>());
    scan_exclusive_async(dibytes.as<uint32_t>(), NI, dibyte_at.as<uint64_t>(), dpart.as<uint64_t>(), s);
    uint64_t raw_bytes = 0;                                           // the unstuffed bytes of the call: the buffer is sized from them
    HIPCHK(hipMemcpyAsync(&raw_bytes, dibyte_at.as<uint64_t>() + NI, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const size_t raw_alloc = ((size_t)raw_bytes + 3) / 4 * 4 + 4;
    const int64_t nchunk = ((int64_t)raw_bytes + JE_TILE - 1) / JE_TILE;
    if ((rc = draw.alloc(raw_alloc, s)) || (rc = dcnt.alloc(4 * (size_t)nchunk, s)) || (rc = dff_at.alloc(8 * (size_t)(nchunk + 1), s)) ||
        (rc = dpart2.alloc(8 * (size_t)((nchunk + JE_TILE - 1) / JE_TILE + 2), s))) return rc;
    HIPCHK(hipMemsetAsync(draw.p, 0, raw_alloc, s));
    k_je_write<<<dim3((unsigned)((N + JE_TPB - 1) / JE_TPB)), dim3(JE_TPB), 0, s>>>(cl, T, c.coef.as<int16_t>(), dbit_at.as<uint64_t>(),
                                                                                     dibyte_at.as<uint64_t>(), draw.as<uint32_t>());
    if ((rc = clk.mark(s))) return rc;
    k_je_ffcount<<<dim3((unsigned)nchunk), dim3(JE_TPB), 0, s>>>(draw.as<uint32_t>(), dibyte_at.as<uint64_t>(), NI, dcnt.as<uint32_t>());
    scan_exclusive_async(dcnt.as<uint32_t>(), nchunk, dff_at.as<uint64_t>(), dpart2.as<uint64_t>(), s);
    k_je_offsets<<<dim3((unsigned)cl.n), dim3(64), 0, s>>>(cl, draw.as<uint8_t>(), dibyte_at.as<uint64_t>(), dff_at.as<uint64_t>(), doff.as<int64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(offsets, doff.p, 8 * (size_t)(cl.n + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t total = offsets[cl.n];
    if (data_dev && (rc = je_fits(fn, total, capacity))) return rc;
    if (!data_dev) {
        if ((rc = own->alloc((size_t)total, s))) return rc;
        data_dev = own->as<uint8_t>();
    }
    k_je_stuff<<<dim3((unsigned)nchunk), dim3(JE_TPB), 0, s>>>(cl, draw.as<uint32_t>(), dibyte_at.as<uint64_t>(), dff_at.as<uint64_t>(), data_dev);
    k_je_headers<<<dim3((unsigned)cl.n), dim3(JE_TPB), 0, s>>>(dhdr.as<uint8_t>(), cl.hdr, doff.as<int64_t>(), data_dev);
    if ((rc = clk.mark(s))) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return ms ? clk.read(ms) : MVS_OK;
}

// The call on pixels in HBM.  offsets: host, written before the capacity is checked.  data_dev != NULL: the streams go there (capacity
// bytes); else `own` receives a block of offsets[n] bytes that holds them.  ms (may be NULL): transform, entropy, stuffing in milliseconds.
// Complete on return
int je_run(const char* fn, JePlan& pl, const uint8_t* imgs_dev, int64_t* offsets, uint8_t* data_dev, int64_t capacity, Scratch* own, hipStream_t s,
           double* ms) {
    JeCoef c;
    StageClock clk(ms != nullptr);
    int rc;
    if ((rc = clk.mark(s)) || (rc = je_transform(pl, imgs_dev, &c, s)) || (rc = clk.mark(s))) return rc;
    return je_entropy(fn, pl, c, clk, offsets, data_dev, capacity, own, s, ms);
}

// E7's symbols end at size 11 for a DC difference and at size 10 for an AC value: NULL, or the first value of the real blocks of n
// images (coef as JpegLayout places them) that jpeg_enc_block_bits has no code for, with its place in *at
const int16_t* je_coef_range(const JeCall& cl, const int16_t* coef, int64_t* at) {
    const JpegLayout& L = cl.L;
    for (int64_t img = 0; img < cl.n; ++img)
        for (int c = 0; c < L.ncomp; ++c)
            for (int by = 0; by < L.bh[c]; ++by)
                for (int bx = 0; bx < L.bw[c]; ++bx) {
                    if (jpeg_enc_dummy(L, c, bx, by)) continue;                 // E6: nothing reads them
                    const int64_t b = img * cl.n_coef + jpeg_block_at(L, c, bx, by);
                    for (int k = 0; k < 64; ++k) {
                        const int v = coef[b + k];
                        if (v > 1023 || v < (k ? -1023 : -1024)) { *at = b + k; return coef + b + k; }
                    }
                }
    return nullptr;
}

int je_check_ptrs(const char* fn, const void* imgs, const void* out) {
    if (!imgs) return bad(fn, "imgs is NULL");
    if (!out) return bad(fn, "the output is NULL");
    return MVS_OK;
}

int je_roundtrip(const char* fn, JePlan& pl, const uint8_t* imgs_dev, uint8_t* out_dev, hipStream_t s) {
    JeCoef c;
    int rc = je_transform(pl, imgs_dev, &c, s);
    if (rc) return rc;
    rc = jpeg_coef_to_pixels_dev(pl.cl.n, pl.cl.L, pl.cl.n_coef, pl.T.quant[0], pl.T.quant[1], c.coef.as<int16_t>(), pl.flags & MVS_JPEG_RGB, out_dev, s);
    if (rc) return rc;
    return mvs_check_hip(hipStreamSynchronize(s), fn);
}

int dp_run(int32_t n, int64_t npx, const float* depths_dev, uint8_t* out_dev, hipStream_t s) {
    Scratch drange;
    int rc = drange.alloc(8 * (size_t)n, s);
    if (rc) return rc;
    std::vector<uint32_t> init((size_t)n * 2);
    for (int i = 0; i < n; ++i) { init[2 * (size_t)i] = 0xFFFFFFFFu; init[2 * (size_t)i + 1] = 0u; }
    HIPCHK(hipMemcpyAsync(drange.p, init.data(), 8 * (size_t)n, hipMemcpyHostToDevice, s));
    const int64_t nb = (npx + JE_TPB - 1) / JE_TPB;
    k_dp_range<<<dim3((unsigned)(nb < 256 ? nb : 256), (unsigned)n), dim3(JE_TPB), 0, s>>>(depths_dev, npx, drange.as<uint32_t>());
    k_dp_write<<<dim3((unsigned)nb, (unsigned)n), dim3(JE_TPB), 0, s>>>(depths_dev, npx, drange.as<uint32_t>(), out_dev);
    HIPCHK(hipGetLastError());
    return mvs_check_hip(hipStreamSynchronize(s), "mvs_depth_preview");
}
int dp_check(const char* fn, int32_t n, int32_t w, int32_t h, const void* depths, const void* out) {
    if (n < 1 || n > 65535) return bad(fn, "need n in 1 .. 65535");
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return bad(fn, "w and h must be in 1 .. 65535");
    if (!depths || !out) return bad(fn, "depths or out is NULL");
    return MVS_OK;
}

// the host forms under the name fn: E1, the entry's own pointer check (ptrs: NULL, or what it found wrong), the call on an upload of
// imgs; the streams end in `dout`, a device block of offsets[n] bytes
int je_host(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p, const char* ptrs,
            int64_t* offsets, Scratch* dout) {
    JePlan pl;
    int rc = je_plan(fn, n, w, h, flags, p, &pl);
    if (rc) return rc;
    if (ptrs) return bad(fn, ptrs);
    if ((rc = need_device())) return rc;
    Scratch dimg;                                                     // the device block is sized from the streams, not from a capacity
    if ((rc = up(dimg, imgs, (size_t)pl.cl.img_bytes * (size_t)n))) return rc;
    return je_run(fn, pl, dimg.as<uint8_t>(), offsets, nullptr, 0, dout, nullptr, nullptr);
}

// mvs_jpeg_encode_dev under the name fn; ms (NULL: not timed): E1, then je_run's three, in milliseconds
int je_dev(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p, int64_t* offsets,
           uint8_t* data_dev, int64_t capacity, void* hip_stream, double* ms) {
    JePlan pl;
    const double t0 = now_ms();
    int rc = je_plan(fn, n, w, h, flags, p, &pl);
    if (ms) ms[0] = now_ms() - t0;
    if (rc) return rc;
    if (!imgs_dev || !offsets || !data_dev || capacity < 0) return bad(fn, "imgs_dev, offsets or data_dev is NULL, or capacity is negative");
    if ((rc = need_device())) return rc;
    return je_run(fn, pl, imgs_dev, offsets, data_dev, capacity, nullptr, (hipStream_t)hip_stream, ms ? ms + 1 : nullptr);
}

}  // namespace

// mvs_jpeg_encode's host form under the name fn with an output that sizes itself: data receives offsets[n] bytes
int jpeg_encode_host(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p,
                     int64_t* offsets, std::vector<uint8_t>* data) {
    Scratch dout;
    int rc = je_host(fn, n, w, h, imgs, flags, p, !imgs || !offsets ? "imgs or offsets is NULL" : nullptr, offsets, &dout);
    if (rc) return rc;
    data->resize((size_t)offsets[n]);
    return down(data->data(), dout, data->size());
}
int jpeg_encode_check(const char* fn, int32_t w, int32_t h, uint32_t flags, const mvs_jpeg_encode_params* p) {
    JePlan pl;
    return je_plan(fn, 1, w, h, flags, p, &pl);
}
// mvs_jpeg_encode_dev under the name fn with an output that sizes itself: dout receives offsets[n] bytes
int jpeg_encode_dev_own(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                        int64_t* offsets, Scratch* dout, hipStream_t s) {
    JePlan pl;
    int rc = je_plan(fn, n, w, h, flags, p, &pl);
    if (rc) return rc;
    if (!imgs_dev || !offsets || !dout) return bad(fn, "imgs_dev, offsets or the output block is NULL");
    if ((rc = need_device())) return rc;
    return je_run(fn, pl, imgs_dev, offsets, nullptr, 0, dout, s, nullptr);
}
// mvs_depth_preview's host form
int depth_preview_host(const char* fn, int32_t n, int32_t w, int32_t h, const float* depths, uint8_t* out) {
    int rc = dp_check(fn, n, w, h, depths, out);
    if (rc || (rc = need_device())) return rc;
    const size_t all = (size_t)n * (size_t)w * (size_t)h;
    Scratch din, dout;
    if ((rc = up(din, depths, all)) || (rc = dout.alloc(all)) || (rc = dp_run(n, (int64_t)w * h, din.as<float>(), dout.as<uint8_t>(), nullptr))) return rc;
    return down(out, dout, all);
}

extern "C" {

void mvs_jpeg_encode_default_params(mvs_jpeg_encode_params* p) {
    if (p) *p = mvs_jpeg_encode_params{95, 420, 0, 0};
}

int64_t mvs_jpeg_encode_bound(int32_t w, int32_t h, uint32_t flags, const mvs_jpeg_encode_params* p) {
    JePlan pl;
    const int rc = je_plan(__func__, 1, w, h, flags, p, &pl);
    return rc ? rc : jpeg_enc_bound(pl.S);
}

int mvs_jpeg_encode(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p, int64_t* offsets,
                    uint8_t* data, int64_t capacity) {
    MVS_TRACE();
    const bool ptrs = !imgs || !offsets || (!data && capacity > 0) || capacity < 0;
    Scratch dout;
    int rc = je_host(__func__, n, w, h, imgs, flags, p, ptrs ? "imgs, offsets or data is NULL, or capacity is negative" : nullptr, offsets, &dout);
    if (rc || (rc = je_fits(__func__, offsets[n], capacity))) return rc;
    return down(data, dout, (size_t)offsets[n]);
}

int mvs_jpeg_encode_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                        int64_t* offsets, uint8_t* data_dev, int64_t capacity, void* hip_stream) {
    MVS_TRACE();
    return je_dev(__func__, n, w, h, imgs_dev, flags, p, offsets, data_dev, capacity, hip_stream, nullptr);
}

int mvs_test_jpeg_encode_timed(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                               int64_t* offsets, uint8_t* data_dev, int64_t capacity, void* hip_stream, double* ms) {
    if (!ms) return bad(__func__, "ms is NULL");
    return je_dev(__func__, n, w, h, imgs_dev, flags, p, offsets, data_dev, capacity, hip_stream, ms);
}

int mvs_test_jpeg_encode_coef(int32_t n, int32_t w, int32_t h, const int16_t* coef, uint32_t flags, const mvs_jpeg_encode_params* p,
                              int64_t* offsets, uint8_t* data, int64_t capacity) {
    JePlan pl;
    int rc = je_plan(__func__, n, w, h, flags, p, &pl);
    if (rc) return rc;
    if (!coef || !offsets || (!data && capacity > 0) || capacity < 0) return bad(__func__, "coef, offsets or data is NULL, or capacity is negative");
    int64_t at = 0;
    if (const int16_t* v = je_coef_range(pl.cl, coef, &at)) {
        mvs_set_error("%s: coef[%lld] = %d (image %lld, value %lld of the image, position %d of its block) is outside %s", __func__, (long long)at,
                      (int)*v, (long long)(at / pl.cl.n_coef), (long long)(at % pl.cl.n_coef), (int)(at % 64),
                      at % 64 ? "-1023 .. 1023 of an AC coefficient" : "-1024 .. 1023 of a DC coefficient");
        return MVS_E_INVALID_ARG;
    }
    if ((rc = need_device())) return rc;
    JeCoef c;
    Scratch dout;
    StageClock clk(false);
    if ((rc = je_coef_alloc(pl, &c, nullptr))) return rc;
    HIPCHK(hipMemcpy(c.coef.p, coef, sizeof(int16_t) * (size_t)pl.cl.n_coef * (size_t)n, hipMemcpyHostToDevice));
    if ((rc = je_entropy(__func__, pl, c, clk, offsets, nullptr, 0, &dout, nullptr, nullptr)) || (rc = je_fits(__func__, offsets[n], capacity))) return rc;
    return down(data, dout, (size_t)offsets[n]);
}

int mvs_jpeg_roundtrip(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p, uint8_t* out) {
    MVS_TRACE();
    JePlan pl;
    int rc = je_plan(__func__, n, w, h, flags, p, &pl);
    if (rc || (rc = je_check_ptrs(__func__, imgs, out)) || (rc = need_device())) return rc;
    const size_t nb = (size_t)n * (size_t)w * (size_t)h * 3;
    Scratch dimg, dout;
    if ((rc = up(dimg, imgs, (size_t)pl.cl.img_bytes * (size_t)n)) || (rc = dout.alloc(nb)) ||
        (rc = je_roundtrip(__func__, pl, dimg.as<uint8_t>(), dout.as<uint8_t>(), nullptr))) return rc;
    return down(out, dout, nb);
}

int mvs_jpeg_roundtrip_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                           uint8_t* out_dev, void* hip_stream) {
    MVS_TRACE();
    JePlan pl;
    int rc = je_plan(__func__, n, w, h, flags, p, &pl);
    if (rc || (rc = je_check_ptrs(__func__, imgs_dev, out_dev)) || (rc = need_device())) return rc;
    return je_roundtrip(__func__, pl, imgs_dev, out_dev, (hipStream_t)hip_stream);
}

int mvs_depth_preview(int32_t n, int32_t w, int32_t h, const float* depths, uint8_t* out) {
    MVS_TRACE();
    return depth_preview_host(__func__, n, w, h, depths, out);
}

int mvs_depth_preview_dev(int32_t n, int32_t w, int32_t h, const float* depths_dev, uint8_t* out_dev, void* hip_stream) {
    MVS_TRACE();
    int rc = dp_check(__func__, n, w, h, depths_dev, out_dev);
    if (rc || (rc = need_device())) return rc;
    return dp_run(n, (int64_t)w * h, depths_dev, out_dev, (hipStream_t)hip_stream);
}

}  // extern "C"
