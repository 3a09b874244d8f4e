// overlay.hip — mvs_draw_overlays(_dev), mvs_match_overlays(_dev), mvs_sift_overlays(_dev), mvs_cv_rng_colours (include/mvs.h) and the
// stream producers behind mvs_processor_match_overlays / mvs_processor_sift_overlays (include/mvs_io.h): the match and SIFT overlay
// pictures of R/Processor/Processor.cpp:767-793, :604-615 and R/FeatureProc/FeatureProc.cpp:67-73, rules O1-O6 (overlay_rules.h).
//
//   k_ovl_draw  ONE launch for all canvases of a call: a workgroup of 256 threads per 16 x 16 tile per canvas, a thread per pixel.  The
//               workgroup reads its canvas's list in chunks of 256 from the highest index down; each thread tests one primitive against
//               the tile (ovl_tile_may: conservative, and tight along a diagonal); the survivors are compacted in order into LDS by
//               ballot and prefix, with the constants of O3 formed once (ovl_record); each pixel walks them from the top and stops at
//               its first hit (O4 as a gather).  The workgroup stops when every pixel is painted or the list ends.  A pixel nothing
//               covers is read from the source, every pixel is written once.  A workgroup touches only its own tile, so out == in is
//               allowed.  No atomics, nothing depends on scheduling: two runs give the same bytes.
//   the source  of a tile is a functor: OvlPlain reads canvas i of a stack; OvlStacked reads row y < h of canvas i * n2 + j from
//               imgs1[i] and row y >= h from imgs2[j] at y - h, so the match form never materialises cv::vconcat.
//
// The lists are built on the host (the generator of O6 is sequential) and uploaded through the stream-ordered scratch type.
#include "engine.h"
#include "trace.h"
#include "overlay_rules.h"
#include "stitch.h"
#include "../../include/mvs_test.h"
#include <cstdlib>

static_assert(sizeof(mvs_draw_prim) == sizeof(OvlPrim) && offsetof(mvs_draw_prim, kind) == offsetof(OvlPrim, kind) &&
              offsetof(mvs_draw_prim, c) == offsetof(OvlPrim, c), "OvlPrim is mvs_draw_prim");
static_assert(MVS_DRAW_DISC == OVL_DISC && MVS_DRAW_RING == OVL_RING && MVS_DRAW_SEGMENT == OVL_SEGMENT, "the kinds of mvs.h");

namespace {

struct OvlPlain {                      // canvas i: imgs + i * h * w * 3
    const uint8_t* imgs;
    int32_t w, h;
    __device__ const uint8_t* operator()(int64_t canvas, int32_t x, int32_t y) const { return imgs + ((canvas * h + y) * w + x) * 3; }
};
struct OvlStacked {                    // canvas first + c = i * n2 + j: imgs1[i] over imgs2[j], each h x w
    const uint8_t *imgs1, *imgs2;
    int32_t w, h, n2, first;
    __device__ const uint8_t* operator()(int64_t canvas, int32_t x, int32_t y) const {
        const int64_t k = canvas + first, i = k / n2, j = k % n2;
        return y < h ? imgs1 + ((i * h + y) * w + x) * 3 : imgs2 + ((j * h + (y - h)) * w + x) * 3;
    }
};

// one primitive as three 8-byte loads (a block of the scratch pool is aligned far beyond 8, and 24 k keeps that): read member by
// member the five uint8 fields would be loads of their own
__device__ inline OvlPrim ovl_load(const OvlPrim* p) {
    union { OvlPrim q; uint2 v[3]; } b;
    const uint2* s = reinterpret_cast<const uint2*>(p);
    b.v[0] = s[0]; b.v[1] = s[1]; b.v[2] = s[2];
    return b.q;
}

// w, h: the canvas (of OvlStacked: both images).  out may be the source
template <class Src>
__global__ __launch_bounds__(OVL_CHUNK) void k_ovl_draw(Src src, int32_t w, int32_t h, const int64_t* __restrict__ off,
                                                        const OvlPrim* __restrict__ prims, uint8_t* out) {
    __shared__ OvlRec s_rec[OVL_CHUNK];
    __shared__ int32_t s_wave[OVL_CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t tx0 = (int32_t)blockIdx.x * OVL_TILE, ty0 = (int32_t)blockIdx.y * OVL_TILE;
    const int32_t x = tx0 + (tid & (OVL_TILE - 1)), y = ty0 + tid / OVL_TILE;
    const int64_t canvas = blockIdx.z;
    const bool inside = x < w && y < h;
    const int64_t lo = off[canvas], hi = off[canvas + 1];
    bool painted = false;
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    for (int64_t end = hi; end > lo; end -= OVL_CHUNK) {               // thread t holds primitive end - 1 - t: the highest index first
        const int64_t k = end - 1 - tid;
        OvlPrim q;
        bool keep = false;
        if (k >= lo) {
            q = ovl_load(prims + k);
            keep = ovl_tile_may(q, tx0, ty0);
        }
        const unsigned long long ballot = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int base = 0, total = 0;
        for (int v = 0; v < OVL_CHUNK / 64; ++v) {
            base += v < wave ? s_wave[v] : 0;
            total += s_wave[v];
        }
        if (keep) s_rec[base + __popcll(ballot & ((1ull << lane) - 1ull))] = ovl_record(q);
        __syncthreads();
        if (inside && !painted)
            for (int m = 0; m < total; ++m)
                if (ovl_hit(s_rec[m], x, y)) {
                    painted = true;
                    c0 = s_rec[m].c[0]; c1 = s_rec[m].c[1]; c2 = s_rec[m].c[2];
                    break;
                }
        if (__syncthreads_and(painted || !inside)) break;               // also the barrier in front of the next chunk's LDS writes
    }
    if (!inside) return;
    if (!painted) {
        const uint8_t* p = src(canvas, x, y);
        c0 = p[0]; c1 = p[1]; c2 = p[2];
    }
    uint8_t* o = out + ((canvas * h + y) * w + x) * 3;
    o[0] = c0; o[1] = c1; o[2] = c2;
}

// ------------------------------------------------------------------ host ----
// O1 and the launch: n canvases of w x h
int ovl_check_size(const char* fn, int64_t n, int32_t w, int32_t h) {
    if (n < 1 || n > 65535) return bad(fn, "need 1 .. 65535 canvases");
    if (w < 1 || h < 1 || w > OVL_MAX_DIM || h > OVL_MAX_DIM) return bad(fn, "a canvas must be 1 .. 16384 wide and high");
    if (n * ((w + OVL_TILE - 1) / OVL_TILE) * ((h + OVL_TILE - 1) / OVL_TILE) > 0x7fffffffLL) return bad(fn, "too many tiles for one call");
    return MVS_OK;
}

// O2, O5 on the lists of n canvases
int ovl_check_lists(const char* fn, int32_t n, int32_t w, int32_t h, const int64_t* off, const mvs_draw_prim* prims) {
    if (!off) return bad(fn, "prim_offsets is NULL");
    if (int rc = check_offsets(fn, "prim_offsets", off, n)) return rc;
    if (off[n] > 0 && !prims) return bad(fn, "prims is NULL");
    for (int32_t i = 0; i < n; ++i)
        for (int64_t k = off[i]; k < off[i + 1]; ++k)
            if (const char* why = ovl_prim_error(reinterpret_cast<const OvlPrim&>(prims[k]), w, h)) {
                mvs_set_error("%s: canvas %d, primitive %lld (%lld of its list): %s", fn, i, (long long)k, (long long)(k - off[i]), why);
                return MVS_E_INVALID_ARG;
            }
    return MVS_OK;
}

// the launch on lists the caller has checked: off (n + 1, from 0) and prims are host arrays; complete on return.  ms (may be NULL)
// receives the milliseconds of the launch alone
template <class Src>
int ovl_draw(Src src, int32_t n, int32_t w, int32_t h, const int64_t* off, const OvlPrim* prims, uint8_t* out_dev, hipStream_t s, double* ms = nullptr) {
    Scratch doff, dprims;
    StageClock clk(ms != nullptr);
    int rc;
    if ((rc = up_async(doff, off, (size_t)n + 1, s)) || (rc = up_async(dprims, prims, (size_t)off[n], s)) || (rc = clk.mark(s))) return rc;
    const dim3 grid((unsigned)((w + OVL_TILE - 1) / OVL_TILE), (unsigned)((h + OVL_TILE - 1) / OVL_TILE), (unsigned)n);
    k_ovl_draw<Src><<<grid, dim3(OVL_CHUNK), 0, s>>>(src, w, h, doff.as<int64_t>(), dprims.as<OvlPrim>(), out_dev);
    HIPCHK(hipGetLastError());
    if ((rc = clk.mark(s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return ms ? clk.read(ms) : MVS_OK;
}

// ---- the match form
int ovl_match_check(const char* fn, int32_t n1, int32_t n2, int32_t w, int32_t h, const void* imgs1, const void* imgs2, const int64_t* moff,
                    const int32_t* matches) {
    if (n1 < 1 || n2 < 1) return bad(fn, "need n1, n2 >= 1");
    if (h < 1 || 2 * (int64_t)h > OVL_MAX_DIM) return bad(fn, "the stacked canvas is 2 h rows: need 1 <= 2 h <= 16384");
    if (int rc = ovl_check_size(fn, (int64_t)n1 * n2, w, 2 * h)) return rc;
    if (!imgs1 || !imgs2 || !moff) return bad(fn, "imgs1, imgs2 or match_offsets is NULL");
    const int32_t n = n1 * n2;
    if (int rc = check_offsets(fn, "match_offsets", moff, n, 0x7fffffffLL / 3)) return rc;
    if (moff[n] > 0 && !matches) return bad(fn, "matches is NULL");
    for (int32_t c = 0; c < n; ++c)
        for (int64_t k = moff[c]; k < moff[c + 1]; ++k) {
            const int32_t* m = matches + 4 * k;
            if (m[0] < 0 || m[0] >= w || m[2] < 0 || m[2] >= w || m[1] < 0 || m[1] >= h || m[3] < 0 || m[3] >= h) {
                mvs_set_error("%s: pair (%d, %d), match %lld of its list: (%d, %d) - (%d, %d) has an end outside the %d x %d images", fn, c / n2,
                              c % n2, (long long)(k - moff[c]), m[0], m[1], m[2], m[3], w, h);
                return MVS_E_INVALID_ARG;
            }
        }
    return MVS_OK;
}
// canvases [c0, c1): ring, ring, segment per match; the generator runs on through them in order
void ovl_match_build(int32_t c0, int32_t c1, int32_t h, const int64_t* moff, const int32_t* matches, bool swap, uint64_t* state,
                     std::vector<int64_t>* off, std::vector<OvlPrim>* prims) {
    off->assign(1, 0);
    prims->resize((size_t)(3 * (moff[c1] - moff[c0])));
    size_t at = 0;
    for (int32_t c = c0; c < c1; ++c) {
        for (int64_t k = moff[c]; k < moff[c + 1]; ++k, at += 3) {
            uint8_t line[3];
            ovl_rng_colour(state, line);
            ovl_match_prims(matches + 4 * k, h, line, swap, prims->data() + at);
        }
        off->push_back((int64_t)at);
    }
}

// ---- the SIFT form
int ovl_sift_check(const char* fn, int32_t n, int32_t w, int32_t h, const void* views, const int64_t* koff, const float* keys) {
    if (int rc = ovl_check_size(fn, n, w, h)) return rc;
    if (!views || !koff) return bad(fn, "views or key_offsets is NULL");
    if (int rc = check_offsets(fn, "key_offsets", koff, n, 0x7fffffffLL)) return rc;
    if (koff[n] > 0 && !keys) return bad(fn, "keys is NULL");
    return MVS_OK;
}
// lists [c0, c1): a filled r = 1 disc in (0, 255, 0) at cvRound of every key; a key whose plus cannot reach the canvas (NaN included:
// INT_MIN) is clipped away here
void ovl_sift_build(int32_t c0, int32_t c1, int32_t w, int32_t h, const int64_t* koff, const float* keys, std::vector<int64_t>* off,
                    std::vector<OvlPrim>* prims) {
    off->assign(1, 0);
    prims->clear();
    for (int32_t c = c0; c < c1; ++c) {
        for (int64_t k = koff[c]; k < koff[c + 1]; ++k) {
            const int32_t x = ovl_round_i32(keys[4 * k]), y = ovl_round_i32(keys[4 * k + 1]);
            if (x < -1 || x > w || y < -1 || y > h) continue;
            prims->push_back(ovl_prim(OVL_DISC, x, y, 0, 0, 1, 0, 255, 0));
        }
        off->push_back((int64_t)prims->size());
    }
}

int ovl_match_run(const char* fn, int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1_dev, const uint8_t* imgs2_dev, const int64_t* moff,
                  const int32_t* matches, uint64_t* rng_state, uint8_t* out_dev, hipStream_t s, double* ms) {
    int rc = ovl_match_check(fn, n1, n2, w, h, imgs1_dev, imgs2_dev, moff, matches);
    if (rc) return rc;
    if (!out_dev) return bad(fn, "out is NULL");
    if ((rc = need_device())) return rc;
    uint64_t fresh = OVL_RNG_DEFAULT;
    std::vector<int64_t> off;
    std::vector<OvlPrim> prims;
    const double t0 = now_ms();
    ovl_match_build(0, n1 * n2, h, moff, matches, false, rng_state ? rng_state : &fresh, &off, &prims);
    if (ms) ms[0] = now_ms() - t0;
    return ovl_draw(OvlStacked{imgs1_dev, imgs2_dev, w, h, n2, 0}, n1 * n2, w, 2 * h, off.data(), prims.data(), out_dev, s, ms ? ms + 1 : nullptr);
}

int ovl_sift_run(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* views_dev, const int64_t* koff, const float* keys, uint8_t* out_dev,
                 hipStream_t s) {
    std::vector<int64_t> off;
    std::vector<OvlPrim> prims;
    ovl_sift_build(0, n, w, h, koff, keys, &off, &prims);
    return ovl_draw(OvlPlain{views_dev, w, h}, n, w, h, off.data(), prims.data(), out_dev, s);
}

// MVS_OVERLAY_BATCH_BYTES (environment, read at every call): the canvas bytes one batch of the stream producers may hold in HBM;
// default 512 MiB, which takes the 256 canvases of 640 x 960 of a 16 x 16 sequence pair (472 MB) in one batch.  The files do not
// depend on it
int64_t ovl_batch_bytes() {
    const char* e = std::getenv("MVS_OVERLAY_BATCH_BYTES");
    const long long v = (e && *e) ? std::atoll(e) : 0;
    return v > 0 ? (int64_t)v : (int64_t)512 << 20;
}
int32_t ovl_batch_canvases(int32_t n, int32_t w, int32_t h) {
    const int64_t per = ovl_batch_bytes() / ((int64_t)w * h * 3);
    return (int32_t)(per < 1 ? 1 : per > n ? n : per);
}

// one batch behind its draw launch: the canvases at canvas_dev encoded by the one encoder call, the streams downloaded, the sink called
int ovl_encode_batch(const char* fn, int32_t first, int32_t count, int32_t w, int32_t h, const uint8_t* canvas_dev, uint32_t flags,
                     const mvs_jpeg_encode_params* params, const OverlaySink& sink) {
    std::vector<int64_t> joff((size_t)count + 1);
    Scratch dstreams;
    int rc = jpeg_encode_dev_own(fn, count, w, h, canvas_dev, flags, params, joff.data(), &dstreams, nullptr);
    if (rc) return rc;
    std::vector<uint8_t> data((size_t)joff[(size_t)count]);
    if ((rc = down(data.data(), dstreams, data.size()))) return rc;
    return sink(first, count, joff.data(), data.data());
}

}  // namespace

int match_overlay_streams(const char* fn, int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1, const uint8_t* imgs2, const int64_t* moff,
                          const int32_t* matches, uint32_t flags, uint64_t* rng_state, const mvs_jpeg_encode_params* params, const OverlaySink& sink) {
    if (flags & ~(uint32_t)MVS_JPEG_RGB) return bad(fn, "unknown flag bits");
    int rc = ovl_match_check(fn, n1, n2, w, h, imgs1, imgs2, moff, matches);
    if (rc || (rc = jpeg_encode_check(fn, w, 2 * h, flags, params)) || (rc = need_device())) return rc;
    const int32_t n = n1 * n2, per = ovl_batch_canvases(n, w, 2 * h);
    const size_t img = (size_t)w * (size_t)h * 3;
    Scratch d1, d2, canvas;
    if ((rc = up(d1, imgs1, img * (size_t)n1)) || (rc = up(d2, imgs2, img * (size_t)n2)) || (rc = canvas.alloc(2 * img * (size_t)per))) return rc;
    uint64_t fresh = OVL_RNG_DEFAULT;
    uint64_t* state = rng_state ? rng_state : &fresh;
    std::vector<int64_t> off;
    std::vector<OvlPrim> prims;
    for (int32_t c0 = 0; c0 < n; c0 += per) {
        const int32_t cnt = n - c0 < per ? n - c0 : per;
        ovl_match_build(c0, c0 + cnt, h, moff, matches, flags & MVS_JPEG_RGB, state, &off, &prims);
        if ((rc = ovl_draw(OvlStacked{d1.as<uint8_t>(), d2.as<uint8_t>(), w, h, n2, c0}, cnt, w, 2 * h, off.data(), prims.data(), canvas.as<uint8_t>(),
                           nullptr)) ||
            (rc = ovl_encode_batch(fn, c0, cnt, w, 2 * h, canvas.as<uint8_t>(), flags, params, sink))) return rc;
    }
    return MVS_OK;
}

int sift_overlay_streams(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* views, const int64_t* koff, const float* keys, uint32_t flags,
                         const mvs_jpeg_encode_params* params, const OverlaySink& sink) {
    if (flags & ~(uint32_t)MVS_JPEG_RGB) return bad(fn, "unknown flag bits");
    int rc = ovl_sift_check(fn, n, w, h, views, koff, keys);
    if (rc || (rc = jpeg_encode_check(fn, w, h, flags, params)) || (rc = need_device())) return rc;
    const int32_t per = ovl_batch_canvases(n, w, h);
    const size_t img = (size_t)w * (size_t)h * 3;
    Scratch canvas;
    if ((rc = canvas.alloc(img * (size_t)per))) return rc;
    std::vector<int64_t> off;
    std::vector<OvlPrim> prims;
    for (int32_t c0 = 0; c0 < n; c0 += per) {                          // the marks are (0, 255, 0) in either channel order
        const int32_t cnt = n - c0 < per ? n - c0 : per;
        HIPCHK(hipMemcpy(canvas.p, views + img * (size_t)c0, img * (size_t)cnt, hipMemcpyHostToDevice));
        ovl_sift_build(c0, c0 + cnt, w, h, koff, keys, &off, &prims);
        if ((rc = ovl_draw(OvlPlain{canvas.as<uint8_t>(), w, h}, cnt, w, h, off.data(), prims.data(), canvas.as<uint8_t>(), nullptr)) ||
            (rc = ovl_encode_batch(fn, c0, cnt, w, h, canvas.as<uint8_t>(), flags, params, sink))) return rc;
    }
    return MVS_OK;
}

extern "C" {

void mvs_cv_rng_colours(uint64_t* state, int64_t n, uint8_t* bgr) {
    if (!state || !bgr) return;
    for (int64_t i = 0; i < n; ++i) ovl_rng_colour(state, bgr + 3 * i);
}

int mvs_draw_overlays(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const int64_t* prim_offsets, const mvs_draw_prim* prims, uint8_t* out) {
    MVS_TRACE();
    int rc = ovl_check_size(__func__, n, w, h);
    if (rc || (rc = ovl_check_lists(__func__, n, w, h, prim_offsets, prims))) return rc;
    if (!imgs || !out) return bad(__func__, "imgs or out is NULL");
    if ((rc = need_device())) return rc;
    const size_t all = (size_t)n * (size_t)w * (size_t)h * 3;
    Scratch d;
    if ((rc = up(d, imgs, all)) || (rc = ovl_draw(OvlPlain{d.as<uint8_t>(), w, h}, n, w, h, prim_offsets, (const OvlPrim*)prims, d.as<uint8_t>(), nullptr)))
        return rc;
    return down(out, d, all);
}

int mvs_draw_overlays_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, const int64_t* prim_offsets, const mvs_draw_prim* prims,
                          uint8_t* out_dev, void* hip_stream) {
    MVS_TRACE();
    int rc = ovl_check_size(__func__, n, w, h);
    if (rc || (rc = ovl_check_lists(__func__, n, w, h, prim_offsets, prims))) return rc;
    if (!imgs_dev || !out_dev) return bad(__func__, "imgs_dev or out_dev is NULL");
    if ((rc = need_device())) return rc;
    return ovl_draw(OvlPlain{imgs_dev, w, h}, n, w, h, prim_offsets, (const OvlPrim*)prims, out_dev, (hipStream_t)hip_stream);
}

int mvs_match_overlays(int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1, const uint8_t* imgs2, const int64_t* match_offsets,
                       const int32_t* matches, uint64_t* rng_state, uint8_t* out) {
    MVS_TRACE();
    int rc = ovl_match_check(__func__, n1, n2, w, h, imgs1, imgs2, match_offsets, matches);
    if (rc) return rc;
    if (!out) return bad(__func__, "out is NULL");
    if ((rc = need_device())) return rc;
    const size_t img = (size_t)w * (size_t)h * 3, all = 2 * img * (size_t)n1 * (size_t)n2;
    Scratch d1, d2, dout;
    if ((rc = up(d1, imgs1, img * (size_t)n1)) || (rc = up(d2, imgs2, img * (size_t)n2)) || (rc = dout.alloc(all)) ||
        (rc = ovl_match_run(__func__, n1, n2, w, h, d1.as<uint8_t>(), d2.as<uint8_t>(), match_offsets, matches, rng_state, dout.as<uint8_t>(), nullptr,
                            nullptr))) return rc;
    return down(out, dout, all);
}

int mvs_match_overlays_dev(int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1_dev, const uint8_t* imgs2_dev, const int64_t* match_offsets,
                           const int32_t* matches, uint64_t* rng_state, uint8_t* out_dev, void* hip_stream) {
    MVS_TRACE();
    return ovl_match_run(__func__, n1, n2, w, h, imgs1_dev, imgs2_dev, match_offsets, matches, rng_state, out_dev, (hipStream_t)hip_stream, nullptr);
}

int mvs_test_match_overlays_timed(int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1_dev, const uint8_t* imgs2_dev,
                                  const int64_t* match_offsets, const int32_t* matches, uint64_t* rng_state, uint8_t* out_dev, void* hip_stream,
                                  double* ms) {
    if (!ms) return bad(__func__, "ms is NULL");
    return ovl_match_run(__func__, n1, n2, w, h, imgs1_dev, imgs2_dev, match_offsets, matches, rng_state, out_dev, (hipStream_t)hip_stream, ms);
}

int mvs_sift_overlays(int32_t n_lists, int32_t w, int32_t h, const uint8_t* views, const int64_t* key_offsets, const float* keys, uint8_t* out) {
    MVS_TRACE();
    int rc = ovl_sift_check(__func__, n_lists, w, h, views, key_offsets, keys);
    if (rc) return rc;
    if (!out) return bad(__func__, "out is NULL");
    if ((rc = need_device())) return rc;
    const size_t all = (size_t)n_lists * (size_t)w * (size_t)h * 3;
    Scratch d;
    if ((rc = up(d, views, all)) || (rc = ovl_sift_run(__func__, n_lists, w, h, d.as<uint8_t>(), key_offsets, keys, d.as<uint8_t>(), nullptr))) return rc;
    return down(out, d, all);
}

int mvs_sift_overlays_dev(int32_t n_lists, int32_t w, int32_t h, const uint8_t* views_dev, const int64_t* key_offsets, const float* keys,
                          uint8_t* out_dev, void* hip_stream) {
    MVS_TRACE();
    int rc = ovl_sift_check(__func__, n_lists, w, h, views_dev, key_offsets, keys);
    if (rc) return rc;
    if (!out_dev) return bad(__func__, "out_dev is NULL");
    if ((rc = need_device())) return rc;
    return ovl_sift_run(__func__, n_lists, w, h, views_dev, key_offsets, keys, out_dev, (hipStream_t)hip_stream);
}

}  // extern "C"
