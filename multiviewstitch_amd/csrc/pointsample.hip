// pointsample.hip — mvs_point_sample (include/mvs.h): the checked inverse-depth rasters of every sequence to oriented points, the
// step GeometryRec::RunPointSample takes between Processor::CheckConsistency and the stitch tail (R/Processor/Processor.cpp:933-949).
// GeoRec is a closed binary: the rules are this library's definition, stated in include/mvs.h; their per-pixel part is
// pointsample_rules.h, one body for these kernels and for host code.
//
//   k_ps_candidates  ONE launch for all frames of all sequences, a thread per cell: rules 1-6 do not depend on coverage.  The
//                    thread walks its cell in row-major order and stops at the first pixel that passes; it writes the cell's int32
//                    (pixel index or -1).  Reads: the pixel's raster neighbourhood and one 4-byte gather per neighbour frame, the
//                    access pattern of k_check_seq.  Frame and sequence come from blockIdx alone, so the cameras stay in scalar
//                    registers.
//   k_ps_emit        one launch per frame step t, over the cells of frame t of every sequence that has one: a cell with a
//                    candidate and a clear coverage byte emits; its thread then marks, with plain byte stores of 1, the cell its
//                    point lands on in every later frame that agrees with it.  A launch writes only bytes of frames above t and
//                    the byte of its own cell, which from then on holds the emit flag: stream order is the only synchronisation.
//   k_ps_count / CompactTail / k_ps_scatter
//                    the ordered compaction of views.hip's key-point cull (compact.hip).  Output order is pixel order, not cell order: a frame is
//                    walked as h x cw slots (pixel row v, cell column cx); the slot is set when cell (v / r, cx) emits and its
//                    candidate lies in row v.  Survivor counts per workgroup, one exclusive scan, then the scatter recomputes point
//                    and normal and writes the rows.  No atomic anywhere: two runs are bit-identical.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "frontend_dev.h"
#include "pointsample_rules.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int PS_TPB = 256, PS_WAVES = PS_TPB / 64;
static_assert(PS_TPB == COMPACT_TPB, "k_ps_count and k_ps_scatter count and place per workgroup of the shared tail");

struct PsSeq {                        // one sequence: its cameras cams[cam0 .. cam0 + n), all w x h, cut into cw x ch cells
    int32_t cam0, n, w, h, cw, ch;
    int64_t ras_off;                  // floats in front of its first raster
    int64_t cell_off;                 // cells in front of its first frame
};

__global__ __launch_bounds__(PS_TPB) void k_ps_candidates(const float* __restrict__ depths, const CamDev* __restrict__ cams,
                                                          const PsSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int maxblk,
                                                          PsRules q, int32_t* __restrict__ cand) {
    const int cam = blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const PsSeq s = seqs[seq_of[cam]];
    const int ncell = s.cw * s.ch, cell = b * PS_TPB + threadIdx.x, f = cam - s.cam0;
    if (cell >= ncell) return;
    cand[s.cell_off + (int64_t)f * ncell + cell] = ps_cell_candidate(cams + s.cam0, depths + s.ras_off, s.n, f, cell % s.cw, cell / s.cw, q);
}

__global__ __launch_bounds__(PS_TPB) void k_ps_emit(const float* __restrict__ depths, const CamDev* __restrict__ cams,
                                                    const PsSeq* __restrict__ seqs, int maxblk, int t, PsRules q,
                                                    const int32_t* __restrict__ cand, uint8_t* __restrict__ cover) {
    const int k = blockIdx.x / maxblk, b = blockIdx.x % maxblk;
    const PsSeq s = seqs[k];
    const int ncell = s.cw * s.ch, cell = b * PS_TPB + threadIdx.x;
    if (t >= s.n || cell >= ncell) return;
    const int64_t at = s.cell_off + (int64_t)t * ncell + cell;
    const int32_t c = cand[at];
    const bool emit = c >= 0 && !cover[at];
    cover[at] = emit ? 1 : 0;                                            // nothing covers frame t any more: the byte is the emit flag now
    if (!emit) return;
    const int64_t npx = (int64_t)s.w * s.h;
    const float* ras = depths + s.ras_off;
    const d3 P = world_from_img_hd(cams[s.cam0 + t], c % s.w, c / s.w, 1.0 / (double)ras[t * npx + c]);
    for (int g = t + 1; g < s.n; ++g) {                                  // rule 7
        int32_t u, v;
        bool in_img;
        if (ps_agrees(P, cams[s.cam0 + g], ras + g * npx, q, &u, &v, &in_img))
            cover[s.cell_off + (int64_t)g * ncell + (int64_t)(v / q.r) * s.cw + u / q.r] = 1;
    }
}

// slot (v, cx) of a frame, in output order: is it the emitted candidate of cell (v / r, cx)?  -> the candidate's pixel index or -1
__device__ inline int32_t ps_slot(const PsSeq& s, int f, int64_t slot, int r, const int32_t* __restrict__ cand, const uint8_t* __restrict__ flag) {
    const int v = (int)(slot / s.cw), cx = (int)(slot % s.cw);
    const int64_t at = s.cell_off + (int64_t)f * s.cw * s.ch + (int64_t)(v / r) * s.cw + cx;
    if (!flag[at]) return -1;
    const int32_t c = cand[at];
    return c / s.w == v ? c : -1;
}

__global__ __launch_bounds__(PS_TPB) void k_ps_count(const PsSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int maxblk, int r,
                                                     const int32_t* __restrict__ cand, const uint8_t* __restrict__ flag, int32_t* __restrict__ cnt) {
    __shared__ int s_wsum[PS_WAVES];
    const int cam = blockIdx.x / maxblk;
    const int64_t slot = (int64_t)(blockIdx.x % maxblk) * PS_TPB + threadIdx.x;     // h * cw may come within a workgroup of 2^31
    const PsSeq s = seqs[seq_of[cam]];
    const bool f = slot < (int64_t)s.h * s.cw && ps_slot(s, cam - s.cam0, slot, r, cand, flag) >= 0;
    const WgRank k = wg_rank<PS_WAVES>(f, s_wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = k.total;
}

__global__ __launch_bounds__(PS_TPB) void k_ps_scatter(const float* __restrict__ depths, const CamDev* __restrict__ cams,
                                                       const PsSeq* __restrict__ seqs, const int32_t* __restrict__ seq_of, int maxblk, PsRules q,
                                                       const int32_t* __restrict__ cand, const uint8_t* __restrict__ flag,
                                                       const int32_t* __restrict__ base, double* __restrict__ points, double* __restrict__ normals,
                                                       int32_t* __restrict__ frame, int32_t* __restrict__ pixel) {
    __shared__ int s_wsum[PS_WAVES];
    const int cam = blockIdx.x / maxblk;
    const int64_t slot = (int64_t)(blockIdx.x % maxblk) * PS_TPB + threadIdx.x;     // h * cw may come within a workgroup of 2^31
    const PsSeq s = seqs[seq_of[cam]];
    const int f = cam - s.cam0;
    const int32_t c = slot < (int64_t)s.h * s.cw ? ps_slot(s, f, slot, q.r, cand, flag) : -1;
    const int64_t pos = (int64_t)base[blockIdx.x] + wg_rank<PS_WAVES>(c >= 0, s_wsum).rank;
    if (c < 0) return;
    d3 P = mk3(0, 0, 0), N = mk3(0, 0, 0);
    ps_point_normal(cams[cam], depths + s.ras_off + (int64_t)f * s.w * s.h, c % s.w, c / s.w, q, &P, &N);   // a candidate: rules 1-3 hold
    st3(points + 3 * pos, P);
    st3(normals + 3 * pos, N);
    if (frame) frame[pos] = f;
    if (pixel) pixel[pos] = c;
}

// what a call is made of, built by the argument checks on the host
struct PsPlan {
    std::vector<PsSeq> seqs;
    std::vector<int32_t> seq_of;
    PsRules q;
    int ncam = 0, max_frames = 0, blk_cells = 0, blk_slots = 0;
    int64_t cells = 0, floats = 0;
};

int check_ps(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const void* depths, const mvs_point_sample_params* p,
             const void* seq_offsets, const void* points, const void* normals, int64_t capacity, PsPlan* pl) {
    if (!cam_off || !cams || !depths || !p || !seq_offsets || !points || !normals)
        return bad(fn, "cam_off, cams, depths, params, seq_offsets, points or normals is NULL");
    if (n_seq < 1) return bad(fn, "need n_seq >= 1");
    int rc = check_offsets(fn, "cam_off", cam_off, n_seq);
    if (rc) return rc;
    if (!std::isfinite(p->dsp_min) || !std::isfinite(p->dsp_max) || !std::isfinite(p->max_dsp_err) || !std::isfinite(p->min_conf) ||
        !std::isfinite(p->edge_sz_thres)) return bad(fn, "a parameter is not finite");
    if (p->dsp_min <= 0.0 || p->dsp_min > p->dsp_max) return bad(fn, "need 0 < dsp_min <= dsp_max");
    if (p->max_dsp_err < 0.0) return bad(fn, "max_dsp_err is negative");
    if (p->min_conf < 0.0 || p->min_conf > 1.0) return bad(fn, "min_conf must lie in [0, 1]");
    if (p->edge_sz_thres <= 0.0) return bad(fn, "need edge_sz_thres > 0");
    if (p->pt_samp_rds < 1) return bad(fn, "need pt_samp_rds >= 1");
    if (p->nbr_frm_num < 0) return bad(fn, "nbr_frm_num is negative");
    if (p->nbr_frm_step < 1) return bad(fn, "need nbr_frm_step >= 1");
    if (capacity < 0) return bad(fn, "capacity is negative");
    pl->q = PsRules{p->dsp_min, p->dsp_max, p->max_dsp_err, p->min_conf, p->edge_sz_thres, p->pt_samp_rds, p->nbr_frm_num, p->nbr_frm_step};
    pl->ncam = cam_off[n_seq];
    pl->seqs.resize((size_t)n_seq);
    pl->seq_of.resize((size_t)pl->ncam);
    for (int k = 0; k < n_seq; ++k) {
        PsSeq& s = pl->seqs[(size_t)k];
        s = PsSeq{cam_off[k], cam_off[k + 1] - cam_off[k], 0, 0, 0, 0, pl->floats, pl->cells};
        if (!s.n) continue;
        const mvs_camera* c = cams + s.cam0;
        for (int f = 0; f < s.n; ++f) {
            if (!cam_fine(c + f)) return bad(fn, "a camera needs w, h > 0 and fx, fy != 0");
            if (c[f].w != c[0].w || c[f].h != c[0].h) return bad(fn, "the frames of a sequence must share one raster size");
            pl->seq_of[(size_t)(s.cam0 + f)] = k;
        }
        if ((int64_t)c[0].w * c[0].h > 0x7fffffffLL) return bad(fn, "w * h of a frame must fit an int32 pixel index");
        s.w = c[0].w; s.h = c[0].h;
        s.cw = ps_cells(s.w, pl->q.r); s.ch = ps_cells(s.h, pl->q.r);
        const int64_t ncell = (int64_t)s.cw * s.ch, nslot = (int64_t)s.h * s.cw;
        pl->floats += (int64_t)s.n * s.w * s.h;
        pl->cells += (int64_t)s.n * ncell;
        if (pl->cells > 0x7fffffffLL) return bad(fn, "too many cells for one call (2^31 and above)");
        if (s.n > pl->max_frames) pl->max_frames = s.n;
        if ((ncell + PS_TPB - 1) / PS_TPB > pl->blk_cells) pl->blk_cells = (int)((ncell + PS_TPB - 1) / PS_TPB);
        if ((nslot + PS_TPB - 1) / PS_TPB > pl->blk_slots) pl->blk_slots = (int)((nslot + PS_TPB - 1) / PS_TPB);
    }
    const int64_t most = pl->ncam > n_seq ? pl->ncam : n_seq;
    if (most * pl->blk_cells > 0x7fffffffLL || most * pl->blk_slots > 0x7fffffffLL) return bad(fn, "cameras * w * h is too large for one launch");
    return MVS_OK;
}

// Candidates, coverage and the scan of a call: everything up to seq_offsets.  The tables stay in the object for scatter().
struct PsRun {
    const PsPlan& pl;
    const float* depths;
    hipStream_t s;
    int n_seq, nb = 0;
    std::vector<CamDev> hc;
    Scratch dcam, dseq, dsof, dcoff, dcand, dcover;
    CompactTail ct;
    PsRun(const PsPlan& plan, int n, const float* depths_dev, hipStream_t st) : pl(plan), depths(depths_dev), s(st), n_seq(n) {}

    int candidates(const mvs_camera* cams, const int32_t* cam_off) {
        int rc;
        if ((rc = up_cams(dcam, hc, cams, (size_t)pl.ncam, s)) || (rc = up_async(dseq, pl.seqs.data(), pl.seqs.size(), s)) ||
            (rc = up_async(dsof, pl.seq_of.data(), pl.seq_of.size(), s)) || (rc = up_async(dcoff, cam_off, (size_t)n_seq + 1, s)) ||
            (rc = dcand.alloc(sizeof(int32_t) * (size_t)pl.cells, s)) || (rc = dcover.alloc((size_t)pl.cells, s))) return rc;
        k_ps_candidates<<<dim3((unsigned)(pl.ncam * pl.blk_cells)), dim3(PS_TPB), 0, s>>>(depths, dcam.as<CamDev>(), dseq.as<PsSeq>(), dsof.as<int32_t>(),
                                                                                         pl.blk_cells, pl.q, dcand.as<int32_t>());
        HIPCHK(hipGetLastError());
        return MVS_OK;
    }

    int emit_and_scan(int64_t* seq_offsets) {
        int rc;
        nb = pl.ncam * pl.blk_slots;
        if ((rc = ct.alloc((size_t)nb, (size_t)n_seq, s))) return rc;
        HIPCHK(hipMemsetAsync(dcover.p, 0, (size_t)pl.cells, s));
        for (int t = 0; t < pl.max_frames; ++t)
            k_ps_emit<<<dim3((unsigned)(n_seq * pl.blk_cells)), dim3(PS_TPB), 0, s>>>(depths, dcam.as<CamDev>(), dseq.as<PsSeq>(), pl.blk_cells, t, pl.q,
                                                                                     dcand.as<int32_t>(), dcover.as<uint8_t>());
        k_ps_count<<<dim3((unsigned)nb), dim3(PS_TPB), 0, s>>>(dseq.as<PsSeq>(), dsof.as<int32_t>(), pl.blk_slots, pl.q.r, dcand.as<int32_t>(),
                                                              dcover.as<uint8_t>(), ct.cnt.as<int32_t>());
        ct.strided(nb, dcoff.as<int32_t>(), n_seq, pl.blk_slots, s);       // seq_offsets: a sequence starts where the workgroups of its first camera start
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(seq_offsets, ct.off.p, sizeof(int64_t) * ((size_t)n_seq + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MVS_OK;
    }

    int scatter(double* points, double* normals, int32_t* frame, int32_t* pixel) {
        k_ps_scatter<<<dim3((unsigned)nb), dim3(PS_TPB), 0, s>>>(depths, dcam.as<CamDev>(), dseq.as<PsSeq>(), dsof.as<int32_t>(), pl.blk_slots, pl.q,
                                                                dcand.as<int32_t>(), dcover.as<uint8_t>(), ct.base.as<int32_t>(), points, normals, frame, pixel);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        return MVS_OK;
    }
};

int too_small(const char* fn) { return bad(fn, "capacity is below the number of points (seq_offsets holds it)"); }

}  // namespace

// the host form for a caller inside the library that cannot know the count in advance (mvs_processor_point_sample): the vectors are
// sized once seq_offsets is known
int point_sample_vectors(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths,
                         const mvs_point_sample_params* p, int64_t* seq_offsets, std::vector<double>* points, std::vector<double>* normals) {
    PsPlan pl;
    int rc = check_ps(fn, n_seq, cam_off, cams, depths, p, seq_offsets, points, normals, 0, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    points->clear();
    normals->clear();
    if (pl.cells == 0) { std::memset(seq_offsets, 0, sizeof(int64_t) * ((size_t)n_seq + 1)); return MVS_OK; }
    Scratch dd, dp, dn;
    if ((rc = up(dd, depths, (size_t)pl.floats))) return rc;
    PsRun run(pl, n_seq, dd.as<float>(), nullptr);
    if ((rc = run.candidates(cams, cam_off)) || (rc = run.emit_and_scan(seq_offsets))) return rc;
    const size_t total = (size_t)seq_offsets[n_seq];
    if ((rc = dp.alloc(sizeof(double) * 3 * total)) || (rc = dn.alloc(sizeof(double) * 3 * total))) return rc;
    if ((rc = run.scatter(dp.as<double>(), dn.as<double>(), nullptr, nullptr))) return rc;
    points->resize(3 * total);
    normals->resize(3 * total);
    if ((rc = down(points->data(), dp, 3 * total))) return rc;
    return down(normals->data(), dn, 3 * total);
}

extern "C" {

void mvs_point_sample_default_params(mvs_point_sample_params* p) {
    if (!p) return;
    p->dsp_min = 0.0025; p->dsp_max = 0.3; p->max_dsp_err = 0.01; p->min_conf = 0.9; p->edge_sz_thres = 4.0;
    p->pt_samp_rds = 2; p->nbr_frm_num = 2; p->nbr_frm_step = 1; p->reserved = 0;
}

int mvs_point_sample_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths_dev, const mvs_point_sample_params* p,
                         int64_t* seq_offsets, double* points_dev, double* normals_dev, int32_t* frame_dev, int32_t* pixel_dev, int64_t capacity,
                         void* hip_stream) {
    MVS_TRACE();
    PsPlan pl;
    int rc = check_ps(__func__, n_seq, cam_off, cams, depths_dev, p, seq_offsets, points_dev, normals_dev, capacity, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.cells == 0) { std::memset(seq_offsets, 0, sizeof(int64_t) * ((size_t)n_seq + 1)); return MVS_OK; }
    PsRun run(pl, n_seq, depths_dev, (hipStream_t)hip_stream);
    if ((rc = run.candidates(cams, cam_off)) || (rc = run.emit_and_scan(seq_offsets))) return rc;
    if (seq_offsets[n_seq] > capacity) return too_small(__func__);
    return run.scatter(points_dev, normals_dev, frame_dev, pixel_dev);
}

int mvs_point_sample(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths, const mvs_point_sample_params* p,
                     int64_t* seq_offsets, double* points, double* normals, int32_t* frame, int32_t* pixel, int64_t capacity) {
    MVS_TRACE();
    PsPlan pl;
    int rc = check_ps(__func__, n_seq, cam_off, cams, depths, p, seq_offsets, points, normals, capacity, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    if (pl.cells == 0) { std::memset(seq_offsets, 0, sizeof(int64_t) * ((size_t)n_seq + 1)); return MVS_OK; }
    Scratch dd, dp, dn, df, dx;
    if ((rc = up(dd, depths, (size_t)pl.floats))) return rc;
    PsRun run(pl, n_seq, dd.as<float>(), nullptr);
    if ((rc = run.candidates(cams, cam_off)) || (rc = run.emit_and_scan(seq_offsets))) return rc;
    const size_t total = (size_t)seq_offsets[n_seq];
    if ((int64_t)total > capacity) return too_small(__func__);
    if ((rc = dp.alloc(sizeof(double) * 3 * total)) || (rc = dn.alloc(sizeof(double) * 3 * total)) || (frame && (rc = df.alloc(sizeof(int32_t) * total))) ||
        (pixel && (rc = dx.alloc(sizeof(int32_t) * total)))) return rc;
    if ((rc = run.scatter(dp.as<double>(), dn.as<double>(), frame ? df.as<int32_t>() : nullptr, pixel ? dx.as<int32_t>() : nullptr))) return rc;
    if ((rc = down(points, dp, 3 * total)) || (rc = down(normals, dn, 3 * total))) return rc;
    if (frame && (rc = down(frame, df, total))) return rc;
    return pixel ? down(pixel, dx, total) : MVS_OK;
}

int mvs_test_point_sample_candidates(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths,
                                     const mvs_point_sample_params* p, int64_t* cell_offsets, int32_t* cand, int64_t capacity) {
    MVS_TRACE();
    PsPlan pl;
    int rc = check_ps(__func__, n_seq, cam_off, cams, depths, p, cell_offsets, cand, cand, capacity, &pl);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    for (int k = 0; k < n_seq; ++k) {
        const PsSeq& s = pl.seqs[(size_t)k];
        for (int f = 0; f < s.n; ++f) cell_offsets[s.cam0 + f] = s.cell_off + (int64_t)f * s.cw * s.ch;
    }
    cell_offsets[pl.ncam] = pl.cells;
    if (pl.cells > capacity) return bad(__func__, "capacity is below the number of cells (cell_offsets holds it)");
    if (pl.cells == 0) return MVS_OK;
    Scratch dd;
    if ((rc = up(dd, depths, (size_t)pl.floats))) return rc;
    PsRun run(pl, n_seq, dd.as<float>(), nullptr);
    if ((rc = run.candidates(cams, cam_off))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    return down(cand, run.dcand, (size_t)pl.cells);
}

}  // extern "C"

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_pointsample() { return (const void*)k_ps_candidates; }
