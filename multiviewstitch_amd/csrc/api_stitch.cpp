// api_stitch.cpp — C-ABI of the tail of Processor::AlignmentSeq (R/Processor/Processor.cpp:952-1105): mvs_visibility_cull(_dev),
// mvs_mesh_vertex_normals(_dev) (include/mvs.h) and the two file-level steps mvs_processor_stitch_points / _cull_model
// (include/mvs_io.h); and of Processor::Render (:1140-1192): mvs_render_depth_views(_dev) (include/mvs.h) and the file-level
// mvs_processor_render (include/mvs_io.h); and the file forms of GeometryRec::RunPointSample (:919-949), mvs_processor_point_sample, and of
// GeometryRec::RunPoisson (:1042-1058), mvs_processor_poisson; and the base images of the sequence directories (:532), mvs_processor_load_images,
// with the file form of the depth refinement that reads them, mvs_processor_refine_depths_files.
// The point work is stitch.hip / align.hip / render_views.hip / pointsample.hip / poisson.hip; the host reads and writes the files and builds the
// small tables.
#include "engine.h"
#include "trace.h"
#include "stitch.h"
#include "geom.h"
#include "../../include/mvs_io.h"
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <sys/stat.h>
#include <algorithm>
#include <string>
#include <vector>

namespace {

// the SRT chain and the cameras of every sequence (host arrays): n_seq >= 1, cam_off ascending from 0, cameras of positive size
int check_seqs(const char* fn, int32_t n_seq, const double* scales, const double* R, const double* t, const int32_t* cam_off,
               const mvs_camera* cams) {
    if (n_seq < 1) return bad(fn, "n_seq must be >= 1");
    if (!scales || !R || !t || !cam_off) return bad(fn, "scales, R, t and cam_off must not be NULL");
    if (int rc = check_offsets(fn, "cam_off", cam_off, n_seq)) return rc;
    if (cam_off[n_seq] > 0 && !cams) return bad(fn, "cams is NULL");
    for (int c = 0; c < cam_off[n_seq]; ++c)
        if (cams[c].w <= 0 || cams[c].h <= 0) return bad(fn, "every camera needs w, h > 0");
    return MVS_OK;
}

int check_cull(const char* fn, const int64_t* seg_off, int32_t n_seg, int32_t n_seq, const double* scales, const double* R,
               const double* t, const int32_t* cam_off, const mvs_camera* cams, int32_t mode, const void* points, const void* keep,
               const int64_t* n_keep) {
    int rc = check_seqs(fn, n_seq, scales, R, t, cam_off, cams);
    if (rc) return rc;
    if (n_seg < 1 || !seg_off || !n_keep) return bad(fn, "need n_seg >= 1, seg_off and n_keep");
    if (mode != MVS_CULL_SEQUENCES && mode != MVS_CULL_ALL_SEQ) return bad(fn, "mode must be MVS_CULL_SEQUENCES or MVS_CULL_ALL_SEQ");
    if (mode == MVS_CULL_SEQUENCES && n_seg != n_seq) return bad(fn, "MVS_CULL_SEQUENCES takes one segment per sequence");
    if ((rc = check_offsets(fn, "seg_off", seg_off, n_seg, 0x7fffffffLL))) return rc;
    if (seg_off[n_seg] > 0 && (!points || !keep)) return bad(fn, "points / keep is NULL");
    return MVS_OK;
}

std::string join(const char* dir, const char* name) {
    std::string s(dir);
    if (!s.empty() && s.back() != '/') s += '/';
    return s + name;
}

// the views of Processor::Render: n_seq >= 1, cam_off ascending from 0, at least one camera and cams[0] in sequence 0 (its size is
// the shared viewport), cameras of positive size with cx, cy != 0 (the frustum divides by them), the SRT all given or all NULL,
// 0 < znear < zfar
int check_views(const char* fn, int32_t n_seq, const double* scales, const double* R, const double* t, const int32_t* cam_off,
                const mvs_camera* cams, float znear, float zfar) {
    if (n_seq < 1) return bad(fn, "n_seq must be >= 1");
    if (!cam_off) return bad(fn, "cam_off is NULL");
    if (int rc = check_offsets(fn, "cam_off", cam_off, n_seq)) return rc;
    if (cam_off[n_seq] < 1) return bad(fn, "no cameras");
    if (cam_off[1] < 1) return bad(fn, "cams[0] must belong to sequence 0 (its size is the viewport of every view)");
    if (!cams) return bad(fn, "cams is NULL");
    for (int c = 0; c < cam_off[n_seq]; ++c)
        if (cams[c].w <= 0 || cams[c].h <= 0 || cams[c].cx == 0.0 || cams[c].cy == 0.0) return bad(fn, "every camera needs w, h > 0 and cx, cy != 0");
    if (!((scales && R && t) || (!scales && !R && !t))) return bad(fn, "scales, R and t must all be given or all be NULL");
    if (!(znear > 0) || !(zfar > znear)) return bad(fn, "need 0 < znear < zfar");
    return MVS_OK;
}

int check_render_mesh(const char* fn, const void* pts, int64_t V, const void* faces, int64_t F, const void* out) {
    if (!pts || V <= 0 || V >= 0x7fffffffLL) return bad(fn, "need points and 0 < V < 2^31 - 1");
    if (F < 0 || F >= 0x7fffffffLL / 3 || (F > 0 && !faces)) return bad(fn, "need faces and 0 <= F < (2^31 - 1) / 3");
    if (!out) return bad(fn, "out is NULL");
    return MVS_OK;
}

// CreateDir (R/Common/Utils.h:84-100): every prefix of the path that ends at a '/'
int make_dirs(const std::string& dir) {
    for (size_t i = 1; i < dir.size(); ++i)
        if (dir[i] == '/') {
            const std::string d = dir.substr(0, i);
            if (mkdir(d.c_str(), 0777) != 0 && errno != EEXIST) { mvs_set_error("%s: cannot create the directory (%s)", d.c_str(), std::strerror(errno)); return MVS_E_IO; }
        }
    return MVS_OK;
}

}  // namespace

extern "C" {

int mvs_visibility_cull_dev(const double* points_dev, const int64_t* seg_off, int32_t n_seg, int32_t n_seq, const double* scales,
                            const double* R, const double* t, const int32_t* cam_off, const mvs_camera* cams, int32_t mode,
                            uint8_t* keep_dev, int64_t* n_keep, void* hip_stream) {
    MVS_TRACE();
    int rc = check_cull(__func__, seg_off, n_seg, n_seq, scales, R, t, cam_off, cams, mode, points_dev, keep_dev, n_keep);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return vis_cull_dev(points_dev, seg_off, n_seg, n_seq, scales, R, t, cam_off, cams, mode, keep_dev, nullptr, n_keep,
                        (hipStream_t)hip_stream);
}

int mvs_visibility_cull(const double* points, const int64_t* seg_off, int32_t n_seg, int32_t n_seq, const double* scales,
                        const double* R, const double* t, const int32_t* cam_off, const mvs_camera* cams, int32_t mode, uint8_t* keep,
                        int64_t* n_keep) {
    MVS_TRACE();
    int rc = check_cull(__func__, seg_off, n_seg, n_seq, scales, R, t, cam_off, cams, mode, points, keep, n_keep);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    const int64_t P = seg_off[n_seg];
    Scratch dp, dk;
    if ((rc = up(dp, points, (size_t)P * 3)) || (rc = dk.alloc((size_t)P))) return rc;
    if ((rc = vis_cull_dev(dp.as<double>(), seg_off, n_seg, n_seq, scales, R, t, cam_off, cams, mode, dk.as<uint8_t>(), nullptr, n_keep,
                           nullptr))) return rc;
    return down(keep, dk, (size_t)P);
}

int mvs_mesh_vertex_normals_dev(int64_t V, const double* points_dev, int64_t F, const int32_t* faces_dev, double* out_normals_dev,
                                void* hip_stream) {
    MVS_TRACE();
    if (V < 0 || F < 0 || V >= 0x7fffffffLL || F >= 0x7fffffffLL / 3 || (V > 0 && (!points_dev || !out_normals_dev)) || (F > 0 && !faces_dev))
        return bad(__func__, "bad arguments");
    int rc = need_device();
    if (rc) return rc;
    return mesh_vertex_normals_dev(points_dev, V, faces_dev, F, out_normals_dev, (hipStream_t)hip_stream);
}

int mvs_mesh_vertex_normals(int64_t V, const double* points, int64_t F, const int32_t* faces, double* out_normals) {
    MVS_TRACE();
    if (V < 0 || F < 0 || V >= 0x7fffffffLL || F >= 0x7fffffffLL / 3 || (V > 0 && (!points || !out_normals)) || (F > 0 && !faces))
        return bad(__func__, "bad arguments");
    int rc = need_device();
    if (rc) return rc;
    if (V == 0) return MVS_OK;
    Scratch dp, df, dn;
    if ((rc = up(dp, points, (size_t)V * 3)) || (rc = up(df, faces, (size_t)F * 3)) || (rc = dn.alloc((size_t)V * 24))) return rc;
    if ((rc = mesh_vertex_normals_dev(dp.as<double>(), V, df.as<int32_t>(), F, dn.as<double>(), nullptr))) return rc;
    return down(out_normals, dn, (size_t)V * 3);
}

int mvs_processor_stitch_points(int32_t n_seq, const char* const* npts_paths, const double* scales, const double* R, const double* t,
                                const int32_t* cam_off, const mvs_camera* cams, uint32_t flags, const char* out_dir, int64_t* n_keep) {
    MVS_TRACE();
    int rc = check_seqs(__func__, n_seq, scales, R, t, cam_off, cams);
    if (rc) return rc;
    if (!npts_paths || !out_dir) return bad(__func__, "npts_paths / out_dir is NULL");
    for (int k = 0; k < n_seq; ++k)
        if (!npts_paths[k]) return bad(__func__, "a path of npts_paths is NULL");
    if (flags & ~MVS_STITCH_TRUNCATE) return bad(__func__, "unknown flag");
    if ((rc = need_device())) return rc;
    // :958-963, every sequence into one array (segment k = sequence k)
    std::vector<int64_t> off(n_seq + 1, 0);
    for (int k = 0; k < n_seq; ++k) {
        int64_t n = 0;
        if ((rc = mvs_npts_read(npts_paths[k], &n, nullptr, nullptr))) return rc;
        off[k + 1] = off[k] + n;
    }
    const int64_t P = off[n_seq];
    if (P >= 0x7fffffffLL) return bad(__func__, "more than 2^31 - 1 points");
    std::vector<double> hp((size_t)P * 3), hn((size_t)P * 3);
    for (int k = 0; k < n_seq; ++k) {
        int64_t n = off[k + 1] - off[k];
        if ((rc = mvs_npts_read(npts_paths[k], &n, hp.data() + 3 * off[k], hn.data() + 3 * off[k]))) return rc;
        if (n != off[k + 1] - off[k]) { mvs_set_error("%s changed while it was read", npts_paths[k]); return MVS_E_IO; }
    }
    const int truncate = (flags & MVS_STITCH_TRUNCATE) ? 1 : 0;
    Scratch dp, dn, dk, op, on;
    if ((rc = up(dp, hp.data(), (size_t)P * 3)) || (rc = up(dn, hn.data(), (size_t)P * 3)) || (rc = dk.alloc((size_t)P * 4 + 4)) ||
        (rc = op.alloc((size_t)P * 24)) || (rc = on.alloc((size_t)P * 24))) return rc;
    std::vector<int64_t> nk(n_seq), oo(n_seq + 1);
    if ((rc = vis_cull_dev(dp.as<double>(), off.data(), n_seq, n_seq, scales, R, t, cam_off, cams, MVS_CULL_SEQUENCES, nullptr,
                           dk.as<int32_t>(), nk.data(), nullptr))) return rc;
    if ((rc = stitch_compact_dev(dp.as<double>(), dn.as<double>(), dk.as<int32_t>(), off.data(), n_seq, nk.data(), truncate, scales, R, t,
                                 op.as<double>(), on.as<double>(), oo.data(), nullptr))) return rc;
    const int64_t Q = oo[n_seq];
    if ((rc = down(hp.data(), op, (size_t)Q * 3)) || (rc = down(hn.data(), on, (size_t)Q * 3))) return rc;
    for (int k = 0; k < n_seq; ++k) {                                     // :1029-1030
        char name[32];
        std::snprintf(name, sizeof name, "PSR%d.obj", k);
        if ((rc = mvs_obj_write(join(out_dir, name).c_str(), oo[k + 1] - oo[k], hp.data() + 3 * oo[k], hn.data() + 3 * oo[k], 0, nullptr)))
            return rc;
    }
    if ((rc = mvs_npts_write(join(out_dir, "PSR.npts").c_str(), Q, hp.data(), hn.data()))) return rc;   // :1033-1040
    if (n_keep) std::memcpy(n_keep, nk.data(), sizeof(int64_t) * n_seq);
    return MVS_OK;
}

int mvs_processor_cull_model(const char* model_obj, int32_t n_seq, const double* scales, const double* R, const double* t,
                             const int32_t* cam_off, const mvs_camera* cams, int32_t all_seq_proj, const char* out_obj, int64_t* V_out,
                             int64_t* F_out) {
    MVS_TRACE();
    int rc = check_seqs(__func__, n_seq, scales, R, t, cam_off, cams);
    if (rc) return rc;
    if (!model_obj || !out_obj) return bad(__func__, "model_obj / out_obj is NULL");
    if ((rc = need_device())) return rc;
    int64_t V = 0, N = 0, F = 0;                                          // ReadObj, :1062
    if ((rc = mvs_obj_read(model_obj, &V, &N, &F, nullptr, nullptr, nullptr))) return rc;
    if (N != 0 && N != V) {
        mvs_set_error("%s: %lld normals for %lld vertices (the reference indexes one per vertex)", model_obj, (long long)N, (long long)V);
        return MVS_E_BAD_MESH;
    }
    if (V >= 0x7fffffffLL || F >= 0x7fffffffLL / 3) return bad(__func__, "mesh too large");
    std::vector<double> hp((size_t)V * 3), hn((size_t)V * 3);
    std::vector<int32_t> hf((size_t)F * 3);
    if ((rc = mvs_obj_read(model_obj, &V, &N, &F, hp.data(), hn.data(), hf.data()))) return rc;
    for (int64_t i = 0; i < F * 3; ++i)
        if (hf[i] < 0 || hf[i] >= V) { mvs_set_error("%s: facet index %d outside [1, %lld]", model_obj, hf[i] + 1, (long long)V); return MVS_E_BAD_MESH; }
    Scratch dp, dn, df, dk;
    if ((rc = up(dp, hp.data(), (size_t)V * 3)) || (rc = up(dn, hn.data(), N ? (size_t)V * 3 : 0, (size_t)V * 3)) ||
        (rc = up(df, hf.data(), (size_t)F * 3)) || (rc = dk.alloc((size_t)V * 4 + 4))) return rc;
    // no `vn` lines: CalculateVertexNormals, PlyObj.cpp:11-14
    if (N == 0 && (rc = mesh_vertex_normals_dev(dp.as<double>(), V, df.as<int32_t>(), F, dn.as<double>(), nullptr))) return rc;
    int32_t* keep = nullptr;
    if (all_seq_proj && V > 0) {                                          // :1064-1100
        const int64_t seg[2] = {0, V};
        int64_t nk = 0;
        HIPCHK(hipMemset(dk.p, 0, (size_t)V * 4 + 4));
        if ((rc = vis_cull_dev(dp.as<double>(), seg, 1, n_seq, scales, R, t, cam_off, cams, MVS_CULL_ALL_SEQ, nullptr, dk.as<int32_t>(), &nk,
                               nullptr))) return rc;
        keep = dk.as<int32_t>();
    }
    if ((rc = cull_retain_dev(dp.as<double>(), dn.as<double>(), &V, df.as<int32_t>(), &F, keep))) return rc;   // :1102-1103
    HIPCHK(hipDeviceSynchronize());
    if ((rc = down(hp.data(), dp, (size_t)V * 3)) || (rc = down(hn.data(), dn, (size_t)V * 3)) || (rc = down(hf.data(), df, (size_t)F * 3))) return rc;
    if ((rc = mvs_obj_write(out_obj, V, hp.data(), hn.data(), F, hf.data()))) return rc;                       // :1104
    if (V_out) *V_out = V;
    if (F_out) *F_out = F;
    return MVS_OK;
}

int mvs_render_depth_views_dev(const double* points_dev, int64_t V, const int32_t* faces_dev, int64_t F, int32_t n_seq, const double* scales,
                               const double* R, const double* t, const int32_t* cam_off, const mvs_camera* cams, float znear, float zfar,
                               float* out_dev, void* hip_stream) {
    MVS_TRACE();
    int rc = check_views(__func__, n_seq, scales, R, t, cam_off, cams, znear, zfar);
    if (rc || (rc = check_render_mesh(__func__, points_dev, V, faces_dev, F, out_dev))) return rc;
    if ((rc = need_device())) return rc;
    return render_views_dev(points_dev, V, faces_dev, F, n_seq, scales, R, t, cam_off, cams, znear, zfar, out_dev, (hipStream_t)hip_stream);
}

int mvs_render_depth_views(const double* points, int64_t V, const int32_t* faces, int64_t F, int32_t n_seq, const double* scales,
                           const double* R, const double* t, const int32_t* cam_off, const mvs_camera* cams, float znear, float zfar,
                           float* out) {
    MVS_TRACE();
    int rc = check_views(__func__, n_seq, scales, R, t, cam_off, cams, znear, zfar);
    if (rc || (rc = check_render_mesh(__func__, points, V, faces, F, out))) return rc;
    for (int64_t k = 0; k < 3 * F; ++k)
        if (faces[k] < 0 || faces[k] >= V) { mvs_set_error("%s: facet index out of range", __func__); return MVS_E_BAD_MESH; }
    if ((rc = need_device())) return rc;
    const size_t n_out = (size_t)cam_off[n_seq] * (size_t)cams[0].w * (size_t)cams[0].h;
    Scratch dp, df, dout;
    if ((rc = up(dp, points, 3 * (size_t)V)) || (rc = up(df, faces, 3 * (size_t)F)) || (rc = dout.alloc(sizeof(float) * n_out))) return rc;
    if ((rc = render_views_dev(dp.as<double>(), V, df.as<int32_t>(), F, n_seq, scales, R, t, cam_off, cams, znear, zfar, dout.as<float>(),
                               nullptr))) return rc;
    return down(out, dout, n_out);
}

int mvs_processor_render(const char* deform_obj, const char* srt_txt, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams,
                         const char* result_dir, const char* const* seq_dirs, float znear, float zfar, int64_t* n_views_out) {
    MVS_TRACE();
    int rc = check_views(__func__, n_seq, nullptr, nullptr, nullptr, cam_off, cams, znear, zfar);
    if (rc) return rc;
    if (!deform_obj || !srt_txt || !result_dir || !seq_dirs) return bad(__func__, "deform_obj, srt_txt, result_dir and seq_dirs must not be NULL");
    for (int k = 0; k < n_seq; ++k)
        if (!seq_dirs[k]) return bad(__func__, "a path of seq_dirs is NULL");
    if ((rc = need_device())) return rc;
    std::vector<double> sc(n_seq), R((size_t)n_seq * 9), t((size_t)n_seq * 3);
    if ((rc = mvs_srt_txt_read(srt_txt, n_seq, sc.data(), R.data(), t.data()))) return rc;          // :1145-1165, through float32
    int64_t V = 0, N = 0, F = 0;                                                                   // ReadObj, :1170
    if ((rc = mvs_obj_read(deform_obj, &V, &N, &F, nullptr, nullptr, nullptr))) return rc;
    if (N != 0 && N != V) {
        mvs_set_error("%s: %lld normals for %lld vertices (the reference indexes one per vertex)", deform_obj, (long long)N, (long long)V);
        return MVS_E_BAD_MESH;
    }
    if (V <= 0 || V >= 0x7fffffffLL || F >= 0x7fffffffLL / 3) { mvs_set_error("%s: no vertices, or mesh too large", deform_obj); return MVS_E_BAD_MESH; }
    std::vector<double> hp((size_t)V * 3), hn((size_t)V * 3);
    std::vector<int32_t> hf((size_t)F * 3);
    if ((rc = mvs_obj_read(deform_obj, &V, &N, &F, hp.data(), hn.data(), hf.data()))) return rc;
    for (int64_t i = 0; i < F * 3; ++i)
        if (hf[i] < 0 || hf[i] >= V) { mvs_set_error("%s: facet index %d outside [1, %lld]", deform_obj, hf[i] + 1, (long long)V); return MVS_E_BAD_MESH; }
    const int n_views = cam_off[n_seq];
    const size_t npx = (size_t)cams[0].w * (size_t)cams[0].h;
    Scratch dp, dn, df, mp, mn, dout;
    if ((rc = up(dp, hp.data(), (size_t)V * 3)) || (rc = up(dn, hn.data(), N ? (size_t)V * 3 : 0, (size_t)V * 3)) ||
        (rc = up(df, hf.data(), (size_t)F * 3)) || (rc = mp.alloc((size_t)V * 24)) || (rc = mn.alloc((size_t)V * 24)) ||
        (rc = dout.alloc(sizeof(float) * npx * n_views))) return rc;
    // no `vn` lines: CalculateVertexNormals, PlyObj.cpp:11-14
    if (N == 0 && (rc = mesh_vertex_normals_dev(dp.as<double>(), V, df.as<int32_t>(), F, dn.as<double>(), nullptr))) return rc;
    std::vector<double> op((size_t)V * 3), on((size_t)V * 3);
    for (int k = 0; k < n_seq; ++k) {                                                              // :1176-1189
        launch_srt_apply(dp.as<double>(), dn.as<double>(), V, sc[k], R.data() + 9 * k, t.data() + 3 * k, 1, mp.as<double>(), mn.as<double>(), nullptr);
        HIPCHK(hipGetLastError());
        if ((rc = down(op.data(), mp, (size_t)V * 3)) || (rc = down(on.data(), mn, (size_t)V * 3))) return rc;
        char name[32];
        std::snprintf(name, sizeof name, "render%d.obj", k);
        if ((rc = mvs_obj_write(join(result_dir, name).c_str(), V, op.data(), on.data(), F, hf.data()))) return rc;
    }
    // Model2Depth::SetInput + Run (Model2Depth.h, Model2Depth.cpp:58-190): every camera of every sequence, in order
    if ((rc = render_views_dev(dp.as<double>(), V, df.as<int32_t>(), F, n_seq, sc.data(), R.data(), t.data(), cam_off, cams, znear, zfar,
                               dout.as<float>(), nullptr))) return rc;
    std::vector<float> hr(npx * n_views);
    if ((rc = down(hr.data(), dout, hr.size()))) return rc;
    std::vector<double> raw(npx);
    for (int k = 0; k < n_seq; ++k) {
        if (cam_off[k + 1] == cam_off[k]) continue;                                               // a sequence without cameras renders nothing
        const std::string dir = join(seq_dirs[k], "DATA/Render/");                                // RenderDepth, :145
        if ((rc = make_dirs(dir))) return rc;
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            for (size_t i = 0; i < npx; ++i) raw[i] = hr[(size_t)c * npx + i];
            char name[32];
            std::snprintf(name, sizeof name, "_depth%d.raw", c - cam_off[k]);
            if ((rc = mvs_depth_raw_write((dir + name).c_str(), (int64_t)npx, raw.data()))) return rc;   // SaveDepth, :151-153
        }
    }
    if (n_views_out) *n_views_out = n_views;
    return MVS_OK;
}

// the checks the file forms of the depth refinement share
static int check_seq_dirs(const char* fn, int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams, size_t* px) {
    if (n_seq < 1) return bad(fn, "n_seq must be >= 1");
    if (!seq_dirs || !cam_off || !cams) return bad(fn, "seq_dirs, cam_off and cams must not be NULL");
    for (int k = 0; k < n_seq; ++k)
        if (!seq_dirs[k]) return bad(fn, "a path of seq_dirs is NULL");
    int rc = check_offsets(fn, "cam_off", cam_off, n_seq);
    if (rc) return rc;
    *px = 0;
    for (int c = 0; c < cam_off[n_seq]; ++c) {
        if (cams[c].w <= 0 || cams[c].h <= 0) return bad(fn, "every camera needs w, h > 0");
        *px += (size_t)cams[c].w * (size_t)cams[c].h;
    }
    return MVS_OK;
}

// DATA/Render -> mvs_refine_depth_maps -> DATA/Refine for checked arguments, under the name fn
static int refine_depths_body(const char* fn, int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                              const uint8_t* imgs, const mvs_depth_refine_params* params, size_t floats) {
    int rc;
    mvs_depth_refine_params prm;
    if (params) prm = *params; else mvs_depth_refine_default_params(&prm);
    std::vector<float> ras(floats ? floats : 1), out(floats ? floats : 1);                        // the rasters of DATA/Render, DepthOptimizer.cpp:28-31
    size_t at = 0;
    for (int k = 0; k < n_seq; ++k)
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            char name[48];
            std::snprintf(name, sizeof name, "DATA/Render/_depth%d.raw", c - cam_off[k]);
            if ((rc = mvs_depth_raw_read(join(seq_dirs[k], name).c_str(), cams[c].w, cams[c].h, ras.data() + at))) return rc;
            at += (size_t)cams[c].w * (size_t)cams[c].h;
        }
    if ((rc = refine_depth_maps_host(fn, n_seq, cam_off, cams, imgs, ras.data(), &prm, out.data(), nullptr, nullptr, nullptr))) return rc;
    std::vector<double> raw;
    at = 0;
    for (int k = 0; k < n_seq; ++k) {                                                             // DATA/Refine, :36-40
        if (cam_off[k + 1] == cam_off[k]) continue;
        const std::string dir = join(seq_dirs[k], "DATA/Refine/");
        if ((rc = make_dirs(dir))) return rc;
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            const size_t npx = (size_t)cams[c].w * (size_t)cams[c].h;
            raw.assign(out.begin() + (std::ptrdiff_t)at, out.begin() + (std::ptrdiff_t)(at + npx));
            char name[32];
            std::snprintf(name, sizeof name, "_depth%d.raw", c - cam_off[k]);
            if ((rc = mvs_depth_raw_write((dir + name).c_str(), (int64_t)npx, raw.data()))) return rc;
            at += npx;
        }
    }
    return MVS_OK;
}

int mvs_processor_refine_depths(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                                const mvs_depth_refine_params* params) {
    MVS_TRACE();
    if (n_seq < 1) return bad(__func__, "n_seq must be >= 1");
    if (!seq_dirs || !cam_off || !cams || !imgs) return bad(__func__, "seq_dirs, cam_off, cams and imgs must not be NULL");
    size_t floats = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &floats);
    if (rc) return rc;
    return refine_depths_body(__func__, n_seq, seq_dirs, cam_off, cams, imgs, params, floats);
}

// <seq_dirs[k]>%05d.jpg of every camera into `out` (all cameras back to back), under the name fn: the files read on host threads, then one
// mvs_jpeg_decode per size; nothing is written to `out` before every file has been read and every stream walked
static int load_images_body(const char* fn, int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                            uint32_t flags, uint8_t* out) {
    const int ncam = cam_off[n_seq];
    if (ncam == 0) return MVS_OK;
    std::vector<std::string> path((size_t)ncam), blob((size_t)ncam);
    std::vector<int> err((size_t)ncam, 0);
    for (int k = 0; k < n_seq; ++k)
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            char name[24];
            std::snprintf(name, sizeof name, "%05d.jpg", c - cam_off[k]);                          // Processor.cpp:532
            path[(size_t)c] = join(seq_dirs[k], name);
        }
    const int nt = io_threads(ncam, IO_UNKNOWN);
    parallel_parts(nt, [&](int t) {
        for (int c = t; c < ncam; c += nt) {
            FILE* f = std::fopen(path[(size_t)c].c_str(), "rb");
            if (!f) { err[(size_t)c] = errno ? errno : EIO; continue; }
            char buf[1 << 16];
            size_t got;
            while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) blob[(size_t)c].append(buf, got);
            if (std::ferror(f)) err[(size_t)c] = EIO;
            std::fclose(f);
        }
    });
    for (int c = 0; c < ncam; ++c)
        if (err[(size_t)c]) { mvs_set_error("%s: %s: %s", fn, path[(size_t)c].c_str(), std::strerror(err[(size_t)c])); return MVS_E_IO; }
    // the cameras by size, in the order of their first camera; pass 0 walks the streams and checks the sizes, pass 1 decodes
    std::vector<char> done((size_t)ncam, 0);
    std::vector<int64_t> px0((size_t)ncam + 1, 0);
    for (int c = 0; c < ncam; ++c) px0[(size_t)c + 1] = px0[(size_t)c] + (int64_t)cams[c].w * cams[c].h;
    for (int pass = 0; pass < 2; ++pass) {
        std::fill(done.begin(), done.end(), 0);
        for (int c0 = 0; c0 < ncam; ++c0) {
            if (done[(size_t)c0]) continue;
            std::vector<int> grp;
            std::vector<int64_t> off(1, 0);
            std::string data;
            for (int c = c0; c < ncam; ++c)
                if (cams[c].w == cams[c0].w && cams[c].h == cams[c0].h) {
                    done[(size_t)c] = 1;
                    grp.push_back(c);
                    data += blob[(size_t)c];
                    off.push_back((int64_t)data.size());
                }
            const size_t npx = (size_t)cams[c0].w * (size_t)cams[c0].h;
            std::vector<uint8_t> px(pass ? grp.size() * npx * 3 : 0);
            int32_t w = 0, h = 0;
            int rc = jpeg_decode_host(fn, (int32_t)grp.size(), off.data(), (const uint8_t*)data.data(), flags, pass ? px.data() : nullptr, &w, &h);
            if (rc) {                                                                              // the index of a group -> the file
                const std::string why = mvs_last_error();
                const size_t at = why.find("image ");
                if (at != std::string::npos) {
                    const int i = std::atoi(why.c_str() + at + 6);
                    if (i >= 0 && i < (int)grp.size()) mvs_set_error("%s (%s)", why.c_str(), path[(size_t)grp[(size_t)i]].c_str());
                }
                return rc;
            }
            if (w != cams[c0].w || h != cams[c0].h) {
                mvs_set_error("%s: %s is %d x %d, its camera %d x %d", fn, path[(size_t)c0].c_str(), w, h, cams[c0].w, cams[c0].h);
                return MVS_E_INVALID_ARG;
            }
            for (size_t i = 0; pass && i < grp.size(); ++i) std::memcpy(out + 3 * px0[(size_t)grp[i]], px.data() + i * npx * 3, npx * 3);
        }
        if (pass == 0)
            if (int rc = need_device()) return rc;
    }
    return MVS_OK;
}

int mvs_processor_load_images(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams, uint32_t flags,
                              uint8_t* imgs) {
    MVS_TRACE();
    size_t px = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &px);
    if (rc) return rc;
    if (!imgs) return bad(__func__, "imgs is NULL");
    if (flags & ~(uint32_t)MVS_JPEG_RGB) return bad(__func__, "unknown flag bits");
    return load_images_body(__func__, n_seq, seq_dirs, cam_off, cams, flags, imgs);
}

int mvs_processor_refine_depths_files(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                      const mvs_depth_refine_params* params) {
    MVS_TRACE();
    size_t px = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &px);
    if (rc) return rc;
    std::vector<uint8_t> imgs(px ? 3 * px : 1);
    if ((rc = load_images_body(__func__, n_seq, seq_dirs, cam_off, cams, MVS_JPEG_RGB, imgs.data()))) return rc;
    return refine_depths_body(__func__, n_seq, seq_dirs, cam_off, cams, imgs.data(), params, px);
}

// mvs_recover_depth_maps (or, with `aggregated`, mvs_recover_depth_maps_aggregated under ap) -> DATA/_depth<i>.raw for checked
// arguments, under the name fn; nothing is written when the call fails
static int recover_depths_body(const char* fn, int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                               const uint8_t* imgs, const mvs_depth_recover_params* params, size_t floats, bool aggregated = false,
                               const mvs_depth_aggregate_params* ap = nullptr) {
    int rc;
    mvs_depth_recover_params prm;
    if (params) prm = *params; else mvs_depth_recover_default_params(&prm);
    std::vector<float> out(floats ? floats : 1);
    rc = aggregated ? recover_depth_maps_aggregated_host(fn, n_seq, cam_off, cams, imgs, &prm, ap, out.data(), nullptr, nullptr, nullptr, nullptr)
                    : recover_depth_maps_host(fn, n_seq, cam_off, cams, imgs, &prm, out.data(), nullptr, nullptr, nullptr);
    if (rc) return rc;
    std::vector<double> raw;
    size_t at = 0;
    for (int k = 0; k < n_seq; ++k) {                                                             // what Processor.cpp:37-38 reads
        if (cam_off[k + 1] == cam_off[k]) continue;
        const std::string dir = join(seq_dirs[k], "DATA/");
        if ((rc = make_dirs(dir))) return rc;
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            const size_t npx = (size_t)cams[c].w * (size_t)cams[c].h;
            raw.assign(out.begin() + (std::ptrdiff_t)at, out.begin() + (std::ptrdiff_t)(at + npx));
            char name[32];
            std::snprintf(name, sizeof name, "_depth%d.raw", c - cam_off[k]);
            if ((rc = mvs_depth_raw_write((dir + name).c_str(), (int64_t)npx, raw.data()))) return rc;
            at += npx;
        }
    }
    return MVS_OK;
}

int mvs_processor_recover_depths(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                                 const mvs_depth_recover_params* params) {
    MVS_TRACE();
    if (n_seq < 1) return bad(__func__, "n_seq must be >= 1");
    if (!seq_dirs || !cam_off || !cams || !imgs) return bad(__func__, "seq_dirs, cam_off, cams and imgs must not be NULL");
    size_t floats = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &floats);
    if (rc) return rc;
    return recover_depths_body(__func__, n_seq, seq_dirs, cam_off, cams, imgs, params, floats);
}

int mvs_processor_recover_depths_files(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                       const mvs_depth_recover_params* params) {
    MVS_TRACE();
    size_t px = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &px);
    if (rc) return rc;
    std::vector<uint8_t> imgs(px ? 3 * px : 1);
    if ((rc = load_images_body(__func__, n_seq, seq_dirs, cam_off, cams, MVS_JPEG_RGB, imgs.data()))) return rc;
    return recover_depths_body(__func__, n_seq, seq_dirs, cam_off, cams, imgs.data(), params, px);
}

int mvs_processor_recover_depths_aggregated(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                            const uint8_t* imgs, const mvs_depth_recover_params* params,
                                            const mvs_depth_aggregate_params* aggregate) {
    MVS_TRACE();
    if (n_seq < 1) return bad(__func__, "n_seq must be >= 1");
    if (!seq_dirs || !cam_off || !cams || !imgs) return bad(__func__, "seq_dirs, cam_off, cams and imgs must not be NULL");
    size_t floats = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &floats);
    if (rc) return rc;
    return recover_depths_body(__func__, n_seq, seq_dirs, cam_off, cams, imgs, params, floats, true, aggregate);
}

int mvs_processor_recover_depths_aggregated_files(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                                  const mvs_depth_recover_params* params, const mvs_depth_aggregate_params* aggregate) {
    MVS_TRACE();
    size_t px = 0;
    int rc = check_seq_dirs(__func__, n_seq, seq_dirs, cam_off, cams, &px);
    if (rc) return rc;
    mvs_depth_recover_params prm;                                                                // every parameter error before a frame is read
    if (params) prm = *params; else mvs_depth_recover_default_params(&prm);
    if ((rc = recover_depth_maps_aggregated_check(__func__, n_seq, cam_off, cams, &prm, aggregate))) return rc;
    std::vector<uint8_t> imgs(px ? 3 * px : 1);
    if ((rc = load_images_body(__func__, n_seq, seq_dirs, cam_off, cams, MVS_JPEG_RGB, imgs.data()))) return rc;
    return recover_depths_body(__func__, n_seq, seq_dirs, cam_off, cams, imgs.data(), &prm, px, true, aggregate);
}

int mvs_processor_colour_model(const char* model_obj, const char* srt_txt, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams,
                               const char* const* seq_dirs, const mvs_colour_params* params, float znear, float zfar, const char* out_obj,
                               int64_t* n_coloured) {
    MVS_TRACE();
    int rc = check_views(__func__, n_seq, nullptr, nullptr, nullptr, cam_off, cams, znear, zfar);
    if (rc || (rc = colour_check_views(__func__, n_seq, nullptr, nullptr, nullptr, cam_off, cams))) return rc;
    mvs_colour_params prm;
    if (params) prm = *params; else mvs_colour_default_params(&prm);
    if ((rc = colour_check_params(__func__, &prm))) return rc;
    if (!model_obj || !srt_txt || !seq_dirs || !out_obj) return bad(__func__, "model_obj, srt_txt, seq_dirs and out_obj must not be NULL");
    for (int k = 0; k < n_seq; ++k)
        if (!seq_dirs[k]) return bad(__func__, "a path of seq_dirs is NULL");
    if ((rc = need_device())) return rc;
    std::vector<double> sc(n_seq), R((size_t)n_seq * 9), t((size_t)n_seq * 3);
    if ((rc = mvs_srt_txt_read(srt_txt, n_seq, sc.data(), R.data(), t.data()))) return rc;          // through float32, as mvs_processor_render
    int64_t V = 0, N = 0, F = 0;
    if ((rc = mvs_obj_read(model_obj, &V, &N, &F, nullptr, nullptr, nullptr))) return rc;
    if (N != 0 && N != V) {
        mvs_set_error("%s: %lld normals for %lld vertices (the reference indexes one per vertex)", model_obj, (long long)N, (long long)V);
        return MVS_E_BAD_MESH;
    }
    if (V <= 0 || V >= 0x7fffffffLL || F >= 0x7fffffffLL / 3) { mvs_set_error("%s: no vertices, or mesh too large", model_obj); return MVS_E_BAD_MESH; }
    std::vector<double> hp((size_t)V * 3), hn((size_t)V * 3);
    std::vector<int32_t> hf((size_t)F * 3);
    if ((rc = mvs_obj_read(model_obj, &V, &N, &F, hp.data(), hn.data(), hf.data()))) return rc;
    for (int64_t i = 0; i < F * 3; ++i)
        if (hf[i] < 0 || hf[i] >= V) { mvs_set_error("%s: facet index %d outside [1, %lld]", model_obj, hf[i] + 1, (long long)V); return MVS_E_BAD_MESH; }
    const int n_views = cam_off[n_seq];
    const size_t npx = (size_t)cams[0].w * (size_t)cams[0].h * (size_t)n_views;
    std::vector<uint8_t> himg(3 * npx);
    if ((rc = load_images_body(__func__, n_seq, seq_dirs, cam_off, cams, MVS_JPEG_RGB, himg.data()))) return rc;
    Scratch dp, dn, df, di, dras, dc, dk;
    if ((rc = up(dp, hp.data(), (size_t)V * 3)) || (rc = up(dn, hn.data(), N ? (size_t)V * 3 : 0, (size_t)V * 3)) ||
        (rc = up(df, hf.data(), (size_t)F * 3)) || (rc = up(di, himg.data(), 3 * npx)) || (F && (rc = dras.alloc(sizeof(float) * npx))) ||
        (rc = dc.alloc((size_t)V * 3)) || (rc = dk.alloc(sizeof(int32_t) * (size_t)V))) return rc;
    // no `vn` lines: CalculateVertexNormals, PlyObj.cpp:11-14
    if (N == 0 && (rc = mesh_vertex_normals_dev(dp.as<double>(), V, df.as<int32_t>(), F, dn.as<double>(), nullptr))) return rc;
    if (F && (rc = render_views_dev(dp.as<double>(), V, df.as<int32_t>(), F, n_seq, sc.data(), R.data(), t.data(), cam_off, cams, znear, zfar,
                                    dras.as<float>(), nullptr))) return rc;
    if ((rc = colour_vertices_dev(__func__, dp.as<double>(), dn.as<double>(), V, n_seq, sc.data(), R.data(), t.data(), cam_off, cams, di.as<uint8_t>(),
                                  F ? dras.as<float>() : nullptr, &prm, dc.as<uint8_t>(), dk.as<int32_t>(), nullptr))) return rc;
    std::vector<uint8_t> hc((size_t)V * 3);
    std::vector<int32_t> hk((size_t)V);
    if ((rc = down(hc.data(), dc, hc.size())) || (rc = down(hk.data(), dk, hk.size()))) return rc;
    const bool with_normals = N != 0 || F != 0;
    if (N == 0 && F != 0 && (rc = down(hn.data(), dn, (size_t)V * 3))) return rc;
    if ((rc = mvs_obj_write_coloured(out_obj, V, hp.data(), with_normals ? hn.data() : nullptr, hc.data(), MVS_JPEG_RGB, F, hf.data()))) return rc;
    if (n_coloured) {
        int64_t n = 0;
        for (int32_t k : hk) n += k > 0;
        *n_coloured = n;
    }
    return MVS_OK;
}

// stream i = data[off[i] .. off[i + 1]) to path[i], on up to 16 host threads; the first file that fails is reported
static int write_streams(const char* fn, const std::vector<std::string>& path, const int64_t* off, const uint8_t* data) {
    const int n = (int)path.size();
    std::vector<int> err((size_t)n, 0);
    const int nt = io_threads(n, IO_UNKNOWN);
    parallel_parts(nt, [&](int t) {
        for (int i = t; i < n; i += nt) {
            FILE* f = std::fopen(path[(size_t)i].c_str(), "wb");
            if (!f) { err[(size_t)i] = errno ? errno : EIO; continue; }
            const size_t len = (size_t)(off[i + 1] - off[i]);
            if (std::fwrite(data + off[i], 1, len, f) != len) err[(size_t)i] = EIO;
            if (std::fclose(f)) err[(size_t)i] = EIO;
        }
    });
    for (int i = 0; i < n; ++i)
        if (err[(size_t)i]) { mvs_set_error("%s: %s: %s", fn, path[(size_t)i].c_str(), std::strerror(err[(size_t)i])); return MVS_E_IO; }
    return MVS_OK;
}

int mvs_processor_save_views(const char* seq_dir, int32_t n_frames, int32_t view_count, int32_t w, int32_t h, const uint8_t* views, uint32_t flags,
                             const mvs_jpeg_encode_params* params) {
    MVS_TRACE();
    if (!seq_dir || !views) return bad(__func__, "seq_dir or views is NULL");
    if (n_frames < 1 || view_count < 1 || (int64_t)n_frames * view_count > 65535) return bad(__func__, "need n_frames, view_count >= 1 and at most 65535 views");
    if (flags & ~(uint32_t)MVS_JPEG_RGB) return bad(__func__, "unknown flag bits");
    const int n = n_frames * view_count;
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<uint8_t> data;
    int rc = jpeg_encode_host(__func__, n, w, h, views, flags, params, off.data(), &data);
    if (rc) return rc;
    const std::string dir = join(seq_dir, "Views/");
    if ((rc = make_dirs(dir))) return rc;
    std::vector<std::string> path;
    for (int i = 0; i < n_frames; ++i)
        for (int j = 0; j < view_count; ++j) {
            char name[48];
            std::snprintf(name, sizeof name, "proj%d_%d.jpg", i, j);                               // Image3D.cpp:218
            path.push_back(dir + name);
        }
    return write_streams(__func__, path, off.data(), data.data());
}

int mvs_processor_depth_previews(const char* seq_dir, const char* sub, int32_t n, int32_t w, int32_t h, const mvs_jpeg_encode_params* params) {
    MVS_TRACE();
    if (!seq_dir || !sub) return bad(__func__, "seq_dir or sub is NULL");
    if (std::strcmp(sub, "CHECK") && std::strcmp(sub, "Render") && std::strcmp(sub, "Refine")) return bad(__func__, "sub must be CHECK, Render or Refine");
    if (n < 1 || n > 65535) return bad(__func__, "need n in 1 .. 65535");
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return bad(__func__, "w and h must be in 1 .. 65535");
    const size_t npx = (size_t)w * (size_t)h;
    const std::string dir = join(seq_dir, (std::string("DATA/") + sub + "/").c_str());
    std::vector<float> ras((size_t)n * npx);
    std::vector<std::string> path;
    int rc;
    for (int i = 0; i < n; ++i) {
        char name[32];
        std::snprintf(name, sizeof name, "_depth%d", i);
        if ((rc = mvs_depth_raw_read((dir + name + ".raw").c_str(), w, h, ras.data() + (size_t)i * npx))) return rc;
        path.push_back(dir + name + ".jpg");
    }
    std::vector<uint8_t> grey((size_t)n * npx), data;
    std::vector<int64_t> off((size_t)n + 1);
    if ((rc = depth_preview_host(__func__, n, w, h, ras.data(), grey.data())) ||
        (rc = jpeg_encode_host(__func__, n, w, h, grey.data(), MVS_JPEG_GREY, params, off.data(), &data))) return rc;
    return write_streams(__func__, path, off.data(), data.data());
}

// the sink of the overlay producers (stitch.h): canvas c goes to dir + name(c); the directory is created in front of the first batch
static OverlaySink overlay_files(const char* fn, const std::string& dir, std::function<std::string(int32_t)> name) {
    return [fn, dir, name](int32_t first, int32_t count, const int64_t* off, const uint8_t* data) {
        if (first == 0)
            if (int rc = make_dirs(dir)) return rc;
        std::vector<std::string> path;
        for (int32_t c = first; c < first + count; ++c) path.push_back(dir + name(c));
        return write_streams(fn, path, off, data);
    };
}

int mvs_processor_match_overlays(const char* match_dir, int32_t k, int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1,
                                 const uint8_t* imgs2, const int64_t* match_offsets, const int32_t* matches, uint32_t flags, uint64_t* rng_state,
                                 const mvs_jpeg_encode_params* params) {
    MVS_TRACE();
    if (!match_dir) return bad(__func__, "match_dir is NULL");
    if (k < 0) return bad(__func__, "k must be >= 0");
    const auto name = [k, n2](int32_t c) {
        char s[64];
        std::snprintf(s, sizeof s, "match%d_%d_%d.jpg", k, c / n2, c % n2);                         // Processor.cpp:787
        return std::string(s);
    };
    return match_overlay_streams(__func__, n1, n2, w, h, imgs1, imgs2, match_offsets, matches, flags, rng_state, params,
                                 overlay_files(__func__, join(match_dir, ""), name));
}

int mvs_processor_sift_overlays(const char* seq_dir, const char* sub, int32_t n_frames, int32_t view_count, int32_t w, int32_t h,
                                const uint8_t* views, const int64_t* key_offsets, const float* keys, uint32_t flags,
                                const mvs_jpeg_encode_params* params) {
    MVS_TRACE();
    if (!seq_dir || !sub) return bad(__func__, "seq_dir or sub is NULL");
    if (std::strcmp(sub, "Sift") && std::strcmp(sub, "Sift1")) return bad(__func__, "sub must be Sift or Sift1");
    if (n_frames < 1 || view_count < 1 || (int64_t)n_frames * view_count > 65535)
        return bad(__func__, "need n_frames, view_count >= 1 and at most 65535 views");
    const auto name = [view_count](int32_t c) {
        char s[48];
        std::snprintf(s, sizeof s, "proj%d_%d.jpg", c / view_count, c % view_count);                // FeatureProc.cpp:71, Processor.cpp:612
        return std::string(s);
    };
    return sift_overlay_streams(__func__, n_frames * view_count, w, h, views, key_offsets, keys, flags, params,
                                overlay_files(__func__, join(seq_dir, (std::string("Views/") + sub + "/").c_str()), name));
}

int mvs_processor_point_sample(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                               const mvs_point_sample_params* params, const char* const* npts_paths, int64_t* n_points) {
    MVS_TRACE();
    if (n_seq < 1) return bad(__func__, "n_seq must be >= 1");
    if (!seq_dirs || !cam_off || !cams) return bad(__func__, "seq_dirs, cam_off and cams must not be NULL");
    for (int k = 0; k < n_seq; ++k)
        if (!seq_dirs[k]) return bad(__func__, "a path of seq_dirs is NULL");
    int rc = check_offsets(__func__, "cam_off", cam_off, n_seq);
    if (rc) return rc;
    size_t floats = 0;
    for (int c = 0; c < cam_off[n_seq]; ++c) {
        if (cams[c].w <= 0 || cams[c].h <= 0) return bad(__func__, "every camera needs w, h > 0");
        floats += (size_t)cams[c].w * (size_t)cams[c].h;
    }
    mvs_point_sample_params prm;
    if (params) prm = *params; else mvs_point_sample_default_params(&prm);
    std::vector<float> ras(floats ? floats : 1);                                                   // the rasters of DATA/CHECK, :919-931
    size_t at = 0;
    for (int k = 0; k < n_seq; ++k)
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            char name[48];
            std::snprintf(name, sizeof name, "DATA/CHECK/_depth%d.raw", c - cam_off[k]);
            if ((rc = mvs_depth_raw_read(join(seq_dirs[k], name).c_str(), cams[c].w, cams[c].h, ras.data() + at))) return rc;
            at += (size_t)cams[c].w * (size_t)cams[c].h;
        }
    std::vector<int64_t> off((size_t)n_seq + 1);
    std::vector<double> pts, nrm;
    if ((rc = point_sample_vectors(__func__, n_seq, cam_off, cams, ras.data(), &prm, off.data(), &pts, &nrm))) return rc;
    for (int k = 0; k < n_seq; ++k) {                                                              // Rec/*.npts, :933-949
        const bool own = npts_paths && npts_paths[k];
        const std::string dir = join(seq_dirs[k], "Rec/");
        if (!own && (rc = make_dirs(dir))) return rc;
        const std::string path = own ? std::string(npts_paths[k]) : dir + "PointSample.npts";
        if ((rc = mvs_npts_write(path.c_str(), off[k + 1] - off[k], pts.data() + 3 * off[k], nrm.data() + 3 * off[k]))) return rc;
        if (n_points) n_points[k] = off[k + 1] - off[k];
    }
    return MVS_OK;
}

// PSR.npts -> Model.obj; dprm != NULL: through rules 14-17, and trimmed by rule 18 when trim_ratio > 0; sprm != NULL (with dprm): rules 19-23
static int poisson_files(const char* fn, const char* psr_npts, const mvs_poisson_params& prm, const mvs_poisson_density_params* dprm, double trim_ratio,
                         const char* model_obj, int64_t* V_out, int64_t* F_out, const mvs_poisson_screen_params* sprm,
                         const mvs_poisson_band_params* bprm = nullptr /*alone: rules 24-31; with dprm: rules 32-35; with sprm too: rules 36-41*/,
                         int64_t* open_out = nullptr) {
    int rc = need_device();
    if (rc) return rc;
    int64_t n = 0;
    if ((rc = mvs_npts_read(psr_npts, &n, nullptr, nullptr))) return rc;
    std::vector<double> hp((size_t)n * 3 + 1), hn((size_t)n * 3 + 1);
    int64_t m = n;
    if ((rc = mvs_npts_read(psr_npts, &m, hp.data(), hn.data()))) return rc;
    if (m != n) { mvs_set_error("%s changed while it was read", psr_npts); return MVS_E_IO; }
    Scratch dp, dn, dv, df, dvn, dd, tv, tf;
    mvs_poisson_info info;
    mvs_poisson_density_info dinfo;
    mvs_poisson_screen_info sinfo;
    if ((rc = up(dp, hp.data(), (size_t)n * 3)) || (rc = up(dn, hn.data(), (size_t)n * 3))) return rc;
    const PnCall call{fn, sprm ? PN_SCREENED : dprm ? PN_DENSITY : PN_PLAIN, n, dp.as<double>(), dn.as<double>(), &prm, &info, dprm, dprm ? &dinfo : nullptr,
                      sprm, sprm ? &sinfo : nullptr};
    mvs_poisson_band_info binfo;
    if (bprm) {
        mvs_poisson_band_screen_info bsinfo;
        const bool screen = dprm && sprm;
        const BdCall band{fn, n, dp.as<double>(), dn.as<double>(), &prm, bprm, &info, &binfo, dprm, dprm ? &dinfo : nullptr, dprm != nullptr,
                          screen ? sprm : nullptr, screen ? &sinfo : nullptr, screen ? &bsinfo : nullptr, screen};
        if ((rc = poisson_band_blocks(band, &dv, &dd, &df))) return rc;
        if (open_out) *open_out = binfo.n_open_edges;
    } else if ((rc = poisson_blocks(call, &dv, &dd, &df))) return rc;
    int64_t V = info.n_vertices, F = info.n_faces;
    const Scratch *mv = &dv, *mf = &df;
    if (dprm && trim_ratio > 0.0) {
        if ((rc = tv.alloc((size_t)V * 24)) || (rc = tf.alloc((size_t)F * 12)) ||
            (rc = mesh_trim_dev(V, dv.as<double>(), nullptr, F, df.as<int32_t>(), dd.as<double>(), trim_ratio * dinfo.mean_density, tv.as<double>(), nullptr,
                                tf.as<int32_t>(), &V, &F, nullptr))) return rc;
        mv = &tv; mf = &tf;
    }
    if ((rc = dvn.alloc((size_t)V * 24))) return rc;
    if (V > 0 && (rc = mesh_vertex_normals_dev(mv->as<double>(), V, mf->as<int32_t>(), F, dvn.as<double>(), nullptr))) return rc;
    std::vector<double> ov((size_t)V * 3 + 1), on((size_t)V * 3 + 1);
    std::vector<int32_t> of((size_t)F * 3 + 1);
    if ((rc = down(ov.data(), *mv, (size_t)V * 3)) || (rc = down(on.data(), dvn, (size_t)V * 3)) || (rc = down(of.data(), *mf, (size_t)F * 3))) return rc;
    if ((rc = mvs_obj_write(model_obj, V, ov.data(), on.data(), F, of.data()))) return rc;
    if (V_out) *V_out = V;
    if (F_out) *F_out = F;
    return MVS_OK;
}

int mvs_processor_poisson(const char* psr_npts, const mvs_poisson_params* params, const char* model_obj, int64_t* V_out, int64_t* F_out) {
    MVS_TRACE();
    if (!psr_npts || !model_obj) return bad(__func__, "psr_npts / model_obj is NULL");
    mvs_poisson_params prm;
    if (params) prm = *params; else mvs_poisson_default_params(&prm);
    return poisson_files(__func__, psr_npts, prm, nullptr, 0.0, model_obj, V_out, F_out, nullptr);
}

int mvs_processor_poisson_density(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_density_params* dparams, double trim_ratio,
                                  const char* model_obj, int64_t* V_out, int64_t* F_out) {
    MVS_TRACE();
    if (!psr_npts || !model_obj) return bad(__func__, "psr_npts / model_obj is NULL");
    if (trim_ratio != trim_ratio) return bad(__func__, "trim_ratio is NaN");
    mvs_poisson_params prm;
    mvs_poisson_density_params dprm;
    if (params) prm = *params; else mvs_poisson_default_params(&prm);
    if (dparams) dprm = *dparams; else mvs_poisson_density_default_params(&dprm);
    return poisson_files(__func__, psr_npts, prm, &dprm, trim_ratio, model_obj, V_out, F_out, nullptr);
}

int mvs_processor_poisson_screened(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_density_params* dparams,
                                   const mvs_poisson_screen_params* sparams, double trim_ratio, const char* model_obj, int64_t* V_out, int64_t* F_out) {
    MVS_TRACE();
    if (!psr_npts || !model_obj) return bad(__func__, "psr_npts / model_obj is NULL");
    if (trim_ratio != trim_ratio) return bad(__func__, "trim_ratio is NaN");
    mvs_poisson_params prm;
    mvs_poisson_density_params dprm;
    mvs_poisson_screen_params sprm;
    if (params) prm = *params; else mvs_poisson_default_params(&prm);
    if (dparams) dprm = *dparams; else mvs_poisson_density_default_params(&dprm);
    if (sparams) sprm = *sparams; else mvs_poisson_screen_default_params(&sprm);
    return poisson_files(__func__, psr_npts, prm, &dprm, trim_ratio, model_obj, V_out, F_out, &sprm);
}

int mvs_processor_poisson_band(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_band_params* bparams, const char* model_obj,
                               int64_t* V_out, int64_t* F_out, int64_t* n_open_edges) {
    MVS_TRACE();
    if (!psr_npts || !model_obj) return bad(__func__, "psr_npts / model_obj is NULL");
    mvs_poisson_params prm;
    mvs_poisson_band_params bprm;
    if (params) prm = *params; else mvs_poisson_default_params(&prm);
    if (bparams) bprm = *bparams; else mvs_poisson_band_default_params(&bprm);
    return poisson_files(__func__, psr_npts, prm, nullptr, 0.0, model_obj, V_out, F_out, nullptr, &bprm, n_open_edges);
}

int mvs_processor_poisson_band_density(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_band_params* bparams,
                                       const mvs_poisson_density_params* dparams, double trim_ratio, const char* model_obj, int64_t* V_out, int64_t* F_out,
                                       int64_t* n_open_edges) {
    MVS_TRACE();
    if (!psr_npts || !model_obj) return bad(__func__, "psr_npts / model_obj is NULL");
    if (trim_ratio != trim_ratio) return bad(__func__, "trim_ratio is NaN");
    mvs_poisson_params prm;
    mvs_poisson_band_params bprm;
    mvs_poisson_density_params dprm;
    if (params) prm = *params; else mvs_poisson_default_params(&prm);
    if (bparams) bprm = *bparams; else mvs_poisson_band_default_params(&bprm);
    if (dparams) dprm = *dparams; else mvs_poisson_density_default_params(&dprm);
    return poisson_files(__func__, psr_npts, prm, &dprm, trim_ratio, model_obj, V_out, F_out, nullptr, &bprm, n_open_edges);
}

int mvs_processor_poisson_band_screened(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_band_params* bparams,
                                        const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams, double trim_ratio,
                                        const char* model_obj, int64_t* V_out, int64_t* F_out, int64_t* n_open_edges) {
    MVS_TRACE();
    if (!psr_npts || !model_obj) return bad(__func__, "psr_npts / model_obj is NULL");
    if (trim_ratio != trim_ratio) return bad(__func__, "trim_ratio is NaN");
    mvs_poisson_params prm;
    mvs_poisson_band_params bprm;
    mvs_poisson_density_params dprm;
    mvs_poisson_screen_params sprm;
    if (params) prm = *params; else mvs_poisson_default_params(&prm);
    if (bparams) bprm = *bparams; else mvs_poisson_band_default_params(&bprm);
    if (dparams) dprm = *dparams; else mvs_poisson_density_default_params(&dprm);
    if (sparams) sprm = *sparams; else mvs_poisson_screen_default_params(&sprm);
    return poisson_files(__func__, psr_npts, prm, &dprm, trim_ratio, model_obj, V_out, F_out, &sprm, &bprm, n_open_edges);
}

}  // extern "C"
