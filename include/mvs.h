/*
 * mvs.h — C-ABI of the MI355X-native SRT + node-driven deformation engine.
 *
 * Drop-in boundary for the three solver classes the reference's Processor
 * uses by value (there is no FFI layer upstream):
 *
 *   SRTSolver      R/Solver/SRTSolver.h:8-39      -> mvs_srt_*
 *   Camera         R/Camera/Camera.h:44-49        -> struct mvs_camera, mvs_depth_*
 *   Deformation    R/Deformation/Deformation.h:224-252 -> mvs_deform_*
 *   SRT glue       R/Processor/Processor.cpp:819-823,979-982,1021-1027,1183-1184
 *                                                 -> mvs_srt_compose / _relative / _apply
 *
 * (R/ = /root/reference/MultiViewStitch/.)  Plain pointers and sizes only; no
 * C++ / torch types.  Every entry returns an int status (MVS_OK == 0,
 * negatives enumerated below) where the reference prints to std::cerr and
 * calls exit(-1) (R/Deformation/Deformation.cpp:41-45,393-397).
 *
 * Buffer conventions (SURVEY.md §8b "Buffer layout / ownership"):
 *   - points / normals : AoS double[3] per element, 24-byte stride — the
 *     memory of std::vector<Eigen::Vector3d>::data().
 *   - faces            : int32[3*F], 0-based (R/Deformation/Deformation.h:72-78).
 *   - matches          : double[6] per match = {p.xyz, q.xyz}, the memory of
 *     std::vector<std::pair<Vector3d,Vector3d>> (R/Solver/SRTSolver.h:36).
 *   - 3x3 matrices     : ROW-major double[9], M[3*i+j] = M(i,j), i.e. the
 *     `double R[3][3]` overload (R/Solver/SRTSolver.cpp:266-268).
 *   - the caller owns every buffer; the callee copies inputs to HBM at the
 *     call and writes outputs into caller buffers.
 * Pointers named *_dev are DEVICE (HBM) pointers, everything else is host.
 *
 * Stream ordering of *_dev arguments: entries that take a `hip_stream` enqueue on it (NULL = the
 * legacy default stream) and read their inputs in stream order — produce the inputs on that stream
 * or complete them first.  The mvs_deform_* handle owns a NON-BLOCKING stream that is ordered after
 * nothing else: mvs_deform_set_target_dev waits for the whole device (hipDeviceSynchronize) before
 * it reads the target, so buffers written by any stream of the caller are complete; the per-step
 * entries (mvs_deform_assoc_*, _solve) read caller buffers in the order of the handle's stream —
 * put the handle on the stream that produces them (mvs_deform_set_stream) or synchronise first.
 *
 * The library needs a gfx950 GPU; with none present every compute entry
 * returns MVS_E_NO_DEVICE.  There is no CPU fallback.
 */
#ifndef MVS_H_
#define MVS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_ABI_VERSION 4   /* 3: tracing hook, mvs_comm_set_exchange, view-sharded RemoveGround / LocalAlignmentCore; 4: mvs_deform_group_*, mvs_align_dev, mvs_retain_connect_region_dev / mvs_remove_ground_dev / mvs_part_recog_dev, mvs_trim (additive); mvs_local_alignment_core_sharded takes the rank; still 4, additive: mvs_visibility_cull(_dev), mvs_mesh_vertex_normals(_dev), mvs_processor_stitch_points / _cull_model (mvs_io.h), mvs_render_depth_views(_dev), mvs_processor_render (mvs_io.h), mvs_match_filter_pairs(_dev), mvs_sequence_pair_srt, mvs_gen_new_views(_dev), mvs_keypoint_cull(_dev), mvs_sift_match, mvs_sift_match_lists(_dev), mvs_sift_detect(_dev), mvs_point_sample(_dev), mvs_processor_point_sample (mvs_io.h) */

enum mvs_status {
    MVS_OK            =  0,
    MVS_E_INVALID_ARG = -1,  /* null pointer, negative size, bad enum          */
    MVS_E_BAD_MESH    = -2,  /* index out of range / degenerate facet          */
    MVS_E_NONMANIFOLD = -3,  /* CGAL builder would reject: Deformation.cpp:38-45 */
    MVS_E_NO_DEVICE   = -4,  /* no HIP device                                   */
    MVS_E_HIP         = -5,  /* HIP runtime error, see mvs_last_error()         */
    MVS_E_OOM         = -6,
    MVS_E_SOLVER      = -7,  /* global solve failed (Deformation.cpp:393-397)   */
    MVS_E_STATE       = -8,  /* call order violated (e.g. no target set)        */
    MVS_E_DEGENERATE  = -9,  /* fewer than 3 matches etc.                       */
    MVS_E_IO          = -10, /* file cannot be opened / parsed (mvs_io.h)        */
    /* positive = the call did its work, with a caveat the caller should look at:   */
    MVS_W_UNCONVERGED =  1   /* at least one global ARAP solve covered by the returned statistics ended above
                                cg_tol (mvs_deform_stats.unconverged_solves / worst_rel_residual_in_batch say how
                                many and by how much); the geometry is that of the inexact solves               */
};

const char* mvs_last_error(void);     /* thread-local message of the last failure */
int  mvs_abi_version(void);
int  mvs_device_count(void);          /* 0 when no GPU; never fails               */
int  mvs_set_device(int device);      /* device used by handles created afterwards */
/* The host-pointer entries (mvs_align, mvs_srt_*, mvs_depth_*, ...) keep the device scratch they used for the next call (up to
 * MVS_SCRATCH_CACHE_MB megabytes, default 4096, 0 = keep nothing: a call on a 2 M-vertex scan makes ~40 allocations and releasing
 * them was 40 % of its time).  mvs_trim() gives the kept blocks of every device back to the runtime. */
int  mvs_trim(void);
int  mvs_device_name(char* buf, int buflen);

/* ---------------------------------------------------------------- camera -- */
/* R/Camera/Camera.h:44-49.  Only fx,fy,cx,cy of K are read by the path
 * (R/Camera/Camera.cpp:40-48).  R row-major as Camera.cpp:68-72 indexes it:
 * Xc = R*Xw + t. */
typedef struct mvs_camera {
    double  fx, fy, cx, cy;
    double  R[9];
    double  t[3];
    int32_t w, h;
} mvs_camera;

/* ------------------------------------------------------------ depth (a2) -- */
/* Depth2Model::SaveModel (R/Depth2Model/Depth2Model.cpp:7-81) followed by
 * Mesh::CalculateVertexNormals (R/PlyObj/PlyObj.cpp:139-185):
 * float32 inverse-depth raster (R/Common/Utils.h:166-176) -> compacted world
 * points (row-major pixel order), their PlyObj-style vertex normals, pixel
 * index per point (texIndex) and the <=2 triangles per 2x2 quad.
 * min_dsp/max_dsp = Depth2Model ctor args; smooth = m_fSmoothThreshold.
 * Call with out_* == NULL to get the counts only.  faces may be NULL. */
int mvs_depth_to_model(const float* inv_depth, const mvs_camera* cam,
                       double min_dsp, double max_dsp, double smooth,
                       int64_t* n_points, int64_t* n_faces,
                       double* out_points, double* out_normals,
                       int32_t* out_tex_index, int32_t* out_faces);

/* Same contract with the raster and every output in HBM (zero-copy chain
 * depth -> points -> mvs_srt_apply_dev -> mvs_deform_set_target_dev). */
int mvs_depth_to_model_dev(const float* inv_depth_dev, const mvs_camera* cam,
                           double min_dsp, double max_dsp, double smooth,
                           int64_t* n_points, int64_t* n_faces,
                           double* out_points_dev, double* out_normals_dev,
                           int32_t* out_tex_index_dev, int32_t* out_faces_dev);

/* Image3D::SolveUnProjectionD (R/Image3D/Image3D.cpp:92-106): dense w*h
 * points + valid mask, no compaction. */
int mvs_depth_unproject(const float* inv_depth, const mvs_camera* cam,
                        double min_dsp, double max_dsp,
                        double* out_points /* w*h*3 */, uint8_t* out_valid /* w*h */);

/* The match-filter cascade in front of RemoveOutliers — Processor::AlignmentSeq, R/Processor/Processor.cpp:644-735, for the
 * matches between the generated views of ONE frame of sequence k and ONE frame of sequence k+1:
 *   raw[n][6] = (view1, u1, v1, view2, u2, v2) pixel matches between generated views;
 *   tex1 / tex2 [view_count][w*h] = Image3D::texIndex (generated-view pixel -> base-view pixel index, -1 none),
 *   valid1 / valid2 [w*h] = Image3D::valid, img1 / img2 [h][w][3] = the base 8-bit images in memory order.
 * Stage 1 drops out-of-range / unmapped / invalid matches and duplicates (std::set order: lexicographic in
 * (u1,v1,u2,v2)); stage 2 keeps matches whose (2 ssd_win + 1)^2 grey windows differ by an RMS <= ssd_err (SSD(),
 * R/Common/Utils.h:221-241; windows touching the border are dropped); stage 3 is the greedy gap filter (a match
 * survives unless it is within sample_interval pixels of a kept one in either image).  out: capacity n x 4
 * (u1,v1,u2,v2); stage_counts (optional) = sizes after the three stages.
 * The entry is the 1 x 1 case of mvs_match_filter_pairs (matchpairs.hip): the stage-1 rule runs on the host over tex / valid, which
 * are not uploaded; the keys and the two images go to the GPU, which sorts, filters and packs them.  A view index outside
 * [0, view_count) gives MVS_E_INVALID_ARG, before a device is needed.  w or h above 65535 gives MVS_E_INVALID_ARG: a match is
 * handled as one 64-bit key, as in mvs_match_filter_pairs. */
typedef struct mvs_match_filter_params {
    int32_t w, h, view_count;
    int32_t ssd_win;           /* ParamParser::ssd_win          */
    double  ssd_err;           /* ParamParser::ssd_err          */
    int32_t sample_interval;   /* ParamParser::sample_interval  */
    int32_t reserved;
} mvs_match_filter_params;
int mvs_match_filter(const int32_t* raw, int64_t n, const int32_t* tex1, const uint8_t* valid1, const int32_t* tex2,
                     const uint8_t* valid2, const uint8_t* img1, const uint8_t* img2, const mvs_match_filter_params* p,
                     int32_t* out, int64_t* n_out, int64_t* stage_counts /*3 or NULL*/);

/* Model2Depth (R/Model2Depth/Model2Depth.cpp:58-156, R/Camera/Camera.cpp:6-38) without GLUT: mesh -> inverse-depth raster of
 * one camera by a z-buffer pass.  Vertex stage in float32 as the fixed-function pipeline (modelview = [R|t] with rows
 * 1,2 negated, glFrustum from the intrinsics, viewport w x h, depth range [0,1]); pixel centres at (i+.5, j+.5),
 * top-left fill rule, window-space linear depth, GL_LEQUAL against a float32 depth buffer cleared to 1; then
 * RenderDepth's conversion z_b -> 1/z_e with the clipping planes recovered from the projection matrix and the rows
 * flipped to image order.  Pixels no triangle covers are 0.  The reference uses znear = 0.01f, zfar = 2000.0f.
 * What OpenGL leaves implementation-defined (fill-rule ties, 24-bit depth, near-plane clipping: triangles with a
 * vertex at or behind the eye plane are dropped here) makes parity with a particular driver unpinned. */
int mvs_render_depth(const double* points, int64_t V, const int32_t* faces, int64_t F, const mvs_camera* cam,
                     float znear, float zfar, float* out /*w*h*/);
/* mesh and raster in HBM; hip_stream may be NULL */
int mvs_render_depth_dev(const double* points_dev, int64_t V, const int32_t* faces_dev, int64_t F, const mvs_camera* cam,
                         float znear, float zfar, float* out_dev, void* hip_stream);

/* Model2Depth::SetInput + Run (R/Model2Depth/Model2Depth.h SetInput, Model2Depth.cpp:58-190) as Processor::Render calls it
 * (R/Processor/Processor.cpp:1183-1191): every camera of every sequence, sequence by sequence and camera by camera, in one call.
 * Sequence k renders the mesh mapped into its frame, p' = 1/s_k R_k^T (p - t_k) in fp64 exactly as mvs_srt_apply(inverse = 1),
 * then narrowed to float32 as SetInput does; scales = R = t = NULL renders the points as given (the world frame).  cam_off
 * (n_seq + 1, ascending from 0) and cams as mvs_visibility_cull; at least one camera, and cams[0] belongs to sequence 0.
 * One viewport for all views: the window, glViewport and glReadPixels are cams[0]'s w0 x h0 (SetInput, Reshape), while each
 * camera keeps its own frustum (w, h, cx, cy, fx, fy; Camera.cpp:15-38), so a camera of another size is rendered with its own
 * frustum into a w0 x h0 raster.  Every other rule is mvs_render_depth's, and a view whose camera has the size w0 x h0 equals
 * mvs_render_depth of the mapped points bit for bit.  out: cam_off[n_seq] rasters of w0 x h0 floats in camera order.
 * The host form rejects a facet index outside [0, V) with MVS_E_BAD_MESH; the device form draws nothing for such a facet.
 * MVS_RENDER_CHUNK_VIEWS (environment, read at every call) bounds the views rendered per chunk (0 or unset: sized from a
 * 256 MiB budget); the results do not depend on it. */
int mvs_render_depth_views(const double* points, int64_t V, const int32_t* faces, int64_t F, int32_t n_seq,
                           const double* scales, const double* R, const double* t, const int32_t* cam_off,
                           const mvs_camera* cams, float znear, float zfar, float* out /*N*h0*w0*/);
/* mesh and rasters in HBM (the tables stay host arrays); hip_stream may be NULL; returns with the work complete */
int mvs_render_depth_views_dev(const double* points_dev, int64_t V, const int32_t* faces_dev, int64_t F, int32_t n_seq,
                               const double* scales, const double* R, const double* t, const int32_t* cam_off,
                               const mvs_camera* cams, float znear, float zfar, float* out_dev, void* hip_stream);

/* Processor::CheckConsistencyCore (R/Processor/Processor.cpp:72-126): depth-consistency filter of one frame against
 * n_ref (<= 4) reference frames, applied in the given order.  A pixel keeps its inverse depth iff it is inside
 * [min_dsp, max_dsp] and for every reference: its world point lands inside the reference image on a pixel with a valid
 * inverse depth whose world point projects back inside the current image within reproj_err INTEGER pixels
 * (`sqrt(int) > reproj_err`, ParamParser::reproj_err is an int); otherwise it becomes 0.  Rasters are the float32
 * files of LoadDepth; `out` is what SaveDepth writes to DATA/CHECK (the values are float32 throughout).  All frames
 * share one raster size (the reference indexes every raster with the current width, :93). */
int mvs_check_consistency(const float* depth, const mvs_camera* cur, int32_t n_ref, const float* const* ref_depths,
                          const mvs_camera* ref_cams, double min_dsp, double max_dsp, int32_t reproj_err,
                          float* out /*w*h*/);

/* Processor::CheckConsistency (R/Processor/Processor.cpp:29-70) for one sequence: frame i is checked against frames
 * i-1 and i+1 (in that order, those that exist), always against the ORIGINAL rasters.  depths / out: n_frames*w*h. */
int mvs_check_consistency_seq(int32_t n_frames, const float* depths, const mvs_camera* cams, double min_dsp,
                              double max_dsp, int32_t reproj_err, float* out);
/* same with both raster stacks in HBM (out_dev must not alias depths_dev); hip_stream may be NULL */
int mvs_check_consistency_seq_dev(int32_t n_frames, const float* depths_dev, const mvs_camera* cams, double min_dsp,
                                  double max_dsp, int32_t reproj_err, float* out_dev, void* hip_stream);

/* ------------------------------------------------------------ SRT (a3-a9) -- */
enum mvs_srt_mode {
    MVS_SRT_CLOSED_FORM = 0,  /* EstimateTransform(double&,Matrix3d&,Vector3d&)  SRTSolver.cpp:272-275 */
    MVS_SRT_RANSAC      = 1   /* EstimateTransformRansac / array overload        SRTSolver.cpp:256-270,277-280 */
};

/* One fit.  `triples` = iters*3 match indices replacing the reference's
 * rand()-driven Shuffle (R/Common/Utils.h:25-34); NULL
 * -> generated from `seed` with the MSVC rand() LCG + Shuffle.  Cameras are
 * read only by the RANSAC score / residual (SRTSolver.cpp:6-29).
 * residual (optional) = ResidualError(scale,R,t) of the returned transform. */
int mvs_srt_fit(const double* matches, int64_t n,
                const mvs_camera* cam1, const mvs_camera* cam2,
                int mode, const int32_t* triples, int iters, uint32_t seed,
                double* scale, double* R /*9*/, double* t /*3*/, double* residual);

/* SRTSolver::ResidualError (SRTSolver.cpp:6-29); per_match (optional, n*2)
 * receives err1,err2 per match — what Processor::RemoveOutliers thresholds
 * (R/Processor/Processor.cpp:207-246). */
int mvs_srt_residual(const double* matches, int64_t n,
                     const mvs_camera* cam1, const mvs_camera* cam2,
                     double scale, const double* R, const double* t,
                     double* mean_err, double* per_match);

/* Processor::RemoveOutliers (Processor.cpp:177-269): <=3 rounds of
 * RANSAC(iters) -> per-match pixel errors -> keep both <= pixel_err*ratio.
 * keep (n bytes) receives the surviving mask.  Each round draws its triples
 * from the MSVC rand() LCG + Shuffle (R/Common/Utils.h:25-34); rand_state is
 * the LCG state (srand seed) in, advanced state out. */
int mvs_srt_remove_outliers(const double* matches, int64_t n,
                            const mvs_camera* cam1, const mvs_camera* cam2,
                            int iters, double pixel_err, double adapt_ratio,
                            uint32_t* rand_state,
                            uint8_t* keep, int64_t* n_keep, double* err);

/* Key-frame pair selection of Processor::AlignmentSeq (R/Processor/Processor.cpp:746-765) between the n1 frames of one
 * sequence and the n2 frames of the next: RemoveOutliers runs on every frame pair (i, j) holding >= min_match_count
 * matches — in the reference's loop order (i outer, j inner), one rand() stream through all of them — and the pair with
 * the strictly smallest residual whose filtered list still holds >= min_match_count matches is selected.
 *   cams1[n1], cams2[n2]      : the frames' cameras;
 *   match_offsets[n1*n2 + 1]  : pair k = i*n2 + j owns matches [match_offsets[k], match_offsets[k+1]) (ascending from 0);
 *   matches                   : lifted 3-D matches {p.xyz, q.xyz} of all pairs, back to back;
 *   rand_state                : srand seed / LCG state in, advanced state out;
 *   frm_idx1, frm_idx2, err   : the selection (-1, -1, HUGE_VAL and MVS_E_DEGENERATE when no pair qualifies — the
 *                               reference prints "No Enough Sift Feature Matches" and exits, :794-800);
 *   keep (optional, total)    : surviving mask of EVERY pair (the reference filters all the lists in place);
 *   n_keep, pair_err (optional, n1*n2): survivors and residual per pair (HUGE_VAL for a pair that was skipped).
 * All hypotheses of a RANSAC round of all pairs run as one launch set. */
int mvs_select_keyframe_pair(int32_t n1, int32_t n2, const mvs_camera* cams1, const mvs_camera* cams2,
                             const int64_t* match_offsets, const double* matches, int32_t min_match_count, int iters,
                             double pixel_err, double adapt_ratio, uint32_t* rand_state,
                             int32_t* frm_idx1, int32_t* frm_idx2, double* err,
                             uint8_t* keep, int64_t* n_keep, double* pair_err);

/* Fill triples with the reference's generator: MSVC rand() LCG driving
 * Shuffle(idx, n, 3) (R/Common/Utils.h:25-34).  state in/out. */
int mvs_srt_make_triples(int64_t n, int iters, uint32_t* state, int32_t* triples);

/* The match-filter cascade of mvs_match_filter for ALL n1 x n2 frame pairs of two adjacent sequences in one launch set — the three
 * loops of Processor::CalcSimilarityTransformationSeq, R/Processor/Processor.cpp:645-735.  Frame i of the first sequence has its own
 * texIndex stack tex1[i][view_count][w*h], valid mask valid1[i][w*h] and base image imgs1[i][h][w][3]; frame j of the second one
 * tex2[j], valid2[j], imgs2[j]; each stack is uploaded once.  Pair k = i*n2 + j owns the raw matches
 * [raw_offsets[k], raw_offsets[k+1]) of raw[total][6] = (view1,u1,v1,view2,u2,v2); raw_offsets (n1*n2 + 1) ascends from 0.
 * out (capacity total x 4) receives the survivors (u1,v1,u2,v2) of every pair back to back, pair k at
 * [out_offsets[k], out_offsets[k+1]); stage_counts (optional, n1*n2 x 3) the sizes after the three stages.  Pair k's slice and its
 * row of stage_counts equal what mvs_match_filter returns for that pair's inputs, bit for bit.  w and h must not exceed 65535 (a
 * match is handled as one 64-bit key), n1*n2 <= 1000000; a view index outside [0, view_count) gives MVS_E_INVALID_ARG.
 * A pair's keys are sorted in LDS; a pair with more stage-1 input than fits takes the same kernel on a global-memory workspace.
 * MVS_MATCH_PAIRS_LDS_CAP (environment, read at every call) lowers that capacity; the results do not depend on it. */
int mvs_match_filter_pairs(int32_t n1, int32_t n2, const int64_t* raw_offsets /*n1*n2+1*/, const int32_t* raw /*total x 6*/,
                           const int32_t* tex1 /*n1 x views x w*h*/, const uint8_t* valid1 /*n1 x w*h*/,
                           const int32_t* tex2 /*n2 x views x w*h*/, const uint8_t* valid2 /*n2 x w*h*/,
                           const uint8_t* imgs1 /*n1 x h x w x 3*/, const uint8_t* imgs2 /*n2 x h x w x 3*/,
                           const mvs_match_filter_params* p, int32_t* out /*capacity total x 4*/, int64_t* out_offsets /*n1*n2+1*/,
                           int64_t* stage_counts /*n1*n2 x 3 or NULL*/);
/* the six stacks in HBM, read in the order of hip_stream (may be NULL); raw, raw_offsets and every output stay host arrays;
 * returns with the work complete */
int mvs_match_filter_pairs_dev(int32_t n1, int32_t n2, const int64_t* raw_offsets, const int32_t* raw, const int32_t* tex1_dev,
                               const uint8_t* valid1_dev, const int32_t* tex2_dev, const uint8_t* valid2_dev,
                               const uint8_t* imgs1_dev, const uint8_t* imgs2_dev, const mvs_match_filter_params* p, int32_t* out,
                               int64_t* out_offsets, int64_t* stage_counts, void* hip_stream);

/* One turn of the loop over adjacent sequences of Processor::CalcSimilarityTransformationSeq (R/Processor/Processor.cpp:629-826,
 * without the match JPEGs of :767-793, which mvs_match_overlays draws and mvs_processor_match_overlays (mvs_io.h) writes from the lists
 * of mvs_match_filter_pairs; SIFT matching, :634, is the caller's: its output is `raw`):
 *   the valid masks of both sequences from their float32 inverse-depth rasters (valid iff inside [min_dsp, max_dsp], Image3D.cpp:98-101),
 *   the cascade of mvs_match_filter_pairs (:645-735), every survivor lifted to {GetPoint(u1,v1) of frame i, GetPoint(u2,v2) of frame j}
 *   with the arithmetic of mvs_depth_unproject ((0,0,0) for a pixel outside [min_dsp, max_dsp]), mvs_select_keyframe_pair on the lifted
 *   lists (:746-765; rand_state in / out, MVS_E_DEGENERATE when no pair qualifies, :794-800), then the closed-form fit
 *   (MVS_SRT_CLOSED_FORM, :814-817) over the selected pair's matches that survived RemoveOutliers, in list order, with the pair's two
 *   cameras; residual = ResidualError of the result (:818).
 * cams1[n1] / cams2[n2] must have the size w x h of p->filter; depths1 [n1][w*h], depths2 [n2][w*h]; raw_offsets / raw / tex / imgs as
 * mvs_match_filter_pairs.  Optional outputs (NULL to skip): residual, stage_counts (n1*n2 x 3), n_keep and pair_err (n1*n2, as
 * mvs_select_keyframe_pair), n_sel and sel_matches (the fitted 3-D matches {p.xyz, q.xyz}; capacity: the largest raw bucket x 6). */
typedef struct mvs_seq_pair_params {
    mvs_match_filter_params filter;      /* w, h, view_count, ssd_win, ssd_err, sample_interval */
    double  min_dsp, max_dsp;            /* ParamParser::m_fMinDsp / m_fMaxDsp: validity and lift */
    int32_t min_match_count;             /* ParamParser::min_match_count */
    int32_t ransac_iters;                /* 200, Processor.cpp:202 */
    double  pixel_err, adapt_ratio;      /* RemoveOutliers */
} mvs_seq_pair_params;
int mvs_sequence_pair_srt(int32_t n1, int32_t n2, const mvs_camera* cams1, const mvs_camera* cams2,
                          const float* depths1 /*n1 x w*h*/, const float* depths2 /*n2 x w*h*/,
                          const int64_t* raw_offsets, const int32_t* raw, const int32_t* tex1, const int32_t* tex2,
                          const uint8_t* imgs1, const uint8_t* imgs2, const mvs_seq_pair_params* p, uint32_t* rand_state,
                          int32_t* frm_idx1, int32_t* frm_idx2, double* scale, double* R /*9*/, double* t /*3*/, double* residual,
                          int64_t* stage_counts, int64_t* n_keep, double* pair_err, int64_t* n_sel, double* sel_matches);

/* Image3D::GenNewViews (R/Image3D/Image3D.cpp:109-222) for all n_frames frames of one sequence in one launch set: view_count rotated
 * homography views of every base image and the texIndex table of each view (generated-view pixel -> base-view pixel, -1 = unmapped).
 * cams[n_frames] share one size w x h (<= 65535 each); imgs [n][h][w][3] uint8 as mvs_match_filter_pairs takes them; view_count >= 1,
 * axis in 0..2 and rot_angle in degrees are ParamParser::view_count / axis / rot_angle.  views [n][view_count][h][w][3] uint8;
 * tex [n][view_count][w*h] int32, exactly the tex1 / tex2 of mvs_match_filter_pairs.  The rules, literally those of :113-217:
 *   angles      : -rot*i for i = view_count/2 .. 1, then rot*i for i = 0 .. view_count/2; the first view_count entries are used (an even
 *                 view_count never uses its largest positive angle) (:131-133);
 *   homography  : axis = row `axis` of the camera's R, R_ = RotationMatrix (R/Common/Utils.h:124-138), K_ the hand-written inverse of
 *                 :123-125, H = K (R_ K_), every 3 x 3 product a0*b0 + a1*b1 + a2*b2 left to right; computed on the host in double (the
 *                 only sin / cos), so the device evaluates no transcendental function;
 *   source      : w2 = int(w*2.0) by h2 = int(h*2.0) pixels i; u = (int)(i % w2 - w2*0.25), v = (int)(i / w2 - h2*0.25), wf, uf, vf as
 *                 :153-155; CheckRange takes ints, so its double arguments are converted first (uf = -0.5 is in range);
 *   double->int : every conversion is one helper (camera_dev.h cvt_i32): a finite x with |x| < 2^31 truncates toward zero, anything else
 *                 (NaN, +-inf, out of range) gives INT_MIN, as the reference's x64 build, which CheckRange always rejects;
 *   pass A      : the bounding box of :146-167 over the source pixels whose (uf, vf) is in range, as an exact integer min / max
 *                 reduction; start values +-1e9 as the reference, so a view with no pixel in range gets the reference's offsets;
 *   pass B      : the paint of :170-216.  The reference scatters in ascending i and a later i overwrites an earlier one; the
 *                 destination (int)(i % w2 - offsetx + 0.5) truncates toward zero, so two source columns (rows) can land on destination
 *                 column (row) 0 and up to four source pixels write one destination pixel.  Here every destination pixel gathers: its
 *                 sources in descending i, the first that passes the three CheckRange tests of :178 paints it.  Same result, no race;
 *   colour      : the four branches of :179-211 (both equal, u11 == u22, v11 == v22, bilinear) with the reference's expressions and
 *                 summation order, (uchar) of the double; tex = v11*w + u11 for the both-equal branch, else int(vf+0.5)*w + int(uf+0.5).
 * Deviations: a destination pixel nothing paints is uninitialised cv::Mat memory in the reference; here it is (0,0,0), tex = -1.  The
 * reference writes the views as JPEG and SIFT reads them back: the entry returns the rasters, mvs_jpeg_roundtrip turns them into the
 * pixels that come back from the file (rules E1-E9 below, pinned against libjpeg-turbo, not against the reference's libjpeg), and
 * mvs_processor_save_views (mvs_io.h) writes the files.
 * MVS_E_INVALID_ARG: view_count < 1, axis outside 0..2, n_frames < 1, cameras of differing sizes, a NULL pointer, w or h > 65535. */
int mvs_gen_new_views(int32_t n_frames, const mvs_camera* cams, const uint8_t* imgs /*n x h x w x 3*/, int32_t view_count, int32_t axis,
                      double rot_angle, uint8_t* views /*n x views x h x w x 3*/, int32_t* tex /*n x views x w*h*/);
/* images and both outputs in HBM, in the order of hip_stream (may be NULL); returns with the work complete */
int mvs_gen_new_views_dev(int32_t n_frames, const mvs_camera* cams, const uint8_t* imgs_dev, int32_t view_count, int32_t axis,
                          double rot_angle, uint8_t* views_dev, int32_t* tex_dev, void* hip_stream);

/* The background cull of the SIFT key points (R/Processor/Processor.cpp:567-600) for every list of one sequence in one launch set.
 * List i (of n_frames*view_count) belongs to frame i / view_count and view i % view_count, the reference's order, and owns the keys
 * [key_offsets[i], key_offsets[i+1]) (ascending from 0) of keys[total][4] float32 = SiftGPU::SiftKeypoint {x, y, s, o}; descs
 * [total][128] float32 or NULL.  tex [n][view_count][w*h] as mvs_gen_new_views writes it, depths [n][w*h] the float32 inverse-depth
 * rasters, mask [n][w*h] uint8 or NULL (NULL: ParamParser::isSegment off; non-zero = inside, Image3D::InMask).  Per key:
 *   1. x = (int)key.x, y = (int)key.y, the implicit float -> int of GetTexIndex's parameters (the conversion rule above);
 *   2. idx = tex[frame][view][y*w + x]; the key is dropped when idx == -1, when depths[frame][idx] is outside [min_dsp, max_dsp]
 *      (Image3D.cpp:98-101) or when mask[frame][idx] == 0 (:576);
 *   3. p3d = the world point of pixel idx with the arithmetic of mvs_depth_unproject (:578);
 *   4. for every OTHER frame of the sequence GetImgCoordFromWorld with that frame's camera (integer rounding, no z test): outside the
 *      image -> removed (:579-589).
 * Survivors keep their order within their list; a key and its 128 floats move together.  keep (optional) [total] uint8; out_offsets
 * [n_frames*view_count + 1]; out_keys / out_descs (capacity total rows; out_descs only with descs) hold the compacted lists back to
 * back, list i at [out_offsets[i], out_offsets[i+1]).  Outputs must not alias inputs.
 * Deviation: a key outside [0,w) x [0,h) (after step 1) is dropped, and so is one whose tex entry is outside [-1, w*h); the
 * reference would read out of bounds.
 * MVS_E_INVALID_ARG: n_frames or view_count < 1, cameras of differing sizes, w or h > 65535, key_offsets not ascending from 0, a
 * required pointer NULL. */
int mvs_keypoint_cull(int32_t n_frames, int32_t view_count, const mvs_camera* cams, const int64_t* key_offsets, const float* keys,
                      const float* descs /*or NULL*/, const int32_t* tex, const float* depths, double min_dsp, double max_dsp,
                      const uint8_t* mask /*or NULL*/, uint8_t* keep /*or NULL*/, int64_t* out_offsets, float* out_keys,
                      float* out_descs /*NULL without descs*/);
/* keys, descs, tex, depths, mask, keep and both compacted outputs in HBM, in the order of hip_stream (may be NULL); key_offsets and
 * out_offsets stay host arrays; returns with the work complete */
int mvs_keypoint_cull_dev(int32_t n_frames, int32_t view_count, const mvs_camera* cams, const int64_t* key_offsets, const float* keys_dev,
                          const float* descs_dev, const int32_t* tex_dev, const float* depths_dev, double min_dsp, double max_dsp,
                          const uint8_t* mask_dev, uint8_t* keep_dev, int64_t* out_offsets, float* out_keys_dev, float* out_descs_dev,
                          void* hip_stream);

/* ------------------------------------------------- foreground masks (Image3D::LoadModel, Segment 1) -- */
/* A minimum cut on n 8-connected grids of gw x gh nodes, the cut of mvs_grabcut_masks as an entry of its own.  Node i = y * gw + x.
 *   excess [n][gh*gw] int32 : the folded terminal link of a node: above 0 capacity from the source, below 0 capacity to the sink.
 *   cap [n][8][gh*gw] int32 : cap[g][d][i] >= 0, the capacity from node i to its neighbour in direction d, direction-major.  The
 *                             directions (dx, dy), y downwards: 0 (-1, 0) left, 1 (-1, -1) up-left, 2 (0, -1) up, 3 (+1, -1) up-right,
 *                             4 (+1, 0) right, 5 (+1, +1) down-right, 6 (0, +1) down, 7 (-1, +1) down-left; d and d ^ 4 are opposite.  An
 *                             entry that points outside the grid is ignored.  cap(i -> j) and cap(j -> i) may differ.
 *   source_side [n][gh*gw] uint8 : 1 / 0.
 * Rule G1: a node is on the source side iff the sink cannot be reached from it in the residual graph of a maximum preflow.  That set is
 * the maximal minimum-cut source set and does not depend on the preflow found: let T be the nodes that reach the sink in the residual
 * graph of a maximum preflow f.  No residual arc leaves V \ T for T, so the cut (V \ T, T) is saturated, carries nothing back and holds
 * no excess in T: it is a minimum cut.  For ANY minimum cut (S', T') the value of f equals cap(S', T'), which forces f to saturate
 * it and to send nothing back; no residual arc then leaves S', S' cannot reach the sink and S' is inside V \ T.  V \ T is therefore the
 * union of all minimum-cut source sets, a property of the capacities alone: no schedule, tile size or order of atomics can change a
 * byte of source_side, and two runs give the same bytes.
 * The solver is push-relabel, phase 1 only: per node an int32 excess, an int32 height and eight residual capacities; lock-free pushes
 * and relabels (Hong and He) on 16 x 16 tiles held in LDS, with integer atomics on LDS inside a tile and on global memory across tile
 * borders; a global relabelling that is the exact backward breadth-first distance from the nodes of negative excess, computed by
 * monotone min-relaxations to a fixed point, after which a node it did not reach has height INF and is inactive.  The cut is done when a
 * converged relabelling leaves no node with excess > 0 and a finite height; source_side = (height == INF).  Heights only steer the
 * pushes: whatever they are, excess and residual capacities stay a preflow, and the answer is read off an exact relabelling.
 * Every kernel does a bounded amount of work and no workgroup waits on another.  Convergence is decided by the host, which reads one
 * small counter record per round (a round: a batch of push launches when nodes are active, then a batch of relabel launches).
 * max_rounds (>= 1) caps the rounds: reaching it gives MVS_E_SOLVER with a mvs_last_error() text, source_side is then not written.
 * rounds (optional) receives the rounds used.
 * Headroom: with |excess| <= E and every capacity <= C a node's excess stays within E + 8 C; inputs where that exceeds 2^31 - 1 give
 * MVS_E_INVALID_ARG (the device form finds it in its first launch).  MVS_E_INVALID_ARG, before a device is needed: a NULL pointer other
 * than rounds, n, gw or gh < 1, gw * gh above 2^26 or n * gw * gh above 2^31 - 1, max_rounds < 1; the host form also finds a negative
 * capacity and the headroom there.  Scratch from the stream-ordered pool: 40 bytes per node. */
int mvs_grid_mincut(int32_t n, int32_t gw, int32_t gh, const int32_t* excess, const int32_t* cap, int32_t max_rounds, uint8_t* source_side,
                    int32_t* rounds /*or NULL*/);
/* excess, cap and source_side in HBM, in the order of hip_stream (may be NULL); returns with the work complete */
int mvs_grid_mincut_dev(int32_t n, int32_t gw, int32_t gh, const int32_t* excess_dev, const int32_t* cap_dev, int32_t max_rounds,
                        uint8_t* source_side_dev, int32_t* rounds, void* hip_stream);

/* Image3D::LoadModel with Segment 1 (R/Image3D/Image3D.cpp:23-51): a foreground mask per frame by cv::grabCut on the half-size image,
 * started from the margin rectangle, 3 iterations, GC_PR_FGD kept, the mask resized back — for all frames of a sequence in one launch
 * set.  OpenCV is not part of the reference tree: the rules below are recalled from OpenCV's grabcut.cpp, are NOT VERIFIED against it and
 * are this library's definition.  imgs [n][h][w][3] uint8; mask [n][h*w] uint8, 255 / 0, what mvs_keypoint_cull reads; half_mask
 * (optional) [n][hh*hw] uint8, 1 / 0.  A colour c is its three bytes (c0, c1, c2) in memory order.
 *   1. half image : hw = w / 2, hh = h / 2; half pixel (x, y), per channel, = (a + b + c + d + 2) >> 2 over the full pixels (2x, 2y),
 *                   (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1).  An odd last row or column is unused.
 *   2. rectangle  : rowL = (int)(hh * vl), colL = (int)(hw * hl), rowR = (int)(hh * vr), colR = (int)(hw * hr) (double products,
 *                   truncated); the rectangle is [colL, hw - colR) x [rowL, hh - rowR).
 *   3. start      : inside the rectangle a pixel is probable foreground; outside it is background and stays so.
 *   4. components : each of the two models (foreground, background) has 5 components.  Per frame and model: the histogram of the luma
 *                   c0 + c1 + c2 (0..765) over the model's m pixels; t_k, k = 1..4, = the smallest luma whose cumulative count reaches
 *                   (k * m + 4) / 5 (integer division); a pixel's component = the number of t_k strictly below its luma.  (OpenCV
 *                   draws k-means++ seeds at random; this start is deterministic.)
 *   5. learn      : per (frame, model, component) the count c, the sums s_a = sum c_a and the product sums p_ab = sum c_a c_b (a <= b),
 *                   exact int64, accumulated in any order.  With m the model's pixels: mean_a = (double)s_a / c; cov_ab = (double)p_ab
 *                   / c - mean_a * mean_b; det = c00 * (c11 * c22 - c12 * c21) - c01 * (c10 * c22 - c12 * c20) + c02 * (c10 * c21 -
 *                   c11 * c20); when det <= DBL_EPSILON, 0.01 is added to c00, c11 and c22 and det is recomputed; the inverse is by
 *                   cofactors, i00 = (c11 * c22 - c12 * c21) / det, i10 = -(c10 * c22 - c12 * c20) / det, i20 = (c10 * c21 - c11 * c20) /
 *                   det, i01 = -(c01 * c22 - c02 * c21) / det, i11 = (c00 * c22 - c02 * c20) / det, i21 = -(c00 * c21 - c01 * c20) / det,
 *                   i02 = (c01 * c12 - c02 * c11) / det, i12 = -(c00 * c12 - c02 * c10) / det, i22 = (c00 * c11 - c01 * c10) / det;
 *                   weight = (double)c / m; lw = log(weight) - 0.5 * log(det).  A component with c = 0 is skipped everywhere.
 *   6. assign     : with d = c - mean (doubles) and q = d0 * (d0 * i00 + d1 * i10 + d2 * i20) + d1 * (d0 * i01 + d1 * i11 + d2 * i21) +
 *                   d2 * (d0 * i02 + d1 * i12 + d2 * i22), a_k = lw_k - 0.5 * q_k; the pixel's component is the k of largest a_k in its
 *                   own model, the lowest k on ties.
 *   7. beta       : S = the exact integer sum over all pixels and their left, up-left, up and up-right neighbours inside the image of
 *                   the squared colour difference; beta = 1 / (2 * ((double)S / (4*hw*hh - 3*hw - 3*hh + 2))); S == 0: beta = 0.
 *   8. n-links    : cap(i -> j) = llrint(1024 * g * exp(-beta * d2)), d2 the squared colour difference of i and j, g = gamma for
 *                   directions 0, 2, 4, 6 and gamma / sqrt(2) for the diagonals; symmetric, computed once per call.
 *   9. t-links    : L(model) = -(M + log(sum_k exp(a_k - M))), M = max_k a_k, over the model's non-empty components; L = 9 * gamma for a
 *                   model without one.  Inside the rectangle excess = llrint(1024 * (L(background) - L(foreground))), clamped to +-K,
 *                   K = llrint(1024 * 9 * gamma); outside excess = -K.  Only the difference of the two links enters a cut.
 *  10. cut        : rule G1 (mvs_grid_mincut) on excess and the n-links; inside the rectangle foreground := source side.
 *  11. iterations : learn (5) on the components of 4; then `iters` times: assign (6), learn (5), t-links (9), cut (10).
 *  12. full size  : mask(x, y) = 255 iff any half pixel of its footprint is foreground: columns x0, x0 + 1 with x0 = x / 2 - 1 for even x
 *                   and (x - 1) / 2 for odd x, clamped to [0, hw - 1]; rows alike.  That is where OpenCV's linear resize at exactly 2x
 *                   is non-zero, the test of Image3D::InMask.  Deviation: the interpolated grey values are not produced.
 * exp and log are the device's; everything else is integer or an IEEE double operation in the order written.
 * MVS_E_INVALID_ARG, before a device is needed: a NULL pointer other than half_mask, n < 1, w or h below 2 or w * h above 2^26 or
 * n * w * h above 2^31 - 1, a margin outside [0, 1] (a NaN included), an empty rectangle, iters < 1, gamma not finite, <= 0 or above
 * 100000 (the headroom of the cut), max_rounds < 1.  MVS_E_SOLVER: a cut reached max_rounds.  Scratch from the stream-ordered pool: 78
 * bytes per half pixel (colour, mask, component, n-links and the cut's 40) and 8248 bytes of tables per frame; the host form adds the
 * images and the masks. */
typedef struct mvs_grabcut_params {
    double  hl, hr, vl, vr;     /* margin ratios left / right / top / bottom (ParamParser), 0.1 each by default   */
    double  gamma;              /* 50                                                                             */
    int32_t iters;              /* 3                                                                              */
    int32_t max_rounds;         /* 4096: rounds of one cut                                                        */
    int64_t reserved;           /* 0                                                                              */
} mvs_grabcut_params;
void mvs_grabcut_default_params(mvs_grabcut_params* p);
int mvs_grabcut_masks(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const mvs_grabcut_params* p, uint8_t* mask,
                      uint8_t* half_mask /*or NULL*/);
/* imgs, mask and half_mask in HBM, in the order of hip_stream (may be NULL); returns with the work complete */
int mvs_grabcut_masks_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, const mvs_grabcut_params* p, uint8_t* mask_dev,
                          uint8_t* half_mask_dev, void* hip_stream);

/* FeatureProc::MatchFeature (R/FeatureProc/FeatureProc.cpp:77-130, call site R/Processor/Processor.cpp:634): SiftMatchGPU's descriptor
 * matching for ALL list pairs of two adjacent sequences in one launch set.  The input is what mvs_keypoint_cull(_dev) writes — list
 * l = frame * view_count + view owns the keys [key_offsets[l], key_offsets[l+1]) of keys[total][4] float32 {x, y, s, o} and of
 * descs[total][128] float32 — and the output is what mvs_match_filter_pairs and mvs_sequence_pair_srt read: raw_offsets (n1*n2 + 1) and
 * raw[total][6] = (view1,u1,v1,view2,u2,v2), bucketed by frame pair.
 * SiftGPU's source is not part of the reference tree.  The rules below are RECALLED from SiftMatchGPU (its GLSL matcher) and NOT
 * VERIFIED against it; they are this library's definition:
 *   1. quantise    : q = (int)(512*d + 0.5) in float32, truncating; d <= 0 or NaN gives 0.  Deviation: a value above 255 saturates to
 *                    255; SiftGPU's narrowing to unsigned char is believed to wrap.  (A unit-norm descriptor clamped at 0.2 stays
 *                    below 0.498.)
 *   2. cap         : only the first max_sift descriptors of a list take part (the reference constructs SiftMatchGPU(4096),
 *                    FeatureProc.cpp:83);
 *   3. score       : s(i,j) = sum_c q1[i][c]*q2[j][c], an exact integer (at most 128*255^2);
 *   4. one direction (list A against list B), for every descriptor i of A: best = the largest score, bestidx = the LOWEST j that
 *                    attains it; second = the largest score over j != bestidx, 0 when there is no other j; best == 0 gives no match;
 *                    in double, dist = acos(min(best/262144.0, 1)) and dist2 likewise from second; m(i) = bestidx when
 *                    dist < distmax and dist < ratiomax*dist2, else -1.  A tie for best never matches when ratiomax <= 1;
 *   5. mutual best : for ascending i, (i,j) is a match when m12(i) = j >= 0 and m21(j) = i (SiftGPU's default);
 *   6. raw row     : for list l1 of sequence 1 and l2 of sequence 2, (l1 % view_count, int(x1+0.5), int(y1+0.5), l2 % view_count,
 *                    int(x2+0.5), int(y2+0.5)); the sum in double (FeatureProc.cpp:96 adds a double constant to the float), the
 *                    conversion is the double->int rule of mvs_gen_new_views (NaN and out of range give INT_MIN);
 *   7. buckets     : bucket k = (l1 / view_count)*n_frames2 + (l2 / view_count); inside a bucket l1 ascending, then l2 ascending,
 *                    then i ascending, the reference's loop order (Processor.cpp:652-664).
 * Every score is exact, so nothing here has a tolerance but the two acos of rule 4.
 * mvs_sift_match is GetSiftMatch for ONE list pair in index form: match_buf (capacity min(n1,n2) x 2) receives (i,j), n_match their
 * number; view_count is not read.  It runs the batched kernels as their 1 x 1 case.
 * mvs_sift_match_lists: raw == NULL writes only raw_offsets and pair_counts (optional, [L1*L2], the matches of list pair l1*L2 + l2 with
 * L = n_frames*view_count), so that the caller can size raw; a raw_capacity (rows) below the total gives MVS_E_INVALID_ARG after
 * raw_offsets and pair_counts are written.
 * MVS_E_INVALID_ARG, before a device is needed: offsets that do not ascend from 0, view_count < 1, max_sift < 1, a frame count < 1, a
 * required pointer NULL, n_frames1*n_frames2 > 1000000. */
typedef struct mvs_sift_match_params {
    int32_t view_count;        /* ParamParser::view_count                                  */
    int32_t max_sift;          /* 4096, FeatureProc.cpp:83                                 */
    double  distmax, ratiomax; /* ParamParser::distmax / ratiomax                          */
} mvs_sift_match_params;
int mvs_sift_match(int64_t n1, const float* descs1 /*n1 x 128*/, int64_t n2, const float* descs2 /*n2 x 128*/,
                   const mvs_sift_match_params* p, int32_t* match_buf /*capacity min(n1,n2) x 2*/, int64_t* n_match);
int mvs_sift_match_lists(int32_t n_frames1, int32_t n_frames2, const mvs_sift_match_params* p, const int64_t* key_offsets1 /*L1+1*/,
                         const float* keys1, const float* descs1, const int64_t* key_offsets2 /*L2+1*/, const float* keys2,
                         const float* descs2, int64_t* raw_offsets /*n1*n2+1*/, int32_t* raw /*raw_capacity x 6, or NULL*/,
                         int64_t raw_capacity, int64_t* pair_counts /*L1*L2 or NULL*/);
/* keys and descriptors in HBM (16-byte aligned), exactly the out_keys_dev / out_descs_dev of mvs_keypoint_cull_dev, read in the order of
 * hip_stream (may be NULL); the offsets and every output stay host arrays; returns with the work complete */
int mvs_sift_match_lists_dev(int32_t n_frames1, int32_t n_frames2, const mvs_sift_match_params* p, const int64_t* key_offsets1,
                             const float* keys1_dev, const float* descs1_dev, const int64_t* key_offsets2, const float* keys2_dev,
                             const float* descs2_dev, int64_t* raw_offsets, int32_t* raw, int64_t raw_capacity, int64_t* pair_counts,
                             void* hip_stream);

/* FeatureProc::DetectFeature (R/FeatureProc/FeatureProc.cpp:14-75,103-112, call site R/Processor/Processor.cpp:562): SIFT keys and
 * descriptors of ALL lists of a call in one launch set.  List l = frame * view_count + view is raster l of imgs (n_lists x h x w x 3
 * bytes, exactly the `views` of mvs_gen_new_views), the order mvs_keypoint_cull expects; the outputs are its inputs: key_offsets
 * (n_lists + 1, ascending from 0), keys[total][4] float32 {x, y, s, o} and descs[total][128] float32.
 * SiftGPU's source is not part of the reference tree.  The rules below are RECALLED from SiftGPU and Lowe's method and NOT VERIFIED
 * against SiftGPU; they are this library's definition.  Rules 1-6 use float32 + - * / only, each in the stated order (the library is
 * built with -ffp-contract=off); the transcendentals they need (the taps) are evaluated on the host in double.
 *   1. grey      : a pixel in the margin (x < int(w*hl), x >= w - int(w*hr), y < int(h*vl), y >= h - int(h*vr); the double -> int
 *                  rule of mvs_gen_new_views; FeatureProc.cpp:28-43) is black; I = (float)g / 255.0f with g = the 8-bit grey of
 *                  mvs_match_filter (4899, 9617, 1868 on the channels in memory order, + 8192, >> 14).
 *   2. base      : first_octave 0: U = I (W0 = w, H0 = h).  first_octave -1: U is 2w x 2h; U[2y][2x] = I[y][x]; an odd column of an
 *                  even row is 0.5f * (a + b), a its left neighbour and b the sample right of that, clamped to the last one; an odd
 *                  row is 0.5f * (a + b) of the even rows above and below (the one below clamped to the last even row).
 *   3. Gaussian  : for sigma (double): r = (int)ceil(4 sigma); taps k[i] = exp(-i^2 / (2 sigma^2)), i = -r..r, in double, divided by
 *                  their sum taken over ascending i, rounded to float32.  Rows first, then the columns of the row result; a pass is
 *                  acc = k[-r] * p[-r], then acc = acc + k[i] * p[i] for ascending i; samples outside replicate the border.
 *   4. pyramid   : n_oct = max(1, floor(log2(min(W0, H0))) - 3) octaves; octave o is W0 >> o by H0 >> o.  S + 3 Gaussian levels each
 *                  (S = dog_levels), sigma_l = sigma0 * 2^(l/S) in double.  Level 0 of the first octave is U blurred by
 *                  sqrt(sigma0^2 - (sigma_in * 2^-first_octave)^2); level l is level l - 1 blurred by sqrt(sigma_l^2 - sigma_(l-1)^2);
 *                  level 0 of the next octave is level S at the even pixels (x, y) <- (2x, 2y).
 *   5. extremum  : d[l] = g[l+1] - g[l], never stored.  For levels l = 1..S and pixels 1 <= xi <= W - 2, 1 <= yi <= H - 2: v = d[l][yi][xi]
 *                  is a candidate when |v| > T, T = dog_threshold / (float)S, and v is strictly above or strictly below all 26
 *                  neighbours in d[l-1..l+1].  A tie gives no key.
 *   6. refinement: on the 27 values D[s][y][x] around the candidate, central differences: g = 0.5f * (D+ - D-); dxx = (D+ + D-) - 2v;
 *                  dxy = 0.25f * ((D++ - D-+) - (D+- - D--)) (likewise xs, ys).  Kept when det2 = dxx*dyy - dxy*dxy > 0 and
 *                  (tr*tr)*e < ((e+1)*(e+1))*det2 with tr = dxx + dyy, e = edge_threshold.  ONE solve of H delta = -g by Cramer's rule
 *                  (the order of operations is that of sift_refine, csrc/sift_rules.h, the one body host and device share); dropped
 *                  when the determinant is 0 or any |delta| >= 1, and when |v + 0.5f * ((gx*dx + gy*dy) + gs*ds)| <= T.
 *                  x = ((xi + dx) + 0.5f) * step, y likewise, step = 2^octave (0.5 for the doubled octave): the top-left pixel centre
 *                  is (0.5, 0.5), SiftGPU's default.  sigma_oct = sigma0 * exp2f((l + ds) / S), s = sigma_oct * step.  Then the filter
 *                  of FeatureProc.cpp:53-57 drops x < left || x > right || y < top || y > bottom (left = int(w*hl), right =
 *                  w - int(w*hr), ...).
 *   7. orientation: on g[l] of the key's octave, the pixels (xi + dx, yi + dy), |dx|, |dy| <= R = (int)(3 * sw + 0.5f), sw = 1.5f *
 *                  sigma_oct, that have all four neighbours.  gx = g[x+1] - g[x-1], gy likewise; vote = exp(-((dx - delta_x)^2 +
 *                  (dy - delta_y)^2) / (2 sw^2)) * sqrt(gx^2 + gy^2); fb = atan2(gy, gx) (in [0, 2pi)) * 36 / 2pi - 0.5; the vote is
 *                  split linearly between bins floor(fb) and floor(fb) + 1 (mod 36).  EVERY vote of rules 7 and 8 is quantised to
 *                  (uint64)(vote * 2^24 + 0.5f) and the bins are integer sums: a histogram does not depend on the order of the
 *                  votes.  h = (float)sum / 2^24, then 6 passes of h[b] = ((h[b-1] + h[b]) + h[b+1]) / 3.0f (circular).  A peak is a
 *                  bin strictly above both neighbours and >= 0.8f * max; its angle is ((b + 0.5f * (hm - hp) / ((hm - 2 h) + hp)) +
 *                  0.5f) * (2pi / 36), wrapped into [0, 2pi).  The max_orient largest peaks are kept (equal peaks: the lower bin
 *                  first); a candidate without a peak gives no key.
 *   8. descriptor: 4 x 4 cells of 8 bins on g[l]; cell width m = 3 * sigma_oct.  For the pixels with |dx|, |dy| <= (int)(m * 3.5355339f)
 *                  + 2 that have all four neighbours: (nx, ny) = the offset from the key rotated by -o and divided by m; fx = nx +
 *                  1.5, fy = ny + 1.5 (samples outside (-1, 4) are skipped); gradient g = 0.5f * central difference; vote = |g| *
 *                  exp(-(nx^2 + ny^2) / 8) (a Gaussian of 2 cells); ft = ((atan2(gy, gx) - o) mod 2pi) * 8 / 2pi; the vote is split
 *                  trilinearly between the cells floor(fx), floor(fx) + 1 (those in 0..3), likewise y, and the bins floor(ft),
 *                  floor(ft) + 1 (mod 8); entry ((cell_y * 4 + cell_x) * 8 + bin).  d = (float)sum / 2^24; d /= (float)sqrt(sum of d^2
 *                  in double over ascending index) when that is positive; d = min(d, 0.2f); normalised once more the same way.
 *   9. order     : within a list octave ascending, level ascending, yi ascending, xi ascending, then a candidate's orientations by
 *                  descending peak, then ascending bin.  The first max_features keys of a list are kept.  No list depends on another.
 * A total above `capacity` (rows) gives MVS_E_INVALID_ARG after key_offsets is written, so that the caller can size the outputs.
 * Scratch comes from the stream-ordered pool; lists are processed in chunks so that the pyramids, base images and candidate flags of a
 * chunk, with the per-workgroup counts and places of its compaction (8 bytes per 256 items), stay below max(512 MiB, what ONE list
 * needs: 4 * (W0*H0 + sum over octaves of (S+3)*W*H) + (1 + 8/256) * S * sum of W*H bytes, rounded up), whatever n_lists is.  On top
 * come the tap table (at most 4 * (S+3) * 103 bytes), 4 bytes per list of a chunk, and the candidate tables (64 bytes per candidate
 * and 8 bytes per key of a chunk).
 * MVS_E_INVALID_ARG, before a device is needed: a NULL pointer, n_lists < 1, w or h below 8 or above 65535, first_octave outside
 * {-1, 0}, dog_levels outside 1..5, max_orient outside 1..4, max_features < 1, a margin ratio outside [0, 1), hl + hr >= 1, vl + vr
 * >= 1, a float parameter that is not finite, dog_threshold < 0, edge_threshold <= 0, sigma0 <= 0, sigma_in < 0, sigma0 not above
 * sigma_in * 2^-first_octave, a blur radius above 51 (sigma0 too large for dog_levels), capacity < 0, an image whose pyramid has
 * 2^31 - 1 or more (octave, level, pixel) items, S * sum over octaves of W*H ("image too large": w = h = 65535 doubled is one), and
 * for mvs_sift_detect_dev a keys_dev or descs_dev that is not 16-byte aligned. */
typedef struct mvs_sift_params {
    int32_t first_octave;    /* -1: FeatureProc.cpp:20 "-fo -1"; 0 also accepted            */
    int32_t dog_levels;      /* S = 3                                                        */
    int32_t max_orient;      /* 2 orientations per extremum at most                          */
    int32_t max_features;    /* per list, the first ones in output order; >= 1               */
    float   dog_threshold;   /* 0.02 (compared as dog_threshold / S)                         */
    float   edge_threshold;  /* 10                                                           */
    float   sigma0, sigma_in;/* 1.6, 0.5                                                     */
    double  hl, hr, vl, vr;  /* ParamParser::*_margin_ratio; 0 = no margin                   */
} mvs_sift_params;
/* the values in the comments above, max_features = INT32_MAX, no margins */
void mvs_sift_default_params(mvs_sift_params* p);
int mvs_sift_detect(int32_t n_lists, int32_t w, int32_t h, const uint8_t* imgs /*n_lists x h x w x 3*/, const mvs_sift_params* p,
                    int64_t* key_offsets /*n_lists+1*/, float* keys /*capacity x 4*/, float* descs /*capacity x 128*/, int64_t capacity);
/* images, keys and descriptors in HBM (keys and descs 16-byte aligned), in the order of hip_stream (may be NULL); key_offsets stays a
 * host array; returns with the work complete */
int mvs_sift_detect_dev(int32_t n_lists, int32_t w, int32_t h, const uint8_t* imgs_dev, const mvs_sift_params* p, int64_t* key_offsets,
                        float* keys_dev, float* descs_dev, int64_t capacity, void* hip_stream);

/* ------------------------------------------------- point sampling (GeometryRec::RunPointSample) -- */
/* The step between Processor::CheckConsistency and the stitch tail (R/Processor/Processor.cpp:933-949): the checked inverse-depth
 * rasters of every sequence to the oriented points `x y z nx ny nz` of Rec/<name>.npts that mvs_processor_stitch_points reads.  GeoRec is a
 * closed binary; its source is not part of the reference tree.  The rules below are not verified against GeoRec; they are this
 * library's definition, chosen to give a meaning to every parameter GeometryRec::Init receives from config.txt (PtSampRds, NbrFrmNum,
 * NbrFrmStep, MaxDspErr, MinConf, EdgeSzThres, MinDsp, MaxDsp).  startFrmIdx / endFrmIdx are 0 / size - 1 at the call site and are
 * not parameters; maxPsDep / minPsDep belong to Poisson.
 * Input: n_seq sequences; sequence k owns cams[cam_off[k] .. cam_off[k+1]) (cam_off as mvs_visibility_cull).  The frames of one
 * sequence share one raster size; sequences may differ.  depths holds the float32 inverse-depth rasters of all cameras back to back in
 * camera order.  All arithmetic is fp64 + - * / sqrt in the stated order (the library is built with -ffp-contract=off); every
 * double -> int conversion is the rule of mvs_gen_new_views (truncation toward zero, INT_MIN when not representable); the camera maps
 * are Camera's (R/Camera/Camera.cpp:40-72) in their operation order: world_from_img(c, u, v, z) = R^T ((u - cx) z / fx - t0,
 * (v - cy) z / fy - t1, z - t2), img_from_world(c, P): Xc = R P + t (row sums left to right, then + t), u' = int(fx Xc.x / Xc.z + cx +
 * 0.5), v' likewise.  A length is sqrt((x*x + y*y) + z*z), a dot product (x*x' + y*y') + z*z'.
 * For frame f of a sequence of n frames, r = pt_samp_rds:
 *   1. valid      : a pixel is valid when d = (double)raster[v][u] lies in [dsp_min, dsp_max]; its point is P = world_from_img(cam_f, u,
 *                   v, 1.0 / d).
 *   2. neighbours : pixel (u, v) needs 1 <= u <= w - 2, 1 <= v <= h - 2 and four valid axial neighbours: Pl, Pr at u -+ 1, Pu, Pd at
 *                   v -+ 1.
 *   3. edge, normal: z0 = 1.0 / d.  Dropped when |Pl - P| or |Pr - P| exceeds edge_sz_thres * (z0 / fabs(fx)), or |Pu - P| or |Pd - P|
 *                   exceeds edge_sz_thres * (z0 / fabs(fy)).  a = Pr - Pl, b = Pd - Pu, nrm = a x b = (a.y*b.z - a.z*b.y, a.z*b.x -
 *                   a.x*b.z, a.x*b.y - a.y*b.x), len its length; dropped unless len > 0; nrm is divided by len component by
 *                   component.  With C = world_from_img(cam_f, 0, 0, 0.0), the camera centre, nrm is negated when nrm . (P - C) > 0.
 *   4. agreement  : P agrees with frame g when Xc = R_g P + t_g has Xc.z > 0, (u', v') = img_from_world's result is inside the raster,
 *                   dg = (double)raster_g[v'][u'] is valid by rule 1 and fabs(dg - 1.0 / Xc.z) <= max_dsp_err.
 *   5. confidence : N(f) = { f + j * nbr_frm_step : j = +-1 .. +-nbr_frm_num } within [0, n); count = |N(f)|, agree = the g of N(f)
 *                   that agree with P; the pixel passes when count == 0 or (double)agree >= min_conf * (double)count.
 *   6. cells      : the raster is cut into r x r cells (partial cells at the right and bottom); the cell of (u, v) is (u / r, v / r).
 *                   A cell's candidate is its pixel of lowest row-major index that passes rules 1, 2, 3 and 5; a cell without one
 *                   has no candidate.
 *   7. coverage   : frames are taken in ascending f.  A cell of frame f emits its candidate unless the cell is covered.  Every emitted
 *                   point P then covers, in every later frame g > f of the sequence that agrees with P (rule 4), the cell (u' / r,
 *                   v' / r).  Nothing covers a cell of an earlier frame; a sequence does not see another sequence.
 *   8. order      : sequence-major, then frame ascending, then pixel index ascending.  Per emitted point: points[3], normals[3]
 *                   (doubles, the layout of mvs_npts_write), frame (its frame within the sequence) and pixel (v * w + u), int32 each,
 *                   both optional.  seq_offsets[n_seq + 1] (int64, host) brackets each sequence.
 * A sequence without a camera emits nothing.  A total above `capacity` (rows) gives MVS_E_INVALID_ARG after seq_offsets is written, so
 * that the caller can size the outputs.  The work is one launch for the candidates of all frames of all sequences, one launch per frame
 * step of the longest sequence for rule 7, and an ordered compaction without atomics: two runs give the same bytes.
 * Scratch comes from the stream-ordered pool: 5 bytes per cell of the call (the int32 candidate and the coverage byte; sum over the
 * cameras of ceil(w / r) * ceil(h / r)), 8 bytes per 256 items of the compaction (h * ceil(w / r) items per camera, every camera rounded
 * up to the largest), 140 bytes per camera and 52 bytes per sequence; the host form adds the rasters and the emitted rows.
 * MVS_E_INVALID_ARG, before a device is needed: a NULL pointer other than frame / pixel, n_seq < 1, cam_off not ascending from 0, a
 * camera with w or h <= 0 or fx or fy == 0, two raster sizes inside one sequence, w * h of a frame above 2^31 - 1, a parameter that is
 * not finite, dsp_min <= 0 or dsp_min > dsp_max, max_dsp_err < 0, min_conf outside [0, 1], edge_sz_thres <= 0, pt_samp_rds < 1,
 * nbr_frm_num < 0, nbr_frm_step < 1, capacity < 0, and a call of 2^31 or more cells (or too many workgroups for one launch). */
typedef struct mvs_point_sample_params {
    double  dsp_min, dsp_max;   /* MinDsp 0.0025, MaxDsp 0.3                                     */
    double  max_dsp_err;        /* MaxDspErr 0.01                                                */
    double  min_conf;           /* MinConf 0.9                                                   */
    double  edge_sz_thres;      /* EdgeSzThres 4.0, in pixels of the frame                       */
    int32_t pt_samp_rds;        /* PtSampRds 2: the side of a cell                               */
    int32_t nbr_frm_num;        /* NbrFrmNum 2: neighbour frames on each side                    */
    int32_t nbr_frm_step;       /* NbrFrmStep 1                                                  */
    int32_t reserved;           /* 0                                                             */
} mvs_point_sample_params;
/* the config.txt values in the comments above */
void mvs_point_sample_default_params(mvs_point_sample_params* p);
int mvs_point_sample(int32_t n_seq, const int32_t* cam_off /*n_seq+1*/, const mvs_camera* cams, const float* depths,
                     const mvs_point_sample_params* p, int64_t* seq_offsets /*n_seq+1*/, double* points /*capacity x 3*/,
                     double* normals /*capacity x 3*/, int32_t* frame /*capacity, or NULL*/, int32_t* pixel /*capacity, or NULL*/,
                     int64_t capacity);
/* rasters and outputs in HBM, in the order of hip_stream (may be NULL); cam_off, cams and seq_offsets stay host arrays; returns with
 * the work complete */
int mvs_point_sample_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths_dev,
                         const mvs_point_sample_params* p, int64_t* seq_offsets, double* points_dev, double* normals_dev,
                         int32_t* frame_dev, int32_t* pixel_dev, int64_t capacity, void* hip_stream);

/* ------------------------------------------------- depth refinement (DepthRecovery/DepthOptimizer) -- */
/* The stage behind Processor::Render in the reference's data flow: the rendered inverse-depth rasters DATA/Render/_depth<i>.raw of every
 * sequence, taken back to the images, become DATA/Refine/_depth<i>.raw (DepthOptimizer::RefineAllDepthMaps, DepthOptimizer.cpp:20-43).
 * The reference defines the files and the frame window (RefineDepthMap, :45-63: refFrmCount = 5 frames around the current one, without
 * it) and stops there: DepthRefineCore is declared and never defined.  The rules below are this library's definition, NOT VERIFIED
 * against any ZJU code: a plane sweep of 2 * steps + 1 disparity hypotheses around the rendered value, scored by the 8-bit grey SSD of
 * the match filter (R/Common/Utils.h:221-241) against the reference frames.
 * Input: n_seq sequences; sequence k owns cams[cam_off[k] .. cam_off[k+1]) (cam_off and cams as mvs_point_sample: the frames of one
 * sequence share one raster size; sequences may differ).  imgs holds the RGB base images of all cameras back to back in camera order,
 * each h x w x 3 bytes in the byte order the grey conversion of mvs_match_filter assumes; depths and out are float32 inverse-depth
 * rasters in camera order; out must not alias depths.  All floating-point arithmetic is fp64 + - * / sqrt in the order written (the
 * library is built with -ffp-contract=off); the camera maps and the double -> int rule are those of mvs_point_sample.
 * For frame f of a sequence of n frames, with N = ssd_win, len = 2 N + 1, K = steps:
 *   1. grey       : G_f[v][u] = (4899 * p0 + 9617 * p1 + 1868 * p2 + 8192) >> 14 of the pixel's three bytes in memory order, the
 *                   integer conversion of mvs_match_filter.
 *   2. references : g = f - ref_frm_count / 2 + i for i = 0 .. ref_frm_count - 1, kept when 0 <= g < n and g != f, in ascending order.
 *   3. candidates : pixel (u, v) is a candidate when d0 = (double)depths_f[v][u] lies in [dsp_min, dsp_max] (a NaN does not) and
 *                   N <= u < w - N, N <= v < h - N.  Any other pixel copies its input float bit for bit to out and reports k = -128,
 *                   sum = -1, cnt = 0.
 *   4. hypotheses : step = rel_range / (double)K and d_k = d0 * (1.0 + (double)k * step) for k = -K .. K, so d_0 == d0 exactly.  A
 *                   hypothesis is live when d_k lies in [dsp_min, dsp_max].
 *   5. cost       : for a live k and a reference g: P = world_from_img(cam_f, u, v, 1.0 / d_k), Xc = R_g P + t_g.  The reference
 *                   counts when Xc.z > 0 and (u', v') = (int(fx Xc.x / Xc.z + cx + 0.5), v' likewise) has N <= u' < w - N,
 *                   N <= v' < h - N.  It then contributes ssd_g = the sum over a, b in [-N, N] of (G_f[v+a][u+b] - G_g[v'+a][u'+b])^2,
 *                   an exact integer.  sum_k is the sum of the ssd_g that count, cnt_k how many did.
 *   6. choice     : only k with cnt_k > 0 are eligible.  k beats j when sum_k * cnt_j < sum_j * cnt_k in int64; on equality the smaller
 *                   |k| wins, then k < 0.  Without an eligible k the pixel is treated as in rule 3.
 *   7. acceptance : with m = (double)sum / (double)cnt of the winner k*, the pixel is accepted when sqrt(m / (double)(len * len)) <=
 *                   ssd_err.  Accepted: k_out = k* and out = (float)d, d = d_k* when MVS_REFINE_SUBSTEP is off.  Not accepted: out is
 *                   the input float bit for bit and k_out = -128; sum_out and cnt_out still report the winner.
 *   8. substep    : (MVS_REFINE_SUBSTEP) when k* - 1 and k* + 1 both lie in [-K, K] and are eligible, c-, c0, c+ are their m values
 *                   and den = (c- - 2.0 * c0) + c+.  If den > 0: o = 0.5 * ((c- - c+) / den) and d = d0 * (1.0 + ((double)k* + o) *
 *                   step).  If that d is not in [dsp_min, dsp_max], or den <= 0, d = d_k*.
 *   9. inputs     : every frame reads the original rasters and images; a sequence does not see another sequence.
 * It follows that a sequence of one frame, or ref_frm_count = 1, returns its input bytes; that on images of one colour every sum is 0,
 * so that k* is the eligible k of smallest |k| and a pixel returns its input bytes wherever k = 0 is eligible (it is not where d_0
 * lands outside the interior of every reference while another d_k lands inside one); and that NaN, +-inf, negative values, -0.0 and
 * zeros pass through unchanged.
 * The result is defined by integers and by fp64 operations in a stated order: no schedule can change a byte, and two runs give the same
 * bytes.  The work is three launches without atomics: the grey rasters of all images, the sum of squares over the window of every
 * pixel, and the refinement of all frames of all sequences (rule 5's sum as sum a^2 + sum b^2 - 2 sum a b, exact in uint32).
 * k_out (int8), sum_out (int32) and cnt_out (uint8), one entry per pixel in raster order, are optional.  With the ranges below a sum is
 * at most 961 * 255^2 * 8 < 2^31.  Scratch comes from the stream-ordered pool: 5 bytes per pixel of the call (the grey byte and the
 * uint32 sum of squares), 140 bytes per camera and 32 bytes per sequence; the host form adds the images, the rasters and the outputs.
 * MVS_E_INVALID_ARG, before a device is needed: a NULL pointer other than the optional outputs, n_seq < 1, cam_off not ascending from
 * 0, a camera with w or h <= 0 or fx or fy == 0, two raster sizes inside one sequence, w * h of a frame above 2^31 - 1, a parameter
 * that is not finite, dsp_min <= 0 or dsp_min > dsp_max, rel_range <= 0 or >= 1, ssd_err < 0, ssd_win outside [0, 15], ref_frm_count
 * outside [1, 9] or even, steps outside [1, 63], unknown flag bits, out == depths, and too many workgroups for one launch. */
#define MVS_REFINE_SUBSTEP 1
typedef struct mvs_depth_refine_params {   /* 48 bytes */
    double  dsp_min, dsp_max;   /* MinDsp 0.0025, MaxDsp 0.3                                     */
    double  rel_range;          /* 0.04: half-width of the search, relative to the rendered disparity */
    double  ssd_err;            /* SSDError 40.0                                                 */
    int32_t ssd_win;            /* SSDWin 7: N, the window is (2N+1)^2; 0..15                    */
    int32_t ref_frm_count;      /* refFrmCount 5 (DepthOptimizer.cpp:45); odd, 1..9              */
    int32_t steps;              /* 8: K hypotheses on each side; 1..63                           */
    int32_t flags;              /* MVS_REFINE_SUBSTEP = 1                                        */
} mvs_depth_refine_params;
/* the values in the comments above; flags = MVS_REFINE_SUBSTEP */
void mvs_depth_refine_default_params(mvs_depth_refine_params* p);
int mvs_refine_depth_maps(int32_t n_seq, const int32_t* cam_off /*n_seq+1*/, const mvs_camera* cams, const uint8_t* imgs,
                          const float* depths, const mvs_depth_refine_params* p, float* out, int8_t* k_out /*or NULL*/,
                          int32_t* sum_out /*or NULL*/, uint8_t* cnt_out /*or NULL*/);
/* images, rasters and outputs in HBM, in the order of hip_stream (may be NULL); cam_off and cams stay host arrays; returns with the
 * work complete */
int mvs_refine_depth_maps_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev,
                              const float* depths_dev, const mvs_depth_refine_params* p, float* out_dev, int8_t* k_out_dev,
                              int32_t* sum_out_dev, uint8_t* cnt_out_dev, void* hip_stream);

/* ------------------------------------------------- depth recovery (DATA/_depth<i>.raw from the images) -- */
/* The one input of the reference's `-a 1` run that no program of the reference writes: the first inverse-depth rasters
 * DATA/_depth<i>.raw of every sequence, which Processor::CheckConsistency reads (Processor.cpp:37-38).  mvs_refine_depth_maps searches
 * a few per cent around an existing value and cannot start a sequence; this call has no input raster: a plane sweep over `levels`
 * disparities of [dsp_min, dsp_max], scored as the refinement scores its hypotheses.  The rules R1-R9 below are this library's
 * definition, NOT VERIFIED against any ZJU code.  levels, peak and min_refs are choices: nobody has measured them on a real sequence.
 * Input: n_seq, cam_off, cams and imgs as mvs_refine_depth_maps (the frames of one sequence share one raster size; sequences may
 * differ; imgs holds the RGB base images of all cameras back to back in camera order).  out: float32 inverse-depth rasters in camera
 * order.  All floating-point arithmetic is fp64 + - * / sqrt in the order written (the library is built with -ffp-contract=off); the
 * camera maps and the double -> int rule are those of mvs_point_sample.  Every cost is an exact integer.
 * For frame f of a sequence of n frames, with N = ssd_win, len = 2 N + 1, L = levels:
 *   R1 grey       : G_f[v][u] = (4899 * p0 + 9617 * p1 + 1868 * p2 + 8192) >> 14 of the pixel's three bytes in memory order, the
 *                   integer conversion of mvs_match_filter.
 *   R2 references : g = f - ref_frm_count / 2 + i for i = 0 .. ref_frm_count - 1, kept when 0 <= g < n and g != f, in ascending order.
 *   R3 candidates : every pixel with N <= u < w - N and N <= v < h - N is a candidate.  Any other pixel gets out = +0.0f, level = -1,
 *                   sum = -1, cnt = 0.
 *   R4 levels     : step = (dsp_max - dsp_min) / (double)(L - 1); d_l = dsp_min + (double)l * step for l < L - 1 and d_{L-1} = dsp_max
 *                   exactly.  The levels are uniform in disparity, so a reference pixel moves by equal amounts per level.
 *   R5 cost       : for a level l and a reference g: P = world_from_img(cam_f, u, v, 1.0 / d_l), Xc = R_g P + t_g.  The reference
 *                   counts when Xc.z > 0 and (u', v') = (int(fx Xc.x / Xc.z + cx + 0.5), v' likewise) has N <= u' < w - N,
 *                   N <= v' < h - N.  It then contributes ssd_g = the sum over a, b in [-N, N] of (G_f[v+a][u+b] - G_g[v'+a][u'+b])^2,
 *                   an exact integer.  sum_l is the sum of the ssd_g that count, cnt_l how many did.
 *   R6 choice     : level l is eligible when cnt_l >= min_refs.  l beats j when sum_l * cnt_j < sum_j * cnt_l in int64; on equality
 *                   the lower l wins.  The worst eligible level W is found by the same comparison reversed; on equality the lower l
 *                   is W.  A pixel without an eligible level is treated as in R3.
 *   R7 acceptance : with m = (double)sum / (double)cnt of the winner l* and m_W of W, the pixel is accepted when both
 *                   sqrt(m / (double)(len * len)) <= ssd_err and m < peak * m_W hold.  A flat cost curve says nothing: an image of
 *                   one colour rejects every pixel, and so does a pixel with one eligible level.  A rejected pixel gets out = +0.0f
 *                   and level = -1; its sum and cnt still report the winner.
 *   R8 substep    : (MVS_RECOVER_SUBSTEP) when l* - 1 and l* + 1 both lie in [0, L - 1] and are eligible, c-, c0, c+ are their m
 *                   values and den = (c- - 2.0 * c0) + c+.  If den > 0: o = 0.5 * ((c- - c+) / den) and d = dsp_min + ((double)l* + o)
 *                   * step.  If that d is not in [dsp_min, dsp_max], or den <= 0, or the substep does not apply, d = d_l*.
 *   R9 value      : out = (float)d.  If (double)out < dsp_min, out becomes the next float32 above; if (double)out > dsp_max, the next
 *                   float32 below.  Every accepted pixel is therefore a valid value for mvs_check_consistency, the model loader and
 *                   mvs_point_sample under the same range.
 * Every frame reads only images; a sequence does not see another sequence.  It follows that a sequence of one frame, or
 * ref_frm_count = 1, or min_refs above the references a frame has, rejects every pixel.
 * The result is defined by integers and by fp64 operations in a stated order: no schedule can change a byte, and two runs give the same
 * bytes.  The work is three launches without atomics: the grey rasters of all images, the sum of squares over the window of every
 * pixel (both shared with the refinement), and the sweep of all frames of all sequences, a thread per pixel walking every level.
 * level_out (int16), sum_out (int32) and cnt_out (uint8), one entry per pixel in raster order, are optional.  Scratch comes from the
 * stream-ordered pool as for the refinement: 5 bytes per pixel, 140 bytes per camera and 32 bytes per sequence; the host form adds the
 * images and the outputs.
 * MVS_E_INVALID_ARG, before a device is needed: a NULL pointer other than the optional outputs, n_seq < 1, cam_off not ascending from
 * 0, a camera with w or h <= 0 or fx or fy == 0, two raster sizes inside one sequence, w * h of a frame above 2^31 - 1, a parameter
 * that is not finite, dsp_min <= 0 or dsp_min >= dsp_max, ssd_err < 0, peak outside (0, 1], ssd_win outside [0, 15], ref_frm_count
 * outside [1, 9] or even, levels outside [2, 1024], min_refs outside [1, 8], unknown flag bits, reserved != 0, and too many workgroups
 * for one launch. */
#define MVS_RECOVER_SUBSTEP 1
typedef struct mvs_depth_recover_params {  /* 56 bytes */
    double  dsp_min, dsp_max;   /* MinDsp 0.0025, MaxDsp 0.3                                     */
    double  ssd_err;            /* SSDError 40.0                                                 */
    double  peak;               /* 0.9: the winner's mean cost must lie below peak * the worst; (0, 1].  A choice, not measured */
    int32_t ssd_win;            /* SSDWin 7: N, the window is (2N+1)^2; 0..15                    */
    int32_t ref_frm_count;      /* refFrmCount 5 (DepthOptimizer.cpp:45); odd, 1..9              */
    int32_t levels;             /* 128: L disparity levels; 2..1024.  A choice, not measured     */
    int32_t min_refs;           /* 2: references a level needs to be eligible; 1..8.  A choice, not measured */
    int32_t flags;              /* MVS_RECOVER_SUBSTEP = 1                                       */
    int32_t reserved;           /* 0                                                             */
} mvs_depth_recover_params;
/* the values in the comments above; flags = MVS_RECOVER_SUBSTEP */
void mvs_depth_recover_default_params(mvs_depth_recover_params* p);
int mvs_recover_depth_maps(int32_t n_seq, const int32_t* cam_off /*n_seq+1*/, const mvs_camera* cams, const uint8_t* imgs,
                           const mvs_depth_recover_params* p, float* out, int16_t* level_out /*or NULL*/, int32_t* sum_out /*or NULL*/,
                           uint8_t* cnt_out /*or NULL*/);
/* images and outputs in HBM, in the order of hip_stream (may be NULL); cam_off and cams stay host arrays; returns with the work
 * complete */
int mvs_recover_depth_maps_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev,
                               const mvs_depth_recover_params* p, float* out_dev, int16_t* level_out_dev, int32_t* sum_out_dev,
                               uint8_t* cnt_out_dev, void* hip_stream);

/* ------------------------------------------------- depth recovery with semi-global aggregation of the cost volume -- */
/* mvs_recover_depth_maps lets every pixel choose its level by itself (R6): a window with little texture picks whatever level happens to
 * score lowest.  This call regularises the cost volume along 4 or 8 path directions (semi-global matching, Hirschmueller) before the
 * winner is taken.  The rules S1-S6 below are this library's definition, NOT VERIFIED against any ZJU code; everything they do not
 * mention is R1-R5 and R9 unchanged.  p1, p2 and cost_cap are choices: nobody has measured them on a real sequence (they were moved
 * from 64, 1024, 4095 on the evidence of one synthetic scene, tests/depth_sgm_scenes.py).  mvs_recover_depth_maps is not changed by this
 * entry.  With len = 2 N + 1 and the *rectangle* of a frame R3's candidate set [N, w - N) x [N, h - N):
 *   S1 volume     : for every pixel p of the rectangle and level l, with sum_l and cnt_l of R5: C(p, l) = min(cost_cap, sum_l / (cnt_l *
 *                   len * len)) by int64 division when cnt_l >= min_refs, and C(p, l) = cost_cap otherwise.  A pixel with no eligible
 *                   level is a flat column of cost_cap and passes messages through.
 *   S2 paths      : for each direction r of the set, over the pixels of the rectangle, with q = p - r: L_r(p, l) = C(p, l) when q is
 *                   outside the rectangle; otherwise L_r(p, l) = C(p, l) + min(L_r(q, l), L_r(q, l - 1) + p1, L_r(q, l + 1) + p1,
 *                   M_r(q) + p2) - M_r(q) with M_r(q) = min over k of L_r(q, k).  A neighbour level outside [0, L - 1] does not take
 *                   part.  The directions are (+-1, 0), (0, +-1) for paths = 4; paths = 8 adds (+-1, +-1).  S(p, l) = the sum over r of
 *                   L_r(p, l).  The argument checks guarantee L_r <= cost_cap + p2 <= 8190 and S <= 65520: both fit uint16.  All of
 *                   it is integers: no schedule can change a byte.
 *   S3 winner     : l* is the lowest l that minimises S(p, l).
 *   S4 acceptance : with the raw (sum, cnt) of level l* and W the worst eligible raw level as R6 finds it, the pixel is accepted when
 *                   l* is eligible and R7's two tests hold for m = sum / cnt of l* and m_W.  sum_out and cnt_out report level l*'s raw
 *                   pair; they are -1 and 0 when l* is not eligible or the pixel is outside the rectangle.  agg_out = S(p, l*), and -1
 *                   outside the rectangle.  level_out = l* when accepted, else -1; out = +0.0f when rejected.
 *   S5 substep    : (MVS_RECOVER_SUBSTEP) R8 with c-, c0, c+ = (double)S(p, l* - 1), (double)S(p, l*), (double)S(p, l* + 1) when both
 *                   neighbours lie in [0, L - 1].  Eligibility is not asked: S is defined at every level.
 *   S6 value      : R9.
 * With p1 = p2 = 0, S2 gives L_r = C: the call is then the winner-takes-all of the quantised, capped cost.
 * The work: the grey rasters and the squares of the plain sweep; then, per group of frames, one launch that writes C as uint16 in the
 * layout [frame][pixel of the rectangle][level] (level fastest) and the worst eligible raw pair of every pixel, one launch per line
 * family (rows, columns, and for paths = 8 the two diagonals) in which one wave64 walks one line in both directions and adds L_r into the
 * uint16 volume S, and one launch that takes the winner and writes the outputs.  No atomic; two runs give the same bytes.  Frames are
 * processed in groups of as many whole frames as the budget holds (max_volume_mb; 0: MVS_SGM_VOLUME_MB of csrc/knobs.h, 4096); a
 * frame's result depends on nothing outside its sequence's images, so the bytes do not depend on the grouping.  Scratch comes from the
 * stream-ordered pool: what the plain sweep takes, and per group 4 bytes per (rectangle pixel, level) for the two volumes plus 8 bytes
 * per rectangle pixel and 8 per camera.
 * MVS_E_INVALID_ARG, before a device is needed: everything mvs_recover_depth_maps reports, and p1 < 0, p1 > p2, p2 > 4095, cost_cap
 * outside [1, 4095], paths other than 4 or 8, max_volume_mb < 0, reserved != 0, and a frame whose volumes do not fit the budget (the
 * message says how many megabytes one frame needs).  aggregate may be NULL (the defaults). */
typedef struct mvs_depth_aggregate_params {  /* 24 bytes */
    int32_t p1;             /* 8: penalty for a change of one level along a path; 0 .. p2.  A choice, not measured */
    int32_t p2;             /* 128: penalty for any larger change; p1 .. 4095.  A choice, not measured */
    int32_t cost_cap;       /* 255: 1 .. 4095: a level's cost is capped here; an ineligible level costs exactly this.  A choice, not measured */
    int32_t paths;          /* 8: 4 or 8 */
    int32_t max_volume_mb;  /* 0: the library's default budget; > 0: device memory the volumes of one group of frames may take */
    int32_t reserved;       /* 0 */
} mvs_depth_aggregate_params;
/* the values in the comments above */
void mvs_depth_aggregate_default_params(mvs_depth_aggregate_params* p);
int mvs_recover_depth_maps_aggregated(int32_t n_seq, const int32_t* cam_off /*n_seq+1*/, const mvs_camera* cams, const uint8_t* imgs,
                                      const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* aggregate /*or NULL*/, float* out,
                                      int16_t* level_out /*or NULL*/, int32_t* sum_out /*or NULL*/, uint8_t* cnt_out /*or NULL*/,
                                      int32_t* agg_out /*or NULL*/);
/* images and outputs in HBM, in the order of hip_stream (may be NULL); cam_off and cams stay host arrays; returns with the work
 * complete */
int mvs_recover_depth_maps_aggregated_dev(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev,
                                          const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* aggregate, float* out_dev,
                                          int16_t* level_out_dev, int32_t* sum_out_dev, uint8_t* cnt_out_dev, int32_t* agg_out_dev,
                                          void* hip_stream);

/* ------------------------------------------------- vertex colours (the pictures back onto the stitched model) -- */
/* The colour of every vertex of Model.obj / PSR%d.obj / deform.obj from the base images of all cameras of all sequences.  The reference
 * has no such stage: the rules C1-C8 below are this library's definition, NOT VERIFIED against any ZJU code.  min_cos = 0.2, occ_tol =
 * 0.01, the cos^2 weight and its 1/4096 quantum are choices: nobody has measured them on a real sequence.
 * Input: V vertices and V normals (fp64) in the world frame; n_seq, the SRT chain (scales, R row-major, t; all NULL: the world frame),
 * cam_off and cams as mvs_render_depth_views takes them; imgs[N][h][w][3] uint8 and depths[N][h][w] float32 inverse depth (or NULL) of
 * all cameras back to back in camera order, N = cam_off[n_seq].  Every camera must have cams[0]'s size, w, h >= 2: the one viewport of
 * mvs_render_depth_views, whose rasters are what depths is meant to hold.  All floating-point arithmetic is fp64 + - * / sqrt in the
 * order written (the library is built with -ffp-contract=off); cvt_i32 is the double -> int rule of mvs_point_sample (truncation toward
 * zero).  For vertex i (point p, normal n) and view (k, c), the views taken in camera order:
 *   C1 map        : p' = (1 / s_k) R_k^T (p - t_k) and n' = R_k^T n, operation for operation as mvs_srt_apply(inverse = 1): M = (1.0 /
 *                   s_k) * R_k^T element by element, p' = M (p - t_k), every row ((a x + b y) + c z).  Without a chain p and n as given.
 *   C2 projection : q = R_c p' + t_c (the camera's map, rows as above, then + t).  The view is rejected unless q.z > 0.  x = fx * q.x /
 *                   q.z + cx, y = fy * q.y / q.z + cy; rejected unless 0 <= x <= w - 1 and 0 <= y <= h - 1 (a NaN rejects).
 *   C3 facing     : m = R_c n'; dot = -((m.x q.x + m.y q.y) + m.z q.z); cos = dot / sqrt(((m.x m.x + m.y m.y) + m.z m.z) * ((q.x q.x +
 *                   q.y q.y) + q.z q.z)).  Rejected unless cos >= min_cos; a NaN normal rejects every view.
 *   C4 occlusion  : only when depths is given.  u = cvt_i32(x + 0.5), v = cvt_i32(y + 0.5), d = (double)depths[view][v][u].  Rejected
 *                   unless d > 0 and fabs(q.z * d - 1.0) <= occ_tol.  The nearest pixel alone is tested, no neighbourhood.
 *   C5 sample     : bilinear, in integers.  x0 = min(cvt_i32(x), w - 2), ax = cvt_i32((x - x0) * 256.0 + 0.5), in [0, 256]; y0 and ay
 *                   likewise.  Per channel S = (256 - ax)(256 - ay) I[y0][x0] + ax (256 - ay) I[y0][x0+1] + (256 - ax) ay I[y0+1][x0] +
 *                   ax ay I[y0+1][x0+1]: an exact integer, at most 255 * 65536.
 *   C6 weight     : Wq = max(1, cvt_i32(cos * cos * 4096.0 + 0.5)).
 *   C7 accumulate : in int64, A_ch += Wq * S_ch and B += Wq.  The sums commute: no schedule can change a byte.  With MVS_COLOUR_BEST the
 *                   one accepted view of greatest Wq replaces the blend; a tie goes to the lowest view index.
 *   C8 result     : colour_ch = (A_ch + 32768 * B) / (65536 * B) by integer division, stored as uint8 in the channel order of the images.
 *                   n_views[i] is the count of accepted views, also under MVS_COLOUR_BEST.  A vertex with no accepted view gets `fill`
 *                   and the count 0.
 * A facet index is never read: occlusion comes from the rasters alone.  The work is ONE launch for all vertices and all views, the camera
 * and SRT tables staged once per workgroup, without atomics; below 262 144 vertices a row of 16 lanes shares the views of a vertex and
 * reduces the integer sums over the row, above it a thread walks all views of its vertex (MVS_COLOUR_MAPPING in the environment, read at
 * every call: 1 or 16 fixes the mapping, for measurements and tests; the bytes are the same).  Two runs give the same bytes.  The tables must
 * fit 64 KiB (144 bytes per camera, 168 per sequence): chunking the views is not built; the int64 sums would make it exact.
 * V = 0 is MVS_OK and writes nothing.  MVS_E_INVALID_ARG, before a device is needed, naming the entry: min_cos outside (0, 1], occ_tol
 * not finite or <= 0, an unknown flag bit, reserved != 0, V < 0 or V >= 2^31 - 1, a NULL points, normals (mvs_mesh_vertex_normals
 * computes them), imgs, colours, cam_off or cams, n_seq < 1, cam_off not ascending from 0, no camera, a chain given in part, a camera
 * whose size is not cams[0]'s, w or h < 2, w * h above 2^31 - 1, tables above 64 KiB.  prm == NULL: the defaults. */
#define MVS_COLOUR_BEST 1
typedef struct mvs_colour_params {  /* 24 bytes */
    double  min_cos;            /* 0.2: C3; (0, 1].  A choice, not measured                      */
    double  occ_tol;            /* 0.01: C4, relative to the vertex's depth; > 0.  A choice, not measured */
    int32_t flags;              /* MVS_COLOUR_BEST = 1                                           */
    uint8_t fill[3];            /* 128, 128, 128: the colour of a vertex no view accepts         */
    uint8_t reserved;           /* 0                                                             */
} mvs_colour_params;
/* the values in the comments above; flags = 0 */
void mvs_colour_default_params(mvs_colour_params* p);
int mvs_colour_vertices(const double* points, const double* normals, int64_t V, int32_t n_seq, const double* scales, const double* R,
                        const double* t, const int32_t* cam_off /*n_seq+1*/, const mvs_camera* cams, const uint8_t* imgs,
                        const float* depths /*or NULL*/, const mvs_colour_params* prm /*NULL: defaults*/, uint8_t* colours /*V*3*/,
                        int32_t* n_views /*V or NULL*/);
/* points, normals, images, rasters and outputs in HBM, in the order of hip_stream (may be NULL); the tables stay host arrays; returns
 * with the work complete */
int mvs_colour_vertices_dev(const double* points_dev, const double* normals_dev, int64_t V, int32_t n_seq, const double* scales,
                            const double* R, const double* t, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs_dev,
                            const float* depths_dev, const mvs_colour_params* prm, uint8_t* colours_dev, int32_t* n_views_dev,
                            void* hip_stream);

/* ------------------------------------------------- base images (cv::imread of <imgdir>%05d.jpg) -- */
/* The batched baseline JPEG decoder: the frames the reference opens with cv::imread (R/Image3D/Image3D.cpp:21, R/Processor/Processor.cpp:
 * 532,545, R/FeatureProc/FeatureProc.cpp:26, R/DepthRecovery/DepthOptimizer.cpp:13-14), all images of a call through each kernel in one
 * launch.  The rules below are this library's definition.  They are pinned byte for byte against the default decompressor of
 * libjpeg-turbo (API 6.2, as Pillow 12.2.0 runs it: np.asarray(Image.open(f))) on the streams of tests/golden/jpeg.  They are NOT VERIFIED
 * against the libjpeg that OpenCV 3.0 bundles in the reference's build: an IJG 9 build upsamples the chroma of subsampled files
 * differently.
 *   J1 accepted  : SOF0 and SOF1 (8-bit, Huffman); 1 component, or 3 components taken as Y Cb Cr; one interleaved scan; sampling factors
 *                  luma 1x1, 2x1 or 2x2 with chroma 1x1 (a single component counts as 1x1 whatever it states); DQT with 8- or 16-bit
 *                  entries; up to 4 + 4 Huffman tables; DRI / RSTn; APPn and COM skipped, the EXIF orientation ignored as cv::imread of
 *                  OpenCV 3.0 does.  Everything else is MVS_E_IO with the image index and the feature in mvs_last_error():
 *                  "progressive", "arithmetic coding", "lossless or hierarchical", "12-bit samples", "<n> components", "Adobe transform
 *                  0", "non-interleaved or multi-scan", "sampling factors";
 *   J2 walk      : host code.  It reads the sizes, the tables and the segment table: one entry per restart interval, or one for the whole
 *                  scan when DRI = 0, each with image, first byte, end byte, first MCU and MCU count.  A marker is FF followed by a byte
 *                  that is neither 00 nor FF; a segment ends at the FF of the next marker or at the end of the data.  The scan must hold
 *                  exactly ceil(MCUs / interval) segments and end with EOI or with the data.  The walk reads nothing past len;
 *   J3 entropy   : canonical Huffman codes of 1-16 bits from BITS / HUFFVAL; receive / extend as T.81 F.2.2; the DC predictor of every
 *                  component is 0 at the start of every segment; FF 00 is one FF byte, an FF followed by anything else ends the
 *                  segment's bits; size categories up to 15; the predictor is int32 (wrapping), a coefficient is stored as int16,
 *                  truncating.  A segment that runs out of bits, or meets a code that is not in its table, a run past coefficient 63 (a
 *                  ZRL that ends past 64 included) or a DC size category above 15 makes the call fail with MVS_E_IO naming the image.
 *                  The decoder never reads a byte outside its segment and never writes outside its MCU range; every loop is bounded by
 *                  the segment's byte count and by MCUs x blocks x 64;
 *   J4 IDCT      : libjpeg's jidctint (Loeffler-Ligtenberg-Moshovitz, CONST_BITS 13, PASS1_BITS 2): columns first, the quantiser
 *                  multiplied in, descaled by 11; then rows, descaled by 18, + 128, clamped to 0..255.  Constants 2446, 3196, 4433, 6270,
 *                  7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172.  All arithmetic is 32-bit two's-complement wrapping; libjpeg's
 *                  zero-AC short cuts give the general path's values, so there is no branch;
 *   J5 upsample  : "fancy" upsampling.  A chroma plane has cw = ceil(W h_c / h_max) by ch = ceil(H v_c / v_max) real samples; edges use
 *                  those, never the MCU padding.  Horizontal 2:1: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] +
 *                  2) >> 2, first = p[0], last = p[cw-1].  2:1 both ways: s = 3 near + far, far the row above for even output rows and
 *                  the row below for odd ones, first and last row replicated; out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i]
 *                  + s[i+1] + 7) >> 4, first = (4 s[0] + 8) >> 4, last = (4 s[cw-1] + 7) >> 4.  A plane of cw <= 2 is replicated in both
 *                  directions instead (out[x][y] = p[y / 2][x / 2]), as libjpeg-turbo does for planes that narrow.  Cropped to W x H;
 *   J6 colour    : cb, cr minus 128; r = y + ((91881 cr + 32768) >> 16), g = y + ((-22554 cb - 46802 cr + 32768) >> 16), b = y +
 *                  ((116130 cb + 32768) >> 16); arithmetic shifts; clamped to 0..255.  A 1-component file writes its sample to all three
 *                  channels, as cv::imread does;
 *   J7 order     : flags bit 0: MVS_JPEG_BGR (0) is cv::imread's layout, what mvs_gen_new_views and the match filter take; MVS_JPEG_RGB
 *                  (1) is what mvs_refine_depth_maps documents;
 *   J8 batch     : all images of a call have one size W x H (W, H <= 65535 by the format), as the cameras of a sequence do; n <= 65535;
 *                  else MVS_E_INVALID_ARG before anything is launched.  A rejected stream (J1, J2) is reported first.
 * The encoder (mvs_jpeg_encode, rules E1-E9) follows the decoder's entries below. */
#define MVS_JPEG_BGR 0u
#define MVS_JPEG_RGB 1u
typedef struct {
    int32_t w, h, components, h_samp, v_samp, restart_interval, n_segments, sof;   /* h_samp, v_samp: the luma's, as J1 counts them */
} mvs_jpeg_info_t;
/* J1, J2 on one stream: host only, no device needed */
int mvs_jpeg_info(const uint8_t* data, int64_t len, mvs_jpeg_info_t* out);
/* stream i is data[offsets[i] .. offsets[i+1]); imgs receives n x h x w x 3 bytes (mvs_jpeg_info of a stream gives w and h) */
int mvs_jpeg_decode(int32_t n, const int64_t* offsets /*n+1, ascending from 0*/, const uint8_t* data, uint32_t flags,
                    uint8_t* imgs /*n x h x w x 3*/);
/* the streams stay a host array, the pixels are written in HBM, in the order of hip_stream (may be NULL); returns with the work complete */
int mvs_jpeg_decode_dev(int32_t n, const int64_t* offsets, const uint8_t* data /*host*/, uint32_t flags, uint8_t* imgs_dev,
                        void* hip_stream);

/* The batched baseline JPEG encoder: cv::imwrite of the generated views (R/Image3D/Image3D.cpp:218-219) and of the depth previews
 * (R/Common/Utils.h:189-217), all images of a call through each kernel in one launch.  The rules below are this library's definition.
 * They are pinned byte for byte against the default compressor of libjpeg-turbo (API 6.2, as Pillow 12.2.0 runs it:
 * Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s, restart_marker_blocks=r), optimize off, no dpi / exif / icc) on the inputs
 * of tests/golden/jpeg_enc.  They are NOT VERIFIED against the libjpeg that OpenCV 3.0 bundles in the reference's build.
 *   E1 input     : n images of one size W x H (1 .. 65535 each, n <= 65535), uint8: [n, h, w, 3] in B G R (MVS_JPEG_BGR) or R G B
 *                  (MVS_JPEG_RGB) order, or [n, h, w] grey (MVS_JPEG_GREY: one component).  mvs_jpeg_encode_params: quality 1 .. 100
 *                  (default 95, cv::imwrite's); sampling 444 / 422 / 420 (default 420: what jpeg_set_defaults leaves and cv::imwrite does
 *                  not change; checked but not used for grey); restart_interval in MCUs, 0 .. 65535 (default 0, as OpenCV writes) or
 *                  MVS_JPEG_RESTART_ROW: one MCU row per interval; reserved = 0 is not checked.  params == NULL: the defaults.  Anything
 *                  else is MVS_E_INVALID_ARG before a launch and before a device is looked for;
 *   E2 colour    : int32, arithmetic shift: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 +
 *                  32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16;
 *   E3 planes    : in this order: a full-resolution plane is extended to the right to whole MCUs by repeating its last column, and
 *                  downward only to a multiple of v_max rows by repeating its last row.  Then it is downsampled: 2:1 horizontally
 *                  (a + b + bias) >> 1 with bias 0, 1, 0, 1, ... by output column; 2:1 both ways (a + b + c + d + bias) >> 2 with bias 1,
 *                  2, 1, 2, ...; 1:1 a copy.  Then every downsampled plane, luma included, is extended downward to whole MCUs by repeating
 *                  its last downsampled row.  (Repeating input rows to the MCU height instead gives other chroma bytes whenever H mod 16
 *                  is in 1 .. 8 at 4:2:0.);
 *   E4 FDCT      : libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2) on samples minus 128, the forward twin of J4 with the same twelve
 *                  constants.  descale(x, n) = (x + (1 << (n - 1))) >> n.  On eight values d0 .. d7: tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1
 *                  = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4; tmp10 = tmp0 + tmp3, tmp13 =
 *                  tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2; z1 = (tmp12 + tmp13) 4433; out2 = descale(z1 + 6270 tmp13, s),
 *                  out6 = descale(z1 - 15137 tmp12, s); z1 = tmp4 + tmp7, z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7, z5 = (z3 +
 *                  z4) 9633; tmp4 *= 2446, tmp5 *= 16819, tmp6 *= 25172, tmp7 *= 12299; z1 *= -7373, z2 *= -20995, z3 = -16069 z3 + z5,
 *                  z4 = -3196 z4 + z5; out7 = descale(tmp4 + z1 + z3, s), out5 = descale(tmp5 + z2 + z4, s), out3 = descale(tmp6 + z2 +
 *                  z3, s), out1 = descale(tmp7 + z1 + z4, s).  Rows first: out0, out4 = (tmp10 +- tmp11) << 2 and s = 11; then columns:
 *                  out0, out4 = descale(tmp10 +- tmp11, 2) and s = 15.  The result is 8 times the DCT; int32 cannot overflow on 8-bit
 *                  input;
 *   E5 quantise  : base tables T.81 K.1 (luma) and K.2 (chroma); scale = 5000 / q for q < 50 (integer division), else 200 - 2 q; entry =
 *                  clamp((base * scale + 50) / 100, 1, 255).  A coefficient c with entry e becomes sign(c) * ((|c| + 4 e) / (8 e)),
 *                  integer division: half away from zero;
 *   E6 blocks    : one interleaved scan, MCUs in row-major order; inside an MCU luma's v x h blocks row-major, then Cb, then Cr.  A
 *                  component has ceil(cw / 8) x ceil(ch / 8) real blocks, cw = ceil(W h_c / h_max), ch = ceil(H v_c / v_max).  An MCU
 *                  position outside them is a dummy block: it codes as DC difference 0 followed by EOB and leaves the predictor
 *                  unchanged;
 *   E7 entropy   : the four tables of T.81 K.3-K.6.  DC: the size category of the difference and its bits, d - 1 for a negative d.  AC,
 *                  in zigzag order: run / size symbols, ZRL (F0) for every 16 zeros in front of a non-zero coefficient, EOB (00) when the
 *                  block ends in zeros.  Bits go MSB first; a produced FF byte is followed by 00.  At the end of every restart interval
 *                  and of the scan the last byte is filled with 1 bits; then FF D0+k follows, k counting the intervals mod 8, and the
 *                  predictors return to 0;
 *   E8 stream    : FF D8; APP0 FF E0 00 10 'JFIF' 00 01 01 00 00 01 00 01 00 00; one DQT segment per table (8-bit entries in zigzag
 *                  order: table 0, and table 1 unless grey); SOF0 (precision 8, H, W, ids 1 2 3, sampling bytes, tables 0 1 1); DHT as
 *                  separate segments in the order DC0, AC0, DC1, AC1 (grey: DC0, AC0); DRI only when the interval is above 0; SOS
 *                  (table selectors 00 11 11, then 00 3F 00); the scan; FF D9.  Nothing else;
 *   E9 batch     : offsets[n + 1] is always written; a total above capacity is MVS_E_INVALID_ARG after that (the rule of
 *                  mvs_point_sample: the caller can size the output and call again).  mvs_jpeg_encode_bound is an upper bound of one
 *                  stream.  Stream positions come from scans, never from an atomic counter: two runs give the same bytes. */
#define MVS_JPEG_GREY 2u
#define MVS_JPEG_RESTART_ROW 65536
typedef struct mvs_jpeg_encode_params {   /* 16 bytes */
    int32_t quality, sampling, restart_interval, reserved;
} mvs_jpeg_encode_params;
void mvs_jpeg_encode_default_params(mvs_jpeg_encode_params* p);
/* bytes that hold any stream of E1-E8 for one w x h image with these flags and params (NULL: the defaults): 640 for the header, then
 * every scan block at 23 + 63 * 26 bits, every interval's last byte, all of it doubled as if every byte were an FF, and two bytes of
 * marker per interval.  Not tight.  A negative value is the error code (MVS_E_INVALID_ARG).  Host code, no device needed */
int64_t mvs_jpeg_encode_bound(int32_t w, int32_t h, uint32_t flags, const mvs_jpeg_encode_params* p);
/* image i's stream is data[offsets[i] .. offsets[i+1]); capacity: the bytes data can take */
int mvs_jpeg_encode(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p,
                    int64_t* offsets /*n+1*/, uint8_t* data, int64_t capacity);
/* pixels and streams in HBM, offsets a host array; in the order of hip_stream (may be NULL); returns with the work complete */
int mvs_jpeg_encode_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                        int64_t* offsets /*n+1, host*/, uint8_t* data_dev, int64_t capacity, void* hip_stream);
/* The pixels mvs_jpeg_decode returns (same order flag; n x h x w x 3, a grey input in all three channels) for mvs_jpeg_encode of the
 * input, without producing a stream: entropy coding is lossless, so the call runs E2-E5 and then J4-J7 on those coefficients.  What
 * SIFT sees after proj%d_%d.jpg. */
int mvs_jpeg_roundtrip(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p,
                       uint8_t* out /*n x h x w x 3*/);
int mvs_jpeg_roundtrip_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                           uint8_t* out_dev, void* hip_stream);
/* RenderDepthMap's grey image (R/Common/Utils.h:189-217) for n rasters of w x h floats: per raster d_min / d_max over the valid values
 * (d >= 0 and finite: an order-free min / max; NaN is not >= 0; +inf is left out here because the reference's expression is undefined
 * on it); a valid pixel is (uint8)(255 * ((double)d - d_min) / (d_max - d_min)), truncating; 255 where the pixel is not valid; 0 for
 * every valid pixel when d_max == d_min (undefined in the reference: a division by zero); a raster without a valid pixel is all 255. */
int mvs_depth_preview(int32_t n, int32_t w, int32_t h, const float* depths, uint8_t* out /*n x h x w*/);
int mvs_depth_preview_dev(int32_t n, int32_t w, int32_t h, const float* depths_dev, uint8_t* out_dev, void* hip_stream);

/* The match and SIFT overlay pictures: the drawing of R/Processor/Processor.cpp:767-793 (every frame pair of two adjacent sequences:
 * cv::vconcat of the two base images, per match two radius-1 rings in (255,255,0) and a thickness-2 line in a cv::RNG colour; :486-505
 * is the same code) and of R/FeatureProc/FeatureProc.cpp:67-73 and Processor.cpp:604-615 (a filled radius-1 mark in (0,255,0) at every
 * key point of a generated view), all canvases of a call in ONE launch.  The rules below are this library's definition, chosen to give
 * the reference's pixels for what the reference draws.  They are RECALLED from OpenCV 3.0's drawing.cpp and cv::RNG and NOT VERIFIED
 * against it: OpenCV is neither on the machines this was written on nor in the reference tree.  csrc/overlay_rules.h holds every
 * decision as one body for host and device.
 *   O1 canvas    : n canvases (1 .. 65535) of h x w x 3 bytes, 1 <= w, h <= 16384.  A colour is three bytes in the canvas's own channel
 *                  order;
 *   O2 primitive : mvs_draw_prim, 24 bytes.  kind is MVS_DRAW_DISC, MVS_DRAW_RING or MVS_DRAW_SEGMENT; (x0, y0) is the centre of a disc
 *                  or ring and one end A of a segment, (x1, y1) the segment's other end B (not read for a disc or ring); size is the
 *                  radius r (0 .. 255) of a disc or ring, or the thickness T (1 .. 255) of a segment; c the colour; pad is not read.
 *                  Canvas i owns prims[prim_offsets[i] .. prim_offsets[i+1]), prim_offsets ascending from 0;
 *   O3 coverage  : exact in int64.  Pixel p = (x, y), dx = x - x0, dy = y - y0.  DISC: dx^2 + dy^2 <= r^2 (r = 1: the 5-pixel plus of
 *                  cv::circle(.., 1, .., -1)).  RING: (r-1)^2 < dx^2 + dy^2 <= r^2; r = 0: the centre pixel; r = 1: the 4 pixels of
 *                  cv::circle(.., 1, colour).  SEGMENT: the capsule 4 dist(p, AB)^2 <= T^2; with e = p - A, d = B - A, L2 = d.d, s = e.d:
 *                  s <= 0: 4 |e|^2 <= T^2; s >= L2: 4 |p - B|^2 <= T^2; otherwise 4 (e.x d.y - e.y d.x)^2 <= T^2 L2.  A == B is a disc
 *                  of diameter T.  Deviation: for the reference's T = 2 OpenCV fills a polygon around the line and round caps at its
 *                  ends in 16.16 fixed point; the capsule is that shape up to the pixels on the fixed-point rim;
 *   O4 order     : a pixel takes the colour of the covering primitive with the HIGHEST index in its canvas's list; a pixel nothing
 *                  covers keeps the source pixel.  This is sequential painting stated as a gather, as mvs_gen_new_views states the
 *                  reference's scatter: every pixel is written once, nothing races, out == in is allowed;
 *   O5 range     : disc and ring centres may lie anywhere with |coordinate| <= 2^20 and are clipped; segment ends must lie inside the
 *                  canvas.  Anything else is MVS_E_INVALID_ARG naming canvas and primitive, before a device is looked for.  With O1
 *                  every product of O3 stays below 2^62 (the bounds stand next to the arithmetic in overlay_rules.h);
 *   O6 colours   : cv::RNG as recalled: the state is uint64, 0xffffffff by default; next() is state = (uint32)state * 4164903690 +
 *                  (state >> 32), returning the low 32 bits; a double is ((uint64)next() << 32 | next()) * 5.4210108624275221700372640043497e-20
 *                  with the high word drawn first.  Per match, in this order, r, g, b = (uint8)(double * 255); the line colour is
 *                  (b, g, r) in a B G R canvas.  The generator is sequential and cheap and runs on the host; one generator runs through
 *                  all (i, j) of a sequence pair in row-major order, as :768 has it.
 * A cv::Point2f becomes a pixel by cvRound, round half to even (the SIFT keys are floats): one helper, which gives INT_MIN for NaN and
 * for values outside int32 as the double -> int helper of mvs_gen_new_views does; such a mark is clipped away. */
#define MVS_DRAW_DISC 0
#define MVS_DRAW_RING 1
#define MVS_DRAW_SEGMENT 2
typedef struct mvs_draw_prim {            /* 24 bytes */
    int32_t x0, y0, x1, y1;
    uint8_t kind, size, c[3], pad[3];
} mvs_draw_prim;
/* out [n][h][w][3] = imgs [n][h][w][3] with every canvas's list painted (O1-O5) */
int mvs_draw_overlays(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const int64_t* prim_offsets /*n+1*/, const mvs_draw_prim* prims,
                      uint8_t* out);
/* the pixels in HBM (out_dev may be imgs_dev), the lists host arrays that are uploaded; in the order of hip_stream (may be NULL);
 * returns with the work complete */
int mvs_draw_overlays_dev(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, const int64_t* prim_offsets, const mvs_draw_prim* prims,
                          uint8_t* out_dev, void* hip_stream);
/* O6: n line colours from the generator at *state (in / out), bgr [n][3] = (b, g, r) each.  Host code, no device needed; a NULL
 * pointer or n < 1 does nothing */
void mvs_cv_rng_colours(uint64_t* state, int64_t n, uint8_t* bgr /*n x 3*/);
/* Processor.cpp:767-793 for all n1 x n2 frame pairs: canvas i*n2 + j of out [n1*n2][2h][w][3] is imgs1[i] over imgs2[j] (rows 0 .. h-1
 * and h .. 2h-1; the stack is never materialised as an input) with, per match (u1, v1, u2, v2) of pair i*n2 + j in list order, a ring
 * (r = 1, (255,255,0)) at (u1, v1), one at (u2, h + v2) and a segment (T = 2) between them in the next colour of O6.  matches
 * [total][4] with match_offsets (n1*n2 + 1) is the `out` / `out_offsets` of mvs_match_filter_pairs; the images are B G R.  rng_state
 * (in / out; NULL: a fresh default generator) runs through the pairs in order: 6 draws per match.  n1*n2 <= 65535, 2h <= 16384; a
 * match with an end outside its image is MVS_E_INVALID_ARG naming pair and match. */
int mvs_match_overlays(int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1 /*n1 x h x w x 3*/, const uint8_t* imgs2 /*n2 x h x w x 3*/,
                       const int64_t* match_offsets /*n1*n2+1*/, const int32_t* matches /*total x 4*/, uint64_t* rng_state,
                       uint8_t* out /*n1*n2 x 2h x w x 3*/);
/* images and canvases in HBM; the match lists host arrays; one launch does the stack and the drawing, in the order of hip_stream (may be
 * NULL); returns with the work complete */
int mvs_match_overlays_dev(int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1_dev, const uint8_t* imgs2_dev,
                           const int64_t* match_offsets, const int32_t* matches, uint64_t* rng_state, uint8_t* out_dev, void* hip_stream);
/* FeatureProc.cpp:67-69 / Processor.cpp:607-609 for n_lists views: out = views with a filled r = 1 disc in (0,255,0) at cvRound of the
 * (x, y) of every key of the view's list, keys [total][4] = (x, y, s, o) floats with key_offsets (n_lists + 1) as mvs_sift_detect and
 * mvs_keypoint_cull return them. */
int mvs_sift_overlays(int32_t n_lists, int32_t w, int32_t h, const uint8_t* views /*n_lists x h x w x 3*/, const int64_t* key_offsets,
                      const float* keys, uint8_t* out);
/* views and out in HBM (out_dev may be views_dev), the key lists host arrays; in the order of hip_stream (may be NULL); returns with the
 * work complete */
int mvs_sift_overlays_dev(int32_t n_lists, int32_t w, int32_t h, const uint8_t* views_dev, const int64_t* key_offsets, const float* keys,
                          uint8_t* out_dev, void* hip_stream);

/* ------------------------------------------------- surface reconstruction (GeometryRec::RunPoisson) -- */
/* The one call between the stitch tail and the trim of the model (R/Processor/Processor.cpp:1042-1058): the oriented points of
 * Result/PSR.npts to the triangle mesh of Result/Model.obj that mvs_processor_cull_model reads.  GeoRec is a closed binary; its source is
 * not part of the reference tree.  The rules below are NOT VERIFIED against GeoRec; they are this library's definition: an unscreened
 * Poisson reconstruction on a dense grid stands in for GeoRec's octree.  GeometryRec::Init receives maxPsDep / minPsDep from config.txt
 * (PsnDptMax 10, PsnDptMin 7); here they are depth_max / depth_min: the grid has 2^D cells per axis, D is never below depth_min, never
 * above min(depth_max, MVS_POISSON_MAX_DEPTH) and, in between, as fine as the sampling supports (rule 3).
 * Input: n rows of points[3] and normals[3] (doubles, the layout of mvs_npts_read); the normals point out of the body and are unit
 * vectors or shorter (a component of magnitude 2^26 or more overflows rule 5's quantisation; its result is unspecified).  All
 * arithmetic is fp64 + - * / in the stated order (the library is built with -ffp-contract=off).
 *   1. used points : a row is used when its six values are finite; N = the used rows.  N < 2, or a bounding box of zero extent, gives
 *                    MVS_E_DEGENERATE; N > 2^26 gives MVS_E_INVALID_ARG (the sums of rule 5 stay inside int64).
 *   2. cube        : lo, hi = the componentwise min and max of the used points; c = 0.5 * (lo + hi); side = scale * max(hi - lo);
 *                    o = c - 0.5 * side.
 *   3. depth       : Dmax = min(depth_max, MVS_POISSON_MAX_DEPTH).  At depth d the cell of a point is, per axis,
 *                    clamp(floor((p - o) / (side / 2^d)), 0, 2^d - 1); occupied(d) = the distinct such cells.  D = the largest d in
 *                    [depth_min, Dmax] with (double)N >= samples_per_node * (double)occupied(d), depth_min when no d qualifies.
 *   4. grid        : G = 2^D, h = side / G; nodes (ix, iy, iz) in [0, G]^3 at o + h * i, node index (iz * (G + 1) + iy) * (G + 1) + ix.
 *                    Boundary nodes carry chi = 0.
 *   5. splat       : per used point g = (p - o) / h, i0 = clamp(floor(g), 0, G - 1), f = g - i0 per axis; corner (bx, by, bz) of the
 *                    cube at i0 has the weight w = (wx * wy) * wz, each factor f (bit set) or 1 - f.  The contribution x = w * n_a to
 *                    component a at that corner is quantised, q = llrint(x * 2^36) (round to nearest even), and summed in int64 per
 *                    node and component; V_a = (double)sum * 2^-36.  Integer sums do not depend on their order.
 *   6. right side  : at interior nodes b = (((Vx[ix+1] - Vx[ix-1]) + (Vy[iy+1] - Vy[iy-1])) + (Vz[iz+1] - Vz[iz-1])) * (0.5 * h).
 *   7. system      : for every interior node (the sum of the six neighbours' chi) - 6 chi = b: the unscaled 7-point Laplacian with
 *                    zero Dirichlet boundary.
 *   8. solve       : multigrid V(2,2) cycles (Jacobi damped by 6/7, full weighting, trilinear prolongation, levels D .. 1) until the
 *                    true residual, recomputed on the device after every cycle, satisfies |b - A chi|_2 <= solve_tol * |b|_2;
 *                    max_cycles without that gives MVS_E_SOLVER (info holds the residual reached).  The norms are sums of
 *                    per-workgroup partials in a fixed order: two runs agree to the bit.  b = 0 gives chi = 0 at once.
 *   9. iso value   : iso = the mean over the used points of the trilinear chi (corners and weights of rule 5, added in corner order
 *                    bx + 2 by + 4 bz), reduced in a fixed order: partials per workgroup, then one workgroup.
 *  10. inside      : a node is inside when chi < iso (a value equal to iso is outside); with outward normals the mesh is wound
 *                    outward.  Every cube (ix, iy, iz) in [0, G)^3 is cut into the six Kuhn tetrahedra along its (0,0,0)-(1,1,1)
 *                    diagonal: tetrahedron (a, b, c) has the corners q0 = cube origin, q1 = q0 + e_a, q2 = q1 + e_b, q3 = q2 + e_c,
 *                    taken in the order xyz, xzy, yxz, yzx, zxy, zyx.  Every edge of a tetrahedron leaves its lower node by one of
 *                    seven types 0..6 = +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z; neighbouring cubes agree on every shared face.
 *  11. vertices    : an edge (node, type) with exactly one inside end carries one vertex: with a, pa at the inside end and b, pb at
 *                    the outside end, t = (iso - a) / (b - a), p = pa + t * (pb - pa).  Vertices are numbered in ascending
 *                    (node index, type); vertices that coincide in position keep distinct numbers.
 *  12. triangles   : a tetrahedron with inside corners I and outside corners O (both non-empty) emits the polygon over its I-O
 *                    edges: for |I| = 1 or 3 the triangle over the three edges, for I = {A, B}, O = {C, D} the quad AC, AD, BD, BC.
 *                    The cycle is reversed when the polygon's normal — (p1 - p0) x (p2 - p0), for the quad plus (p2 - p0) x (p3 - p0)
 *                    — has a negative dot product with mean(O corners) - mean(I corners), then rotated so that its smallest
 *                    vertex number comes first.  A triangle is (v0, v1, v2), a quad (v0, v1, v2) then (v0, v2, v3).  Faces are
 *                    ordered by cube index (iz * G + iy) * G + ix, then by tetrahedron, then as listed.
 *  13. no crossing : V = F = 0 and MVS_OK.
 * info is written by every call that gets as far as the device; counts above a capacity (rows) give MVS_E_INVALID_ARG after info is
 * written, so that the caller can size the outputs.
 * Scratch comes from the stream-ordered pool.  Per node of the finest level, (G + 1)^3 of them: 24 bytes for the three int64 sums —
 * reused for chi and the smoother's second buffer — and 8 for b; 1 byte per cube; 7/8 byte for the edge flags (one bit each, 7 per
 * node); 12 bytes per 256 edge flags and per 256 face slots (12 per cube) for the two compactions.  Per node of every level below,
 * (2^l + 1)^3 for l < D: 24 bytes.  2^(3 d - 3) bytes per candidate depth d of rule 3 when depth_min < Dmax.  8 bytes per workgroup of
 * the residual norm.  The host form adds the points, the normals and the mesh.  D = 9 takes about 5 GB.
 * MVS_E_INVALID_ARG, before a device is needed: points, normals, params or info NULL, an output NULL with a capacity above 0, n < 0, a
 * negative capacity, a non-finite or non-positive scale, samples_per_node or solve_tol, scale <= 1 + 4.0 / 2^depth_min (every point
 * then lies at least a cell from the boundary), depth_min < 3, depth_min > depth_max, depth_min > MVS_POISSON_MAX_DEPTH, max_cycles < 1. */
#define MVS_POISSON_MAX_DEPTH 9
typedef struct mvs_poisson_params {
    double  scale;              /* 1.1: the cube's side over the largest extent of the points    */
    double  samples_per_node;   /* 1.5                                                           */
    double  solve_tol;          /* 1e-8                                                          */
    int32_t depth_max;          /* PsnDptMax 10; above MVS_POISSON_MAX_DEPTH means that depth    */
    int32_t depth_min;          /* PsnDptMin 7                                                   */
    int32_t max_cycles;         /* 64                                                            */
    int32_t reserved;           /* 0                                                             */
} mvs_poisson_params;
typedef struct mvs_poisson_info {
    double  origin[3], h;       /* o and h of rules 2 and 4                                      */
    double  iso;                /* rule 9                                                        */
    double  rel_residual;       /* |b - A chi|_2 / |b|_2 after the last cycle                    */
    int64_t n_used;             /* N of rule 1                                                   */
    int64_t n_vertices, n_faces;
    int32_t depth, cycles;      /* D of rule 3; V-cycles run                                     */
} mvs_poisson_info;
/* the values in the comments above */
void mvs_poisson_default_params(mvs_poisson_params* p);
int mvs_poisson_reconstruct(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p, mvs_poisson_info* info,
                            double* vertices /*vertex_capacity x 3*/, int64_t vertex_capacity, int32_t* faces /*face_capacity x 3*/,
                            int64_t face_capacity);
/* points, normals and outputs in HBM, in the order of hip_stream (may be NULL); params and info stay host structs; returns with the work
 * complete */
int mvs_poisson_reconstruct_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                mvs_poisson_info* info, double* vertices_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                int64_t face_capacity, void* hip_stream);

/* Sampling density: weighting of the normals, a density per vertex, and a trim of the mesh by it.  PSR.npts concatenates every
 * sequence's points, so the sampling density doubles where two sequences overlap; rule 5 splats every normal with unit mass, the jump of
 * chi across the surface follows the local density and the one iso value of rule 9 cuts the surface at the wrong offset where the
 * density differs from the mean.  Rules 14-18 continue the list above; like rules 1-13 they are this library's definition and are NOT
 * VERIFIED against GeoRec.  By default the weighting is off and nothing is trimmed: the results are those of mvs_poisson_reconstruct.
 *  14. density grid : Dd = max(D - density_drop, 2), Gd = 2^Dd, hd = side / Gd, the origin o of rule 2.  Every used point has the corners
 *                    and weights of rule 5 on that grid; q = llrint(w * 2^36) is summed in int64 per node; W = (double)sum * 2^-36.
 *  15. point density: rho_p = the trilinear W at p: corners and weights of rule 14, added in corner order bx + 2 by + 4 bz.  A point sees
 *                    its own splat: rho_p >= 1/8 up to the quantisation.  rho_mean = ((double) sum_p llrint(rho_p * 2^16)) * 2^-16 /
 *                    (double)N: an int64 sum, which does not depend on its order (it stays inside int64 while sum_p rho_p < 2^47,
 *                    which every N <= 2^23 ensures; beyond that the result is unspecified).
 *  16. weighted splat (flag MVS_POISSON_WEIGHT_NORMALS): s_p = min(rho_mean / rho_p, max_gain), and rule 5's contribution becomes
 *                    x = w * (n_a * s_p).  With the flag a call of more than 2^22 rows, used or not, gives MVS_E_INVALID_ARG: with
 *                    w <= 1, |n_a| <= 1 and s_p <= max_gain <= 16 = 2^4 a contribution is at most 2^36 * 2^4 = 2^40 units, and 2^22 of
 *                    them stay at or below 2^62, inside int64 like the 2^26 unit contributions of rule 1.  Rules 6-13 are unchanged;
 *                    the iso value of rule 9 is the unweighted mean over the points, as without the flag.
 *  17. vertex density: d_v = the trilinear W, evaluated as in rule 15, at the vertex position p of rule 11 (clamped into the grid as
 *                    rule 5 clamps).
 *  18. trim         : given V vertices, F faces, values[V] and a threshold, a vertex passes when values[v] >= threshold (NaN does not
 *                    pass); a face is kept when its three vertices pass; a vertex is kept when it passes and lies in a kept face.
 *                    Kept vertices and kept faces keep their order, the faces are renumbered.  Nothing kept: V = F = 0 and MVS_OK.
 * mvs_poisson_reconstruct_density takes the arguments of mvs_poisson_reconstruct, the density parameters, a second info and
 * vertex_density (vertex_capacity doubles, d_v of rule 17 per vertex; may be NULL).  With flags = 0 vertices, faces and info hold the
 * bytes mvs_poisson_reconstruct gives, with or without vertex_density.  dinfo is written by every call that gets as far as the device
 * and past rule 4.  Scratch, beyond that of mvs_poisson_reconstruct and from the same pool: 8 bytes per node of the density grid,
 * (Gd + 1)^3 of them — at most an eighth of the solve grid's nodes at density_drop = 1 —, 16 bytes per row (rho_p and s_p) and 24 bytes per
 * workgroup of the reduction over the points.
 * MVS_E_INVALID_ARG, before a device is needed: what mvs_poisson_reconstruct refuses, dparams or dinfo NULL, max_gain not finite or
 * outside [1, 16], density_drop outside [0, 8], a flag other than MVS_POISSON_WEIGHT_NORMALS, n > 2^22 with that flag. */
#define MVS_POISSON_WEIGHT_NORMALS 1
typedef struct mvs_poisson_density_params {
    double  max_gain;           /* 4: the largest s_p of rule 16                                 */
    int32_t flags;              /* 0; MVS_POISSON_WEIGHT_NORMALS                                 */
    int32_t density_drop;       /* 1: levels the density grid lies below the solve grid          */
} mvs_poisson_density_params;
typedef struct mvs_poisson_density_info {
    double  mean_density;       /* rho_mean of rule 15                                           */
    double  min_point_density, max_point_density;   /* over the used points                      */
    int32_t density_depth;      /* Dd of rule 14                                                 */
    int32_t n_clamped;          /* used points with rho_mean / rho_p > max_gain                  */
} mvs_poisson_density_info;
/* the values in the comments above */
void mvs_poisson_density_default_params(mvs_poisson_density_params* p);
int mvs_poisson_reconstruct_density(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                    const mvs_poisson_density_params* dparams, mvs_poisson_info* info, mvs_poisson_density_info* dinfo,
                                    double* vertices, double* vertex_density, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity);
/* the device form, as mvs_poisson_reconstruct_dev */
int mvs_poisson_reconstruct_density_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                        const mvs_poisson_density_params* dparams, mvs_poisson_info* info, mvs_poisson_density_info* dinfo,
                                        double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                        int64_t face_capacity, void* hip_stream);
/* Screening: the point-interpolation term of Kazhdan and Hoppe (Screened Poisson Surface Reconstruction, 2013).  Rules 1-9 cut one iso
 * surface at the mean of chi over the points; where the local jump of chi differs from the mean the surface sits at the wrong offset.
 * The screened call penalises (chi(p) - T)^2 at every used point p, T the iso value of the unscreened field: a second solve that starts
 * from that field.  Rules 19-23 continue the list above; like rules 1-18 they are this library's definition and are NOT VERIFIED against
 * GeoRec.  alpha = 0 does no second solve: vertices, faces, vertex_density, info and dinfo hold the bytes of
 * mvs_poisson_reconstruct_density, and sinfo holds cycles = 0, lambda = 0, target = iso_unscreened = iso.
 *  19. weight      : occ = occupied(D) of rule 3, computed also when depth_min == Dmax; m = max(1.0, (double)N / (double)occ);
 *                    lambda = alpha / m, the same for every used point.  MVS_POISSON_WEIGHT_NORMALS keeps its meaning for both solves
 *                    and does not change lambda.
 *  20. stencil     : every used point has the eight corners and weights w_c of rule 5 (the scale check makes all eight interior nodes).
 *                    For every unordered corner pair c1 <= c2 (corner order bx + 2 by + 4 bz) x = (lambda * w_c1) * w_c2 and
 *                    q = llrint(x * 2^30); q is added in int64 to the entry (node of c1, offset c2 - c1) and, for c1 != c2, also to the
 *                    entry (node of c2, offset c1 - c2): the stencil is exactly symmetric and does not depend on the order of the
 *                    points.  S_{i,o} = (double)sum * 2^-30 for the 27 offsets o in {-1, 0, 1}^3, kept in the order
 *                    (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); rs_i = (double)(the int64 sum of node i's 27 sums) * 2^-30.
 *                    The sums stay inside int64: the 64 entries a point adds to belong to eight rows, and what it adds to one row i is
 *                    at most lambda * w_i * (the sum of its eight weights, 1 up to rounding) * 2^30 plus half a unit per entry; with
 *                    alpha <= 64 = 2^6, w <= 1 and N <= 2^26 a row sum, and so every entry of it (all are >= 0), is at most
 *                    2^6 * 2^30 * 2^26 * (1 + 2^-50) + 8 * 2^26 < 2^63.
 *  21. system      : chi0 and T are the field and the iso value of rules 1-9 (with the flag the weighted ones).  At interior nodes
 *                    (the sum of the six neighbours' chi - 6 chi_i) - sum_o S_{i,o} chi_{i+o} = f_i, f_i = b_i - T * rs_i; the
 *                    sum over o runs in the order of rule 20 into one accumulator that starts at 0.  M names the operator on the left.
 *                    The boundary stays zero Dirichlet.
 *  22. solve       : from chi0, multigrid cycles until the TRUE residual, recomputed on the device after every cycle with partial sums
 *                    in a fixed order, satisfies |f - M chi|_2 <= solve_tol * |f|_2.  max_cycles applies to this solve on its own;
 *                    failing it gives MVS_E_SOLVER with the residual reached in sinfo.  |f| = 0 gives chi = chi0.  The cycle is not
 *                    part of the definition (csrc/poisson.hip: the V(2,2) cycle of rule 8 on M_l = A_l - S_l, S_D = S and
 *                    S_l = 1/2 P^T S_(l+1) P with the trilinear prolongation P, Jacobi damped by 6/7 over the diagonal 6 + rs_i / 2).
 *  23. surface     : iso = rule 9 evaluated on the screened chi; rules 10-13 and 17 are unchanged.
 * Scratch beyond the density call's: 2^(3 D - 3) bytes for rule 19; per level 4 bytes per node (the number of the node's stencil row)
 * and 228 bytes per node that a point touches (27 entries, the row sum and the node), a few per occupied cell; 1 byte per node of the
 * finest level for the flags.
 * MVS_E_INVALID_ARG, before a device is needed: what mvs_poisson_reconstruct_density refuses, sparams or sinfo NULL, alpha not finite or
 * outside [0, 64], reserved != 0. */
typedef struct mvs_poisson_screen_params {
    double  alpha;              /* 4: the screening weight per point before rule 19's division   */
    int64_t reserved;           /* 0                                                             */
} mvs_poisson_screen_params;
typedef struct mvs_poisson_screen_info {
    double  target;             /* T of rule 21                                                  */
    double  lambda;             /* rule 19                                                       */
    double  rel_residual;       /* |f - M chi|_2 / |f|_2 after the last cycle of rule 22         */
    double  iso_unscreened;     /* rule 9 on chi0                                                */
    int64_t occupied;           /* occ of rule 19                                                */
    int64_t active_nodes;       /* nodes of the finest level with a stencil                      */
    int32_t cycles;             /* cycles of rule 22                                             */
    int32_t reserved;
} mvs_poisson_screen_info;
/* the values in the comments above */
void mvs_poisson_screen_default_params(mvs_poisson_screen_params* p);
int mvs_poisson_reconstruct_screened(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                     const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams, mvs_poisson_info* info,
                                     mvs_poisson_density_info* dinfo, mvs_poisson_screen_info* sinfo, double* vertices, double* vertex_density,
                                     int64_t vertex_capacity, int32_t* faces, int64_t face_capacity);
/* the device form, as mvs_poisson_reconstruct_dev */
int mvs_poisson_reconstruct_screened_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                         const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams,
                                         mvs_poisson_info* info, mvs_poisson_density_info* dinfo, mvs_poisson_screen_info* sinfo,
                                         double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                         int64_t face_capacity, void* hip_stream);

/* Band-refined levels over the dense grid: the way to config.txt's PsnDptMax 10.  The surface occupies O(G^2) of the G^3 cells of a
 * level; mvs_poisson_reconstruct pays for the empty volume and stops at MVS_POISSON_MAX_DEPTH.  mvs_poisson_reconstruct_band solves a
 * dense base level (base_depth, 3 .. 9) and refines it level by level on the blocks of MVS_POISSON_BAND_BLOCK^3 cells within `band`
 * blocks (1 .. 64, Chebyshev) of the points only, each level taking its boundary values from the level below: still fp64, integer splats
 * that do not depend on their order, a stop criterion on the true residual, two runs the same bytes.  It is unscreened and unweighted;
 * mvs_poisson_reconstruct_band_density, below, carries the sampling density of rules 14-17 over every level (rules 32-35); screening
 * over the band is mvs_poisson_reconstruct_band_screened, further below (rules 36-41).  Like rules 1-23 this is this library's
 * definition, NOT VERIFIED against GeoRec.
 *  24. depth       : D = rule 3 with Dmax = min(depth_max, MVS_POISSON_BAND_MAX_DEPTH).  At depth 10 the node index and the cube
 *                    index still fit in int32; a (node index, type) key needs int64.  B = min(D, base_depth).  With D <= base_depth
 *                    the result is that of mvs_poisson_reconstruct at depth_min = depth_max = D.
 *  25. base        : rules 4-8 at depth B give chi_B on the dense grid of that depth.  Every solve of the call has the budget of rule
 *                    28, max_cycles * 64 iterations; a V-cycle of the base solve counts as one.  The base solve runs one cycle past
 *                    its criterion (info.cycles counts it, info.rel_residual is the residual after it): every finer level takes
 *                    chi_B in its fixed values and its right side and cannot reduce the error it carries.
 *  26. blocks      : for every level l = B + 1 .. D: G_l = 2^l, h_l = side / G_l, and the cells form blocks of MVS_POISSON_BAND_BLOCK
 *                    cells per axis, G_l / 4 blocks per axis.  The block of a used point is the block of its level-l cell (rule 3's
 *                    formula at d = l).  A block is active when some used point's block lies at Chebyshev distance <= band blocks
 *                    from it.  A cell is active when its block is; cells outside the grid are not active.  A node is FREE when all
 *                    eight cells that touch it are active, FIXED when at least one but not all of them are, and has no value
 *                    otherwise.  The active set of level l - 1 covers that of level l (the same points, the same band, blocks twice
 *                    as wide).
 *  27. start       : every node of level l that has a value starts as 0.125 * the trilinear prolongation of chi_(l-1): a node that
 *                    coincides with a coarse node copies its value, an edge midpoint is 0.5 * (a + b), and face and cube centres
 *                    follow by the same halving applied axis after axis in the order x, y, z (first along x on the coarse rows,
 *                    then along y on those results, then along z).  The factor is a power of two: no rounding.  Fixed nodes keep
 *                    this value.  (Between two dense levels the field shrinks by 1/8 per level: the splat carries unit mass, b
 *                    carries 0.5 h, the stencil is unscaled.)
 *  28. system      : rules 5-6 at level l define b at the free nodes (V is needed one node beyond them; every such node has a
 *                    value).  The free nodes satisfy rule 7, the terms of fixed neighbours moved to the right side: A_ff chi_f = b',
 *                    b' = b - A_fc chi_c.  The solve runs until the true residual, recomputed on the device, satisfies
 *                    |b' - A_ff chi|_2 <= solve_tol * |b'|_2; the norms are sums of per-workgroup partials in a fixed order, as in
 *                    rule 8.  max_cycles * 64 iterations without that give MVS_E_SOLVER, with the level and the residual reported.
 *                    b' = 0 gives chi_f = 0 at once.  The solver is not part of the definition (csrc/poisson_band.hip: conjugate
 *                    gradients from the start values); the stop criterion and the identity of two runs are.
 *  29. iso value   : rule 9 on level D.  The cube of every used point is active, so its eight corners have values.  The sum runs
 *                    over the used points in their order, whatever rows that are not used stand between them.
 *  30. surface     : rules 10-12 over the active cubes of level D only.  An edge (node, type) exists when an active cube contains
 *                    it.  Vertices are numbered in ascending (node index, type) and faces ordered by ascending cube index, then
 *                    tetrahedron, then as listed, over what exists: the numbers of the dense call when every block is active.
 *  31. open edges  : a crossed edge of an active cube that lies on a face shared with an inactive cell, or on the boundary of the
 *                    grid, is counted in n_open_edges (once, whatever the number of such faces).  The mesh is returned as it is,
 *                    open there.  Where the solve closes a scan far from every sample, level D has no field and the surface ends;
 *                    mvs_processor_cull_model removes such closure anyway.
 * The per-point, per-block, per-node and per-edge decisions are csrc/poisson_band_rules.h.
 * info keeps its meaning: depth, h and iso are those of level D, cycles and rel_residual those of the base solve.  binfo's arrays are
 * indexed by the level l and zero outside B + 1 .. D.  info and binfo are written first; then a capacity below a count gives
 * MVS_E_INVALID_ARG and nothing is written to the outputs, as in mvs_poisson_reconstruct.  With D <= base_depth the call IS
 * mvs_poisson_reconstruct at depth_min = depth_max = D — its bytes — and binfo is zero apart from base_depth.
 * MVS_E_SOLVER: the base solve (failed_level = B) or a band level (failed_level = l, rel_residual[l] and iterations[l] what it reached).
 * Scratch, from the same pool: the base stage as mvs_poisson_reconstruct at depth B (given back after level B + 1 has started), 2^(3 d
 * - 3) bytes for one candidate depth d of rule 3 at a time, and per level (T = 2^l / 4 + 1) 7 T^3 bytes of block tables and 49.5
 * bytes per stored node (64 per stored block), two levels at most alive at once; on level D about 4 more bytes per stored node for
 * the surface (csrc/poisson_band_plan.h).  binfo.scratch_bytes is the peak of it all for the call made.  A level that needs more than
 * the device has gives MVS_E_OOM with the level named, before its arrays are asked for.
 * MVS_E_INVALID_ARG, before a device is needed: what mvs_poisson_reconstruct refuses, except that depth_min may reach
 * MVS_POISSON_BAND_MAX_DEPTH; bparams or binfo NULL; base_depth outside [3, MVS_POISSON_MAX_DEPTH]; band outside [1, 64]; a non-zero
 * reserved field.  After the blocks of a level are counted: a level whose stored nodes would not fit an int32 index (the level is
 * named in mvs_last_error). */
#define MVS_POISSON_BAND_MAX_DEPTH 10
#define MVS_POISSON_BAND_BLOCK 4
typedef struct mvs_poisson_band_params {
    int32_t base_depth;         /* 8: the depth of the dense base level                           */
    int32_t band;               /* 2: blocks around the block of a point that are active          */
    int32_t reserved[2];        /* 0                                                              */
} mvs_poisson_band_params;
typedef struct mvs_poisson_band_info {           /* arrays indexed by level l, entries outside B+1..D zero */
    int64_t n_active_blocks[MVS_POISSON_BAND_MAX_DEPTH + 1], n_free[MVS_POISSON_BAND_MAX_DEPTH + 1];
    double  rel_residual[MVS_POISSON_BAND_MAX_DEPTH + 1], bnorm[MVS_POISSON_BAND_MAX_DEPTH + 1];   /* |b' - A_ff chi| / |b'|, |b'| */
    int32_t iterations[MVS_POISSON_BAND_MAX_DEPTH + 1];
    int64_t n_open_edges, scratch_bytes;          /* rule 31; peak bytes taken from the pool by the call */
    int32_t base_depth, failed_level;             /* B of rule 24; the level of MVS_E_SOLVER, else 0    */
} mvs_poisson_band_info;
/* the values in the comments above */
void mvs_poisson_band_default_params(mvs_poisson_band_params* p);
int mvs_poisson_reconstruct_band(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                 const mvs_poisson_band_params* bparams, mvs_poisson_info* info, mvs_poisson_band_info* binfo,
                                 double* vertices, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity);
/* the device form, as mvs_poisson_reconstruct_dev */
int mvs_poisson_reconstruct_band_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                     const mvs_poisson_band_params* bparams, mvs_poisson_info* info, mvs_poisson_band_info* binfo,
                                     double* vertices_dev, int64_t vertex_capacity, int32_t* faces_dev, int64_t face_capacity,
                                     void* hip_stream);

/* The band call with the sampling density: rules 14-17 carried over every level, so that the depth config.txt asks for weights the
 * normals where sequences overlap and its mesh, the one that ends in open edges and base-level closure, has a density per vertex for
 * mvs_mesh_trim_by_value.  Rules 32-35 continue the list; like rules 1-31 they are this library's definition, NOT VERIFIED against GeoRec.
 *  32. density grid: D and B are those of rule 24.  With D <= B the call IS mvs_poisson_reconstruct_density at depth_min = depth_max
 *                    = D: its bytes, dinfo included, and binfo zero apart from base_depth.  Otherwise rule 14 applies with this D:
 *                    Dd = max(D - density_drop, 2), and rule 15 (rho_p, rho_mean, the minimum and maximum, density_depth) is
 *                    unchanged, with the same integer sums.  W is the function rule 14 defines on the full grid of depth Dd.
 *                    Storage is not part of the definition, but a memory condition is: for Dd > B no array over all (2^Dd + 1)^3
 *                    nodes is allocated.  The sums then live on stored blocks of level Dd (MVS_POISSON_BAND_BLOCK^3 cells; stored: a
 *                    block that holds a node of a cell of the block of some used point, rule 26's block without the dilation),
 *                    found through a table of the blocks, and a node without storage reads as 0.  That zero is exact: a point
 *                    adds only to the corners of its own cell, that cell's block is marked, every node that touches a marked
 *                    cell is stored, so every node with a non-zero sum is stored.  For Dd <= B the sums are a dense array, at most
 *                    the base grid's size.  The structure lives from before the base splat until rule 34.
 *  33. weighted levels (flag MVS_POISSON_WEIGHT_NORMALS): s_p of rule 16 is computed once, and the splat of rule 5 uses
 *                    x = w * (n_a * s_p) at the base level (rule 25) and at every band level (rule 28).  Rule 26's blocks depend on
 *                    the positions only and are unchanged; rule 29's iso value stays the unweighted mean over the used points.  The
 *                    limit n <= 2^22 of rule 16 applies, by the same int64 argument on every level.
 *  34. vertex density: rule 17 at the vertices of rule 30, W read as rule 32 says: 0 at a node that is not stored.  vertex_density
 *                    may be NULL.
 *  35. flags = 0   : vertices, faces, info and binfo hold the bytes of mvs_poisson_reconstruct_band, with or without vertex_density —
 *                    but for binfo.scratch_bytes, which counts the density structure.
 * The read of rule 32 is csrc/poisson_band_rules.h (bd_density_at).  dinfo is written by every call that gets past rule 24 and, with
 * D > B, past rule 32.  Capacities, MVS_E_SOLVER and MVS_E_OOM as in mvs_poisson_reconstruct_band; vertex_density holds vertex_capacity
 * doubles.  Scratch beyond the band call's, counted in binfo.scratch_bytes (csrc/poisson_band_plan.h, bd_density_bytes): 16 bytes per
 * row for rho_p and s_p, 24 bytes for each of 1024 workgroups of the reduction over the points, and the node sums — 8 (2^Dd + 1)^3
 * bytes for Dd <= B; for Dd > B 8 bytes per stored node (64 per stored block, plus 4 for its coordinates) and 4 bytes per entry of the
 * table, (2^Dd / 4 + 1)^3 of them, with 2 more bytes per entry and 8 per table row while the blocks are numbered.
 * MVS_E_INVALID_ARG, before a device is needed: what mvs_poisson_reconstruct_band refuses and what mvs_poisson_reconstruct_density
 * refuses of dparams and dinfo: either NULL, max_gain not finite or outside [1, 16], density_drop outside [0, 8], a flag other than
 * MVS_POISSON_WEIGHT_NORMALS, n > 2^22 with that flag.  Default parameters: mvs_poisson_band_default_params and
 * mvs_poisson_density_default_params. */
int mvs_poisson_reconstruct_band_density(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                         const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                         mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo,
                                         double* vertices, double* vertex_density, int64_t vertex_capacity, int32_t* faces,
                                         int64_t face_capacity);
/* the device form, as mvs_poisson_reconstruct_dev */
int mvs_poisson_reconstruct_band_density_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                             const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                             mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo,
                                             double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                             int64_t face_capacity, void* hip_stream);

/* The band-density call with screening on the base level and on every band level: the depth config.txt asks for and the point-
 * interpolation term of rules 19-23 in one call.  Every level pulls its field to a target at the samples before the next level starts
 * from it: one field and one solve per band level.  Rules 36-41 continue the list; like rules 1-35 they are this library's definition,
 * NOT VERIFIED against GeoRec.
 *  36. cases       : D and B are those of rule 24.  With D <= B the call IS mvs_poisson_reconstruct_screened at depth_min = depth_max
 *                    = D: its bytes, sinfo included; binfo is zero apart from base_depth and bsinfo is zero.  Otherwise, with alpha =
 *                    0, vertices, faces, vertex_density, info, binfo and dinfo hold the bytes of mvs_poisson_reconstruct_band_density
 *                    with the same dparams, and sinfo and bsinfo are zero.  MVS_POISSON_WEIGHT_NORMALS keeps rule 33's meaning on
 *                    every level and does not change any lambda.
 *  37. base        : rules 19-23 at depth B give the screened chi_B: chi0 and T are rule 25's field (with the flag the weighted one)
 *                    and rule 9 on it, occ = occupied(B), computed even when rule 3 does not need it.  Both solves of the base run one
 *                    cycle past their criterion, for rule 25's reason, and each has rule 25's budget.  sinfo describes this level
 *                    (cycles and rel_residual count and follow the extra cycle).
 *  38. weight and stencil of level l (B < l <= D): lambda_l = alpha / max(1.0, (double)N / (double)occupied(l)).  The stencil S_l is
 *                    rule 20's at level l with lambda_l: the same quantisation, the same symmetric int64 sums, the same offset order
 *                    and the same int64 bound.  Every node that a used point touches is FREE: the eight cells around a corner of the
 *                    point's cell lie within one cell of that cell, hence in blocks at Chebyshev distance <= 1 <= band from the
 *                    point's block, which are active (the scale check keeps them inside the grid), and a node whose eight cells are
 *                    active is FREE.  So S_l has no entry at a FIXED node: a row belongs to a FREE node and each of its 27 offsets
 *                    points at a node that is touched too or carries a zero entry, and every one of the 26 neighbours of a node with
 *                    a row has a value and is stored.  Storage is not part of the definition, but a memory condition is: no array
 *                    over all nodes of a level is allocated, and rows exist only for touched nodes.
 *  39. target      : T_l is rule 29's mean (the used points in their order) evaluated on the START values of level l, which are rule
 *                    27 applied to the screened chi of level l - 1.  No unscreened solve is made on a band level.
 *  40. system      : the free nodes satisfy rule 21's equation with lambda_l, S_l and T_l, the terms of fixed neighbours moved to
 *                    the right: M_ff chi_f = f', f' = f - A_fc chi_c, f = b - T_l rs (b of rule 28).  The solve runs from the start
 *                    values until |f' - M_ff chi|_2 <= solve_tol * |f'|_2 on the true residual, recomputed on the device with
 *                    partials in a fixed order.  The budget is rule 28's; past it the call returns MVS_E_SOLVER with the level
 *                    named.  f' = 0 gives chi_f = 0.  binfo.rel_residual, bnorm (|f'|) and iterations of level l describe this
 *                    solve.  The solver is not part of the definition (csrc/poisson_band.hip: conjugate gradients on the positive
 *                    definite -M_ff, preconditioned by its diagonal 6 + S_{i,0}); the stop criterion and the identity of two runs are.
 *  41. surface     : rule 29 on the screened chi_D; rules 30, 31 and 34 are unchanged.
 * bsinfo's arrays are indexed by the level l and zero outside B + 1 .. D.  info, binfo and dinfo keep the meaning they have in
 * mvs_poisson_reconstruct_band_density.  Capacities, MVS_E_SOLVER (failed_level = B for either solve of the base) and MVS_E_OOM as
 * there.  Scratch beyond the band-density call's, counted in binfo.scratch_bytes (csrc/poisson_band_plan.h, bd_screen_block_bytes and
 * bd_screen_row_bytes): the base as rule 23's scratch says; 8 bytes per used point for their list; per level 2^(3 l - 3) bytes for
 * occupied(l) while it is counted, per stored block 109 bytes (its 27 neighbours and a flag) and per stored node 12 bytes (the number
 * of its row, the preconditioner) plus 1 byte and the scan while the rows are numbered, and 228 bytes per touched node (27 entries, the
 * row sum and the node).  A level whose rows need more than the device has gives MVS_E_OOM with the level named, before they are asked for.
 * MVS_E_INVALID_ARG, before a device is needed: what mvs_poisson_reconstruct_band_density refuses, what
 * mvs_poisson_reconstruct_screened refuses of sparams and sinfo (either NULL, alpha not finite or outside [0, 64], reserved != 0), and
 * bsinfo NULL. */
typedef struct mvs_poisson_band_screen_info {    /* arrays indexed by level l, entries outside B+1..D zero */
    double  lambda[MVS_POISSON_BAND_MAX_DEPTH + 1], target[MVS_POISSON_BAND_MAX_DEPTH + 1];        /* rules 38 and 39      */
    int64_t occupied[MVS_POISSON_BAND_MAX_DEPTH + 1], active_nodes[MVS_POISSON_BAND_MAX_DEPTH + 1]; /* occupied(l); the rows */
} mvs_poisson_band_screen_info;
int mvs_poisson_reconstruct_band_screened(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                          const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                          mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo,
                                          double* vertices, double* vertex_density, int64_t vertex_capacity, int32_t* faces,
                                          int64_t face_capacity, const mvs_poisson_screen_params* sparams, mvs_poisson_screen_info* sinfo,
                                          mvs_poisson_band_screen_info* bsinfo);
/* the device form, as mvs_poisson_reconstruct_dev */
int mvs_poisson_reconstruct_band_screened_dev(int64_t n, const double* points_dev, const double* normals_dev, const mvs_poisson_params* p,
                                              const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                              mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo,
                                              double* vertices_dev, double* vertex_density_dev, int64_t vertex_capacity, int32_t* faces_dev,
                                              int64_t face_capacity, void* hip_stream, const mvs_poisson_screen_params* sparams,
                                              mvs_poisson_screen_info* sinfo, mvs_poisson_band_screen_info* bsinfo);

/* Rule 18 on any triangle mesh: vertices[V][3], normals[V][3] (may be NULL, then normals_out is not written), faces[F][3], values[V].
 * The outputs hold V resp. F rows and do not overlap the inputs; V_out / F_out receive the rows kept.  An ordered compaction without
 * atomics: two runs give the same bytes.  MVS_E_INVALID_ARG, before a device is needed: a NULL argument other than normals /
 * normals_out (normals given without normals_out included), V or F negative or above 2^31 - 1, a NaN threshold.  MVS_E_BAD_MESH: a
 * face index outside [0, V). */
int mvs_mesh_trim_by_value(int64_t V, const double* vertices, const double* normals, int64_t F, const int32_t* faces, const double* values,
                           double threshold, double* vertices_out, double* normals_out, int32_t* faces_out, int64_t* V_out, int64_t* F_out);
/* arrays in HBM, in the order of hip_stream (may be NULL); V_out / F_out stay host pointers; returns with the work complete */
int mvs_mesh_trim_by_value_dev(int64_t V, const double* vertices_dev, const double* normals_dev, int64_t F, const int32_t* faces_dev,
                               const double* values_dev, double threshold, double* vertices_out_dev, double* normals_out_dev,
                               int32_t* faces_out_dev, int64_t* V_out, int64_t* F_out, void* hip_stream);

/* Chain composition, Processor.cpp:819-823: (s0,R0,t0) <- (sk,Rk,tk) o (s0,R0,t0). */
int mvs_srt_compose(double sk, const double* Rk, const double* tk,
                    double* s0, double* R0, double* t0);
/* Cross-sequence map k -> k0, Processor.cpp:979-982. */
int mvs_srt_relative(double s_k0, const double* R_k0, const double* t_k0,
                     double s_k,  const double* R_k,  const double* t_k,
                     double* s, double* R, double* t);
/* Point map over P points (+normals, may be NULL):
 * forward  v = s R p + t, n' = R n          (Processor.cpp:1021-1027)
 * inverse  p = (1/s) R^T (v - t), n' = R^T n (Processor.cpp:1183-1184). */
int mvs_srt_apply(const double* pts, const double* normals, int64_t P,
                  double s, const double* R, const double* t, int inverse,
                  double* out_pts, double* out_normals);
/* Same map, device pointers (zero-copy from mvs_depth_* device output). */
int mvs_srt_apply_dev(const double* pts_dev, const double* normals_dev, int64_t P,
                      double s, const double* R, const double* t, int inverse,
                      double* out_pts_dev, double* out_normals_dev, void* hip_stream);

/* ------------------------------------------- chain refinement (joint ICP) -- */
/* Refine the SRT chain on the sequences' oriented points: a joint point-to-plane similarity ICP over the overlaps of ALL sequences,
 * between the pairwise feature fit that made the chain (Processor.cpp:813-823) and the fusion of the points
 * (mvs_processor_stitch_points).  The reference has no such stage.  The rules I1-I9 are this library's definition, NOT VERIFIED against
 * any ZJU code; rel_dist = 0.02, min_cos = 0.7 and min_pairs = 64 are choices measured on no real sequence.  The per-match part (I1,
 * I3-I6) is one host/device body, csrc/srt_refine_rules.h; tests/ref_srt_refine.py restates all nine in numpy.
 *
 * points, normals: the rows of each sequence's .npts in that sequence's OWN frame, segment k = [seg_off[k], seg_off[k+1]) (host,
 * n_seq + 1 offsets ascending from 0).  scales[n_seq], R[n_seq*9] (row-major), t[n_seq*3]: the chain as mvs_visibility_cull takes
 * it, read and, when a step was made, overwritten.  iters_done: the steps made.  history (optional, iters*2 doubles): per step the
 * accepted matches of all pairs and the rms residual before the step, D sqrt(sum r^2 / count), in common-frame units; rows
 * [iters_done, iters) are not written.  pair_count (optional, n_seq*n_seq): the accepted matches of the last search, [a*n_seq+b] for
 * the queries of a against the points of b.
 *
 *   I1 maps      : entry k maps y = s_k R_k p + t_k as mvs_srt_apply does (M = s_k R_k element by element, then M p + t).  A normal is
 *                  used as n / |n| in fp64.  A point takes part iff its three coordinates are finite and no larger than FLT_MAX in
 *                  magnitude (they stay finite as float32): any other point is never a query and never a nearest point.  A point
 *                  whose normal is not finite or has |n|^2 zero or not finite is still searched, and its match is rejected.
 *   I2 frame     : once per call, from the input chain: lo, hi = the bounding box of the mapped points that take part, c = (lo+hi)/2,
 *                  D = |hi-lo|/2, normalised coordinates x = (y-c)/D, the cap is 2 rel_dist.  No such point, D == 0 or D not finite
 *                  is MVS_E_DEGENERATE.  The frame stays while the chain moves.
 *   I3 search    : for every ordered pair (a, b), a != b, and every query i of a (i % stride == 0): the point is mapped into b's OWN
 *                  frame by mvs_srt_relative(b, a) and mvs_srt_apply's expression in fp64, rounded to float32 (a result that is not
 *                  finite has no match), and its nearest point j of b is found by d2f (float32, FLANN's accumulation order) over
 *                  b's float32-rounded coordinates, ties to the lower index: the arithmetic and the tie rule of mvs_part_recog.
 *   I4 accept    : iff, in fp64, |x_a - x_b|^2 <= cap^2 and (R_a n_a) . (R_b n_b) >= min_cos.  The search stops early only where that
 *                  cannot change an acceptance: once every point within cap D / s_b * (1 + 1/64) + 2^-18 (E_b + cap D / s_b) of
 *                  the query has been seen (E_b: the largest coordinate magnitude of b's grid box) and none is proven nearest, there
 *                  is no match.  The slack covers the float32 rounding of both points and of d2f, and an R_b whose singular values
 *                  lie within 1 +- 2^-7.
 *   I5 terms     : with n = R_b n_b: r = n . (x_a - x_b) and the 14-vector J = [x_a x n, n, n . x_a, -(x_b x n), -n, -(n . x_b)]:
 *                  the derivative of r by (w, tau, sigma) of a, then of b (I8).  n is held fixed (point to plane).
 *   I6 sums      : per ordered pair, int64: the count; q(J_i J_j) for i <= j, row by row (105); q(J_i r) (14); q(r r): 121 numbers,
 *                  q(v) = llrint(v * 2^36), every product one fp64 multiply.  |entries| <= 1 by I2 (a little more once the chain has
 *                  moved), so the 2^24 queries a sequence may have cannot overflow.  Integer adds commute: two runs give the same
 *                  bytes.  These 121 numbers per pair are all that leaves the device per iteration.
 *   I7 solve     : on the host.  The 7 n_seq square normal matrix H = sum J^T J and the gradient g = sum J r from the dequantised
 *                  sums, pairs added in ascending (a, b) order.  The rows and columns of fixed_seq (-1: the last sequence, the
 *                  chain's identity, Processor.cpp:851-853), of every HELD sequence — fewer than min_pairs accepted matches this
 *                  iteration as query or target over all pairs, or none at all — and, with MVS_SRT_REFINE_FIX_SCALE, every scale
 *                  column are dropped; damping * (the largest diagonal entry) is added to every diagonal entry; H step = -g by
 *                  Cholesky factorisation in plain row order, no pivoting.  A pivot <= 0 is MVS_E_SOLVER.  An iteration in which no
 *                  sequence is free ends the call without a step: when that is the first, the call returns MVS_OK with the
 *                  chain's bytes unchanged and iters_done = 0.
 *   I8 step      : (w, tau, sigma) of sequence k acts in the normalised frame, x' = e^sigma Exp(w) x + tau: dR = Exp(w) (Rodrigues:
 *                  I + sin(th)/th K + (1 - cos th)/th^2 K^2, th = |w|; I for th == 0), g = e^sigma, s' = g s, R' = dR R,
 *                  t' = g dR t + (c - g dR c + D tau).
 *   I9 stop      : after the iteration whose largest |step entry| is below tol, or after `iters` iterations.
 *
 * Device side: the n_seq target grids are built once per call, in each sequence's own frame (knn.hip's grid); each iteration is ONE
 * launch over all ordered pairs and one wait: the sums come down, the host solves, the 13 n_seq doubles of the chain go up.  Scratch
 * from the stream-ordered pool: 24 bytes per point, a grid per sequence, 968 n_seq^2 bytes of sums.
 * MVS_E_INVALID_ARG, before a device is needed, naming the entry: a NULL pointer other than params (NULL: the defaults), history or
 * pair_count; n_seq < 2 or above 128; offsets that do not ascend from 0 or reach 2^31 - 1; more than 2^24 queries in one sequence;
 * rel_dist outside (0, 1], min_cos outside [-1, 1], damping or tol negative or not finite, iters outside 1..64, stride < 1,
 * fixed_seq outside -1..n_seq-1, min_pairs < 0, unknown flags, reserved != 0; a scale that is not finite and positive, an R or t
 * that is not finite. */
enum { MVS_SRT_REFINE_FIX_SCALE = 1 };           /* 6 instead of 7 unknowns per sequence */
typedef struct mvs_srt_refine_params {
    double  rel_dist;    /* 0.02  match cap, as a fraction of the bounding-box diagonal of all mapped points (I2) */
    double  min_cos;     /* 0.7   least dot product of the two unit normals in the common frame */
    double  damping;     /* 1e-9  times the largest diagonal entry, added to every diagonal entry (I7) */
    double  tol;         /* 1e-9  stop when no entry of the step exceeds it (I9) */
    int32_t iters;       /* 20    at most, 1..64 */
    int32_t stride;      /* 1     point i of a sequence is a query iff i % stride == 0 */
    int32_t fixed_seq;   /* -1    the sequence that does not move; -1 = the last (the chain's identity, Processor.cpp:851-853) */
    int32_t min_pairs;   /* 64    a sequence with fewer accepted matches (as query or target, all pairs) is held this iteration */
    int32_t flags, reserved;
} mvs_srt_refine_params;
void mvs_srt_refine_default_params(mvs_srt_refine_params* p);
int mvs_srt_refine(const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq,
                   double* scales, double* R, double* t, const mvs_srt_refine_params* p,
                   int32_t* iters_done, double* history, int64_t* pair_count);
/* Same with the points and normals in HBM; the chain and the reports stay host arrays.  Everything is ordered on hip_stream (NULL =
 * legacy default stream); returns with the work complete. */
int mvs_srt_refine_dev(const double* points_dev, const double* normals_dev, const int64_t* seg_off, int32_t n_seq,
                       double* scales, double* R, double* t, const mvs_srt_refine_params* p,
                       int32_t* iters_done, double* history, int64_t* pair_count, void* hip_stream);

/* ------------------------------------------------- stitch tail (f1) -- */
/* The visibility cull of Processor::AlignmentSeq: a point stays iff, for every sequence k0 and every camera c of k0, the point
 * mapped into k0's frame projects inside c's image (Camera::GetImgCoordFromWorld, R/Camera/Camera.cpp:45-48,68-72, then
 * CheckRange, R/Common/Utils.h:20-22).
 *   MVS_CULL_SEQUENCES (:966-1004, before Poisson): segment k holds the points of sequence k (n_seg == n_seq); for k0 != k the
 *     point is mapped by mvs_srt_relative(k0, k) forward (s R p + t, :979-982), for k0 == k it is not mapped at all (:973).
 *   MVS_CULL_ALL_SEQ (:1064-1083, AllSeqProj on the Poisson model): every k0, its own sequence included, maps by the inverse
 *     (1/s_k0) R_k0^T (p - t_k0); segments are independent point ranges (usually one).
 * seg_off: host, n_seg + 1 ascending offsets from 0 into points; scales[n_seq], R[n_seq*9] (row-major), t[n_seq*3]: the SRT
 * chain as AlignmentSeq holds it; cam_off: host, n_seq + 1 ascending offsets from 0 into cams (sequences may differ in camera
 * count and image size).  keep[P] = 1 / 0, n_keep[n_seg] = kept points per segment.  Every test is exact fp64 (true divides). */
enum mvs_cull_mode {
    MVS_CULL_SEQUENCES = 0,
    MVS_CULL_ALL_SEQ   = 1
};
int mvs_visibility_cull(const double* points, const int64_t* seg_off, int32_t n_seg, int32_t n_seq,
                        const double* scales, const double* R, const double* t,
                        const int32_t* cam_off, const mvs_camera* cams, int32_t mode,
                        uint8_t* keep, int64_t* n_keep);
/* Same with the points and the mask in HBM, enqueued on hip_stream (NULL = legacy default stream); returns once n_keep (host) is
 * known, i.e. with the stream's work up to the cull complete. */
int mvs_visibility_cull_dev(const double* points_dev, const int64_t* seg_off, int32_t n_seg, int32_t n_seq,
                            const double* scales, const double* R, const double* t,
                            const int32_t* cam_off, const mvs_camera* cams, int32_t mode,
                            uint8_t* keep_dev, int64_t* n_keep, void* hip_stream);

/* Mesh::CalculateVertexNormals for a general triangle list (R/PlyObj/PlyObj.cpp:139-185, what ReadObj computes for a file without
 * `vn` lines, :3-16): the unit normal of every facet (the 1e-6 rescue of a short edge, n/|n| — a zero-area facet gives NaN) summed
 * per vertex in ascending facet order (a facet listing a vertex twice counts twice), / count, normalised; a vertex of no facet
 * gives NaN.  No manifold test: every mesh ReadObj accepts is accepted.  A facet index outside [0, V) is MVS_E_BAD_MESH. */
int mvs_mesh_vertex_normals(int64_t V, const double* points, int64_t F, const int32_t* faces, double* out_normals);
int mvs_mesh_vertex_normals_dev(int64_t V, const double* points_dev, int64_t F, const int32_t* faces_dev,
                                double* out_normals_dev, void* hip_stream);

/* ---------------------------------------------------- Alignment (a10-a15) -- */
/* Template -> scan coarse alignment, class Alignment (R/Alignment/Alignment.h:21-36) and its helpers.
 * Labels are the 16 body parts of enum PART (R/PartRecognition/PartRecognition.h:13-30), 0..31 accepted;
 * a `mask` selects points by label (bit l = label l), labels == NULL selects every point.
 * Conventions for what the reference leaves open (PCA axis sign, component tie-break, the erased label of
 * LocalAlignmentCore) are listed in DESIGN.md §3. */

/* PointSetUtils::SetInput + CalcPivots (R/SetUtils/PointSetUtils.cpp:3-61): barycentre, bounding box
 * {min xyz, max xyz}, the three pivots (row i of axes = i-th pivot, largest eigenvalue first), eigenvalues.
 * Fewer than 2 selected points (n of 0 or 1 included): MVS_E_DEGENERATE, nothing is written; mvs_remove_ground[_dev], whose
 * first step this is, answer a scan of 0 or 1 vertices the same way and leave counts and arrays alone. */
int mvs_pca(const double* pts, int64_t n, const int32_t* labels, uint32_t mask,
            double* barycentre /*3*/, double* bbox /*6*/, double* axes /*9*/, double* eigenvalues /*3*/);

/* Alignment::RetainConnectRegion (Alignment.cpp:618-654): keep the largest facet-connected component,
 * compact points / normals (may be NULL) / facets IN PLACE; V, F in/out. */
int mvs_retain_connect_region(int64_t* V, double* pts, double* normals, int64_t* F, int32_t* faces);

/* Alignment::RemoveGround (Alignment.cpp:79-233): dist_thres = ParamParser::dist_thres (R/config.txt:37);
 * in place like the reference; ground_ray[3] out. */
int mvs_remove_ground(int64_t* V, double* pts, double* normals, int64_t* F, int32_t* faces,
                      double dist_thres, double* ground_ray);
/* The two on DEVICE arrays, trimmed in place — a view's mesh as mvs_depth_to_model_dev leaves it (R/Image3D/Image3D.cpp:87-88
 * trims every view's mesh), the fused scan (Processor.cpp:1103-1104).  They wait for the device before they start (the arrays
 * come from some other stream) and return with the arrays final; normals_dev may be NULL; ground_ray is a HOST array. */
int mvs_retain_connect_region_dev(int64_t* V, double* pts_dev, double* normals_dev, int64_t* F, int32_t* faces_dev);
int mvs_remove_ground_dev(int64_t* V, double* pts_dev, double* normals_dev, int64_t* F, int32_t* faces_dev,
                          double dist_thres, double* ground_ray);

/* Alignment::InitAlignment (Alignment.cpp:235-314): src -> tgt similarity from PCA axes and extents. */
int mvs_init_alignment(const double* src, int64_t ns, const double* tgt, int64_t nt,
                       const double* ground_ray, const double* view_ray, double* R /*9*/, double* t /*3*/, double* scale);

/* InitAlignment with the scan sharded over ranks by view: `tgt_local` holds this rank's share (may be empty), the
 * template `src` is replicated.  The scan's count / sums, bounding box, centred second moments (PointSetUtils.cpp:9-39) and its
 * extent along the first pivot (Alignment.cpp:281-296) are reduced over the ranks through the caller's all-reduce — four calls
 * of at most 7 doubles (the last one is the ranks' failure flag, see mvs_local_alignment_core_sharded) — so every rank returns the same R, t, scale; they equal mvs_init_alignment on the whole scan up to the
 * order of the floating-point sums.  `reduce(ctx, v, n, op)` all-reduces the n HOST doubles v in place, op 0 = sum, 1 = min,
 * and returns 0 on success; mvs_comm_reduce (ctx = an mvs_comm_t) is a ready one over RCCL. */
typedef int (*mvs_reduce_fn)(void* ctx, double* v, int n, int op);
int mvs_init_alignment_sharded(const double* src, int64_t ns, const double* tgt_local, int64_t nt_local,
                               const double* ground_ray, const double* view_ray, mvs_reduce_fn reduce, void* reduce_ctx,
                               double* R /*9*/, double* t /*3*/, double* scale);

/* RemoveGround with the scan sharded over ranks by view (R/Alignment/Alignment.cpp:79-233): the arrays hold this
 * rank's points / normals / facets (facets never join points of two ranks).  The moments, the two extents along the first pivot
 * (:103-113), the candidate counts (:115-138), the plane-fit sums (:148-153) and the largest plane distance (:182-187) are reduced
 * through `reduce`; removal and compaction are local; of the connected components (:227, RetainConnectRegion) the largest over
 * ALL ranks stays (ties: the lower rank) and every other rank is left with V = F = 0.  Every rank returns the same ground_ray.
 * Equal to mvs_remove_ground on the stitched scan up to the order of the floating-point sums. */
int mvs_remove_ground_sharded(int64_t* V, double* pts, double* normals, int64_t* F, int32_t* faces, double dist_thres,
                              mvs_reduce_fn reduce, void* reduce_ctx, int rank, double* ground_ray);

/* PartRecognition::PartRecog (R/PartRecognition/PartRecognition.cpp:50-77): label of the nearest template vertex. */
int mvs_part_recog(const double* tmpl_pts, const int32_t* tmpl_labels, int64_t V,
                   const double* pts, int64_t P, int32_t* out_labels);
/* ... with template, labels, queries and result on the device (same waiting rule as above). */
int mvs_part_recog_dev(const double* tmpl_pts_dev, const int32_t* tmpl_labels_dev, int64_t V,
                       const double* pts_dev, int64_t P, int32_t* out_labels_dev);

/* Alignment::LocalAlignmentCore (Alignment.cpp:423-546) for one limb group (slabel == tlabel == label). */
int mvs_local_alignment_core(const double* src, const int32_t* s_labels, int64_t ns,
                             const double* tgt, const int32_t* t_labels, int64_t nt,
                             uint32_t group_mask, int label, double* R /*9*/, double* t /*3*/, double* scale);

/* LocalAlignmentCore with the scan sharded over ranks by view (template replicated): the scan's labelled moments, the labels
 * present (Alignment.cpp:475-477), its extent along the limb axis and the label at its far end (:519-528) are reduced through
 * `reduce`; every rank returns the same R, t, scale.  When several points reach the largest projection the reference keeps the
 * first of them (strict >, :521): here the lowest `rank` (= position of this share in the stitched scan) that reaches it, and within
 * the rank the lowest index.
 *
 * All three sharded entries: a rank whose LOCAL stage fails (allocation, copy, kernel) still joins the next reduce, which carries one
 * more element — the failure flag — so every rank returns an error from the same collective instead of waiting for the failed one
 * (the failed rank returns its own code and message, the others MVS_E_STATE).  `reduce` must therefore accept any n <= 24.
 * After mvs_remove_ground_sharded only ONE rank still holds points (RetainConnectRegion keeps one component and facets never join
 * two ranks' points): the stages the reference runs next (InitAlignment, PartRecog, LocalAlignment) are then single-rank work with
 * empty shares elsewhere — the sharded forms of those exist for scans sharded WITHOUT that trim (per-view parts, config 5). */
int mvs_local_alignment_core_sharded(const double* src, const int32_t* s_labels, int64_t ns,
                                     const double* tgt_local, const int32_t* t_labels_local, int64_t nt_local,
                                     uint32_t group_mask, int label, mvs_reduce_fn reduce, void* reduce_ctx, int rank,
                                     double* R /*9*/, double* t /*3*/, double* scale);

/* Alignment::Align (Alignment.cpp:11-76; call site R/Processor/Processor.cpp:1130-1131) without its file I/O:
 * tgt / t_normals / t_faces are trimmed in place (ground removal + largest component; nt, nf in/out),
 * src / s_normals are moved in place, t_labels (capacity: the input *nt) receives the scan's part labels
 * (what PartRecog returns), ground_ray[3] (optional) the detected ground direction.  s_labels are the template's
 * part labels (the contents of ./Template/part/parts, Alignment.cpp:38-41). */
int mvs_align(double* src, double* s_normals, int64_t ns, const int32_t* s_labels,
              double* tgt, double* t_normals, int64_t* nt, int32_t* t_faces, int64_t* nf,
              const double* view_ray, double dist_thres, int32_t* t_labels, double* ground_ray);
/* The same with the scan resident in HBM (tgt_dev / t_normals_dev / t_faces_dev / t_labels_dev are DEVICE arrays, trimmed in
 * place — what mvs_depth_to_model_dev / mvs_srt_apply_dev leave and mvs_deform_set_target_dev takes); the template stays a host
 * argument.  The call waits for the device before it starts (the caller's arrays come from some other stream). */
int mvs_align_dev(double* src, double* s_normals, int64_t ns, const int32_t* s_labels,
                  double* tgt_dev, double* t_normals_dev, int64_t* nt, int32_t* t_faces_dev, int64_t* nf,
                  const double* view_ray /*3*/, double dist_thres, int32_t* t_labels_dev, double* ground_ray /*3, optional*/);

/* ------------------------------------------------------------------ tracing */
/* SURVEY §8b "Side effects": the engine writes no files and prints nothing (the reference's only timer is a clock() pair around
 * PartRecog printed to stdout, R/Alignment/Alignment.cpp:46-52).  A caller that wants timing registers a callback: every compute
 * entry of this header then calls fn(ctx, "mvs_<entry>", 0, 0) when entered and fn(ctx, "mvs_<entry>", 1, ms) when left (ms = host
 * wall time of the call; entries that only enqueue return before the device has finished — mvs_deform_kernel_time has the
 * device-side phase times).  Process-wide; NULL switches it off.  mvs_set_trace_roctx(1) additionally marks every entry as a
 * roctx range (rocprofv3 --marker-trace) when libroctx64 is present. */
typedef void (*mvs_trace_fn)(void* ctx, const char* entry, int phase, double host_ms);
int mvs_set_trace(mvs_trace_fn fn, void* ctx);
int mvs_set_trace_roctx(int on);

/* ----------------------------------------------------- Deformation (a16-a22) */
typedef struct mvs_deform_s* mvs_deform_t;

typedef struct mvs_deform_params {
    double  proj_len_err;    /* Deform(...,projLenErr,...)  = 100.0  Processor.cpp:1136 */
    double  proj_dist_err;   /* Deform(...,projDistErr)     = 100.0                      */
    double  min_cos;         /* 0.1     Deformation.cpp:353                               */
    int32_t max_result;      /* 10000   Deformation.cpp:244                               */
    int32_t top_k;           /* 8       Deformation.cpp:338 (<= 8)                        */
    int32_t graph_k;         /* 8  -> 9-NN incl. self, w = 1/9   Deformation.cpp:359,143  */
    int32_t smooth_sweeps;   /* 2       Deformation.cpp:362                               */
    int32_t arap_iters;      /* 5       Deformation.cpp:398                               */
    double  arap_tol;        /* 1e-4    Deformation.cpp:398                               */
    double  cg_tol;          /* 1e-8: relative residual (M^-1 norm of the rhs) at which the
                                CG global solve stops; build's own — the reference
                                factorises with SparseLU inside CGAL.  Measured: vertex
                                RMS vs a direct solve ~ 0.6 * cg_tol per outer iteration  */
    int32_t cg_max_iters;    /* safety cap                                                */
    int32_t update_normals;  /* 0: keep ctor normals for every outer iteration as the
                                reference does (Deformation.cpp:34,304); 1: recompute
                                (Deformation.h:86-128) after each outer iteration        */
    int32_t solver;          /* MVS_SOLVER_AUTO: overlapping-patch sweeps with LDS-resident local
                                solves when the mesh fits (>= 2048 vertices, degree <= 16), else
                                CG; MVS_SOLVER_CG: always the one-kernel-per-iteration CG.  Both
                                run a launch plan sized from the handle's previous solves (the host
                                follows every solve's measured residual while it enqueues and adds
                                sweeps as soon as a margin gets thin); EVERY solve's result is
                                checked on the device against cg_tol (true residual b - A x, taken
                                by the local step) and a miss is reported: MVS_W_UNCONVERGED      */
    int32_t reserved0;
} mvs_deform_params;
enum { MVS_SOLVER_AUTO = 0, MVS_SOLVER_CG = 1 };

void mvs_deform_default_params(mvs_deform_params* p);

typedef struct mvs_deform_stats {
    int32_t outer_done;
    int32_t arap_iters_run;   /* of the last outer iteration           */
    int32_t cg_iters;         /* largest per-solve CG launch count      */
    int32_t n_valid;          /* nodes with isValid (Deformation.cpp:355) */
    double  energy[8];        /* ARAP energy after each iteration      */
    double  cg_rel_residual;  /* worst TRUE relative residual (|b - A x| / |b|, M^-1 norm) over the solves of the
                                 last outer iteration                                         */
    int32_t cg_launches;      /* CG-iteration kernels launched in the last outer iteration   */
    int32_t cg_active;        /* ... of which did work (the rest exited early: converged)    */
    /* every solve since the handle's statistics were last read (the whole batch of an mvs_deform_iterate call, or
     * everything enqueued with stats == NULL before this mvs_deform_collect): */
    double  worst_rel_residual_in_batch;
    int32_t solves_in_batch;
    int32_t unconverged_solves;   /* of those, how many ended above cg_tol (0 <=> return value MVS_OK)           */
    int32_t escalated;            /* 1: after a miss the device switched the remaining solves of the batch to the
                                     strong local-solve coefficients (patch solver)                               */
    int32_t reserved1;
} mvs_deform_stats;

/* Deformation(points,normals,facets)  R/Deformation/Deformation.cpp:29-46.
 * Validity: indices in range, no repeated vertex in a facet, no directed edge
 * used twice and no edge with >2 facets (what Polyhedron_incremental_builder_3
 * + is_valid() reject, Deformation.h:65-79) -> MVS_E_BAD_MESH / _NONMANIFOLD. */
int mvs_deform_create(int64_t V, const double* points, const double* normals,
                      int64_t F, const int32_t* faces, mvs_deform_t* out);
int mvs_deform_destroy(mvs_deform_t h);

/* New positions (and, if given, normals) for the handle's mesh — SAME topology: the next fit starts from them, e.g. from the
 * template's rest pose again for the next scan of a sequence.  The reference builds a new `Deformation` per call
 * (Processor.cpp:1135); here everything that depends on the topology alone (adjacency and patch tables, node set, the solver's
 * launch plans) stays, which is what mvs_deform_create spends its time on.  The target is kept too (set a new one as needed). */
int mvs_deform_set_vertices(mvs_deform_t h, const double* points /*V*3*/, const double* normals /*V*3 or NULL: keep*/);

/* UniformSampling()  Deformation.cpp:63-106 (knn = 16). Exact NN on float32
 * coordinates.  K receives sampIdx.size(). */
int mvs_deform_sample_nodes(mvs_deform_t h, int knn, int64_t* K);
int mvs_deform_set_nodes(mvs_deform_t h, const int32_t* vertex_idx, int64_t K);
int mvs_deform_get_nodes(mvs_deform_t h, int32_t* vertex_idx /*K*/);
int mvs_deform_sizes(mvs_deform_t h, int64_t* V, int64_t* F, int64_t* K, int64_t* P);

/* Target point set of this rank (Deform(tpts,tnormals,..) arguments,
 * Deformation.cpp:232-246): float32 spatial index built on the GPU.
 * index_base = global index of pts[0] (ties between equal keys break on the
 * global index so a sharded run reproduces the single-device result). */
int mvs_deform_set_target(mvs_deform_t h, int64_t P, const double* pts,
                          const double* normals, int64_t index_base);
int mvs_deform_set_target_dev(mvs_deform_t h, int64_t P, const double* pts_dev,
                              const double* normals_dev, int64_t index_base);

/* One or more passes of the while(counter--) body, Deformation.cpp:253-401:
 * associate -> 9-NN graph -> 2 Jacobi sweeps -> ARAP(arap_iters, arap_tol) ->
 * overwrite_initial_geometry. */
int mvs_deform_iterate(mvs_deform_t h, const mvs_deform_params* p, int n_outer,
                       mvs_deform_stats* stats);
/* (n_outer passes are enqueued in batches of at most 32 between host synchronisations: each batch ends with a read-back
 * of the solver statistics from which the launch plan of the next one is made.  Inside a batch the host stays at most
 * 3 passes ahead of the device and reads, without synchronising, the residual every finished solve reported into a
 * pinned ring: a solve whose margin got thin gets one more sweep from the next pass it enqueues.  Returns
 * MVS_W_UNCONVERGED (> 0) when any solve of the call ended above cg_tol.) */
/* stats == NULL after the handle's first (calibrating) call: mvs_deform_iterate only ENQUEUES the passes on the
 * handle's stream and returns — independent handles (e.g. one per body part, each on its own stream) then overlap
 * on the device.  mvs_deform_collect waits for the handle's stream and reads the statistics of the last pass back
 * (and re-plans the solver's launch counts from them, as a synchronous call does). */
int mvs_deform_collect(mvs_deform_t h, const mvs_deform_params* p, mvs_deform_stats* stats);

/* The same body split at its exchange points for view-sharded targets
 * (one process per GPU).  All *_dev buffers are caller-owned
 * HBM (torch tensors) so the collective runs on them directly:
 *   1. _assoc_dmin   : d2min_dev[K] float  <- local 1-NN squared distance  (then all-reduce MIN)
 *   2. _assoc_select : local best <=top_k candidates inside the global ball
 *                      -> records_dev[K*8] (mvs_cand), counts_dev[K*2] int32
 *                      {ball population, survivors of the normal test}     (then all-gather)
 *   3. _assoc_merge  : merge nranks record sets -> node targets + isValid
 *   4. _solve        : graph smoothing + ARAP + geometry update (replicated) */
typedef struct mvs_cand {      /* 48 bytes */
    double  proj_dist;
    double  proj_len;
    double  pos[3];
    int64_t index;             /* global target index, -1 = empty slot */
} mvs_cand;

/* NOTE on _assoc_dmin: from the second pass against the same target on, the search of a node is bounded by the GLOBAL
 * distance _assoc_select was given last time plus the distance the node has moved since (triangle inequality).  A rank
 * none of whose points can be the nearest one then reports some value ABOVE the global minimum instead of its own
 * exact minimum; the MIN over ranks is unaffected.  _assoc_select must therefore always receive the reduced array. */
int mvs_deform_assoc_dmin(mvs_deform_t h, const mvs_deform_params* p, float* d2min_dev);
int mvs_deform_assoc_select(mvs_deform_t h, const mvs_deform_params* p,
                            const float* d2min_dev, mvs_cand* records_dev, int32_t* counts_dev);
int mvs_deform_assoc_merge(mvs_deform_t h, const mvs_deform_params* p,
                           const mvs_cand* records_all_dev, const int32_t* counts_all_dev,
                           int nranks);
/* The same merge over ONE gathered buffer: rank r's block = [K*8 mvs_cand records][K*2 int32 counts], blocks back to back
 * (K*392 bytes each) — what a single all-gather of each rank's packed [records | counts] buffer produces (one collective
 * per outer iteration less than gathering the two arrays separately). */
int mvs_deform_assoc_merge_packed(mvs_deform_t h, const mvs_deform_params* p, const void* packed_all_dev, int nranks);
/* Owner-merges form of step 3 for many ranks.  The all-gather of every rank's records delivers nranks * K * 392 bytes INTO
 * every rank; with an owner per node block an all-to-all moves K * 392 bytes into a rank and the merged targets come back
 * in an all-gather of K * 25 bytes.  Blocks: block_nodes = ceil(K / nranks), rank r owns [r * block_nodes, min(K, (r+1) *
 * block_nodes)).  Rank r receives every rank's records / counts OF ITS BLOCK — rank s's at records_blk_dev + s * (k1-k0) * 8
 * records, counts_blk_dev + s * (k1-k0) * 2 — and merges them into block_dev = [block_nodes * 3 doubles (targets) |
 * block_nodes bytes (valid)]; after the all-gather of the blocks every rank installs all K targets with
 * _set_node_targets_dev (block b at blocks_dev + b * block_stride_bytes) and calls _solve.  Same merge, same total order:
 * the same targets as _assoc_merge, bit for bit (the best-8 index lists stay with the owners: mvs_deform_top_idx gives -1). */
int mvs_deform_assoc_merge_block(mvs_deform_t h, const mvs_deform_params* p, const mvs_cand* records_blk_dev,
                                 const int32_t* counts_blk_dev, int nranks, int64_t k0, int64_t k1, int64_t block_nodes,
                                 void* block_dev);
int mvs_deform_set_node_targets_dev(mvs_deform_t h, const void* blocks_dev, int nblocks, int64_t block_nodes,
                                    int64_t block_stride_bytes);
/* stats == NULL (after the first, calibrating call): enqueue only, no host synchronisation. */
int mvs_deform_solve(mvs_deform_t h, const mvs_deform_params* p, mvs_deform_stats* stats);
int mvs_deform_sync(mvs_deform_t h);            /* wait for the handle's stream */
void* mvs_deform_stream(mvs_deform_t h);        /* hipStream_t of the handle     */
/* Run the handle's kernels on a caller-owned stream (e.g. the stream the caller
 * issues its RCCL collectives on, so that collectives and engine kernels order
 * without host syncs).  NULL restores the handle's own (non-blocking) stream —
 * note that the legacy default stream IS the NULL handle and therefore cannot
 * be selected: create a stream.  The handle's stream is drained first. */
int mvs_deform_set_stream(mvs_deform_t h, void* hip_stream);

/* ---- multi-GPU: one process (or thread) per GPU, RCCL over xGMI (SURVEY.md §8b "Threading", §8e) ----
 * The view-sharded body above, driven from C: every rank holds the target points of its views (mvs_deform_set_target
 * with the global index_base of its first point), the template and the node set are the same everywhere.  RCCL is
 * bound at run time (dlopen): a host that never calls these entries does not need it.
 *   mvs_comm_unique_id : rank 0 makes the 128-byte id and hands it to the other ranks by its own means (file, socket,
 *                        MPI, torch.distributed broadcast ...);
 *   mvs_comm_init      : collective over all ranks; uses the CURRENT HIP device (mvs_set_device / hipSetDevice first);
 *   mvs_deform_iterate_sharded : n_outer passes; per pass one ncclAllReduce(min) of K floats and one ncclAllGather of
 *                        K * 392 bytes per rank, both on the handle's stream (no host synchronisation between engine
 *                        kernels and collectives); merge and solve replicated — the replicas stay bit-identical.
 *                        Statistics / status as mvs_deform_iterate (read back every 32nd pass and at the end). */
#define MVS_COMM_ID_BYTES 128
typedef struct mvs_comm_s* mvs_comm_t;
int mvs_comm_unique_id(uint8_t* id /*MVS_COMM_ID_BYTES*/);
int mvs_comm_init(int rank, int nranks, const uint8_t* id /*MVS_COMM_ID_BYTES*/, mvs_comm_t* out);
int mvs_comm_destroy(mvs_comm_t c);
/* an mvs_reduce_fn over a communicator (ctx = the mvs_comm_t): n <= 24 host doubles, op 0 = sum, 1 = min */
int mvs_comm_reduce(void* comm, double* v, int n, int op);
int mvs_comm_info(mvs_comm_t c, int* rank, int* nranks);
/* How the ranks' best-8 records meet in mvs_deform_iterate_sharded: AUTO = ALL_GATHER at every rank count; OWNER (on request)
 * = every rank receives and merges only the node block it owns (K * 392 bytes into a rank instead of N * K * 392, then one
 * all-gather of 25 bytes per node); the result is the same bits either way.  OWNER has run with one rank only on hardware
 * (the point-to-point step is then a device copy): AUTO does not select it until a multi-GPU run has pinned it. */
enum { MVS_EXCHANGE_AUTO = 0, MVS_EXCHANGE_ALL_GATHER = 1, MVS_EXCHANGE_OWNER = 2 };
int mvs_comm_set_exchange(mvs_comm_t c, int mode);
int mvs_deform_iterate_sharded(mvs_deform_t h, mvs_comm_t c, const mvs_deform_params* p, int n_outer, mvs_deform_stats* stats);

/* ---- groups: several handles on one device stepping in lockstep as ONE sequence of launches ----
 * BASELINE config 5's per-part deformation graphs (R/PartRecognition/PartRecognition.cpp:50-77 labels, one Deformation per
 * part): every part is an ordinary handle — its own sub-mesh, nodes, target, control block and verdicts — but sixteen small
 * launch chains cost sixteen times the launch overhead.  A group launches every kernel of an outer iteration once for all its
 * handles (grid = workgroups x parts); what a part computes is what its handle computes stepping alone — bit for bit as long as
 * every solve stops at the same sweep; the partial sums the stop rules read are grouped differently (a group's local step is a
 * launch of its own), so over hundreds of solves one may stop a sweep apart: a difference at the solve tolerance (cg_tol).
 *   mvs_deform_group_create  : the handles (one device, no duplicates) stay owned by the caller and must outlive the group;
 *   mvs_deform_group_iterate : n_outer outer iterations of every handle, stats[n] per handle (may be NULL).  Returns
 *                              MVS_E_STATE having done nothing when the handles cannot step as a group yet — each must have
 *                              stepped twice on its own (mvs_deform_iterate: the unbounded first passes and the calibration of
 *                              its launch plan) with the overlapping-patch solver, smooth_sweeps = 2, update_normals = 0 —
 *                              mvs_last_error says which condition failed; the caller then steps the handles one by one.
 *                              A handle that stops qualifying DURING a call (between two batches of 32 outer iterations: its
 *                              solves begin to stall, a solve was abandoned) ends the group launches; the rest of the call's
 *                              outer iterations are stepped handle by handle inside the call (same results, more launches). */
typedef struct mvs_group_s* mvs_group_t;
int mvs_deform_group_create(mvs_deform_t* handles, int n, mvs_group_t* out);
int mvs_deform_group_iterate(mvs_group_t g, const mvs_deform_params* p, int n_outer, mvs_deform_stats* stats /*n, or NULL*/);
int mvs_deform_group_destroy(mvs_group_t g);

/* Read-back (host buffers). */
int mvs_deform_get_vertices(mvs_deform_t h, double* pts /*V*3*/);
int mvs_deform_get_normals(mvs_deform_t h, double* normals /*V*3*/);
int mvs_deform_get_rotations(mvs_deform_t h, double* R /*V*9 row-major*/);
/* controls[] / isValid[] after association (+ smoothing if smoothed != 0),
 * Deformation.cpp:262-264,355-356,378-380.  Optional debug outputs:
 * d2min (K float), counts (K*2 int32), top_idx (K*8 int64, -1 padded). */
int mvs_deform_get_node_targets(mvs_deform_t h, int smoothed, double* controls /*K*3*/,
                                uint8_t* valid /*K*/, float* d2min, int32_t* counts,
                                int64_t* top_idx);
int mvs_deform_get_node_graph(mvs_deform_t h, int32_t* nbr /*K*(graph_k+1)*/);
/* exportOBJ's normals (Deformation.h:86-150,174-191) for the current geometry. */
int mvs_deform_compute_normals(mvs_deform_t h, double* normals /*V*3*/);

/* Which global solver mvs_deform_solve would use with `p` (NULL = defaults): kind 0 = CG (one launch per iteration),
 * 1 = overlapping-patch sweeps; for kind 1 the number of patches, the total number of patch-local rows (owned +
 * overlap) and the stored entries per row. */
int mvs_deform_solver_info(mvs_deform_t h, const mvs_deform_params* p, int32_t* kind, int64_t* patches,
                           int64_t* local_rows, int32_t* width);

/* Stand-alone pieces of the body (parity tests / callers that only need one):
 * KNearestNeighbor on arbitrary points (Deformation.cpp:108-153) and the
 * CGAL-equivalent ARAP solve with explicit constraints (Deformation.cpp:383-400). */
int mvs_knn_points(const double* pts, int64_t n, int k, int32_t* out_idx /*n*k*/);
int mvs_deform_arap(mvs_deform_t h, const mvs_deform_params* p,
                    const double* ctrl_targets /*K*3, for the handle's nodes*/,
                    mvs_deform_stats* stats);

/* Kernel timing of the last mvs_deform_iterate / _solve call, measured with
 * hipEvents on the handle's stream (bench.py's roofline object).  names:
 * "assoc", "graph", "smooth", "weights", "rhs", "cg", "local", "finalize". */
int mvs_deform_kernel_time(mvs_deform_t h, const char* name, double* total_ms, int64_t* launches);
/* on: 0 off, 1 every phase, 2 only the "cg" / "tail" groups (two events per global solve), 3 the planned sweeps ("cg") of
 * every eighth pass, with the idle flags those very launches left on the device read back: the `launches` field of "cg_idle"
 * counts the bracketed launches that found their solve already finished, and every bracket is also filed under its
 * composition, "cg:a<active>:i<idle>" (total ms, number of such brackets). */
int mvs_deform_enable_timing(mvs_deform_t h, int on);

#ifdef __cplusplus
}
#endif
#endif /* MVS_H_ */
