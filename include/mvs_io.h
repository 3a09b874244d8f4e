/* mvs_io.h — file formats and the Processor::Deform call sequence around the engine.
 *
 * Host-only C-ABI (no GPU work except mvs_processor_deform, which drives the entries of mvs.h).  Every reader and
 * writer reproduces the reference's text quantisation: coordinates pass through float32 (`sscanf "%f"`,
 * `ofs << (float)x`) and are printed with the C++ stream default of 6 significant digits ("%g").
 * Two-call pattern for readers: call with NULL output arrays to obtain the sizes, then with arrays of that size.
 * All functions return MVS_OK or a negative mvs_status; mvs_last_error() has the text.  Nothing exits the process.
 *
 * `R/` = MultiViewStitch/ in the reference repository.
 */
#ifndef MVS_IO_H
#define MVS_IO_H

#include "mvs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Mesh::ReadObjCore — R/PlyObj/PlyObj.cpp:29-75.  `v x y z` (float32 -> double), `vn x y z` (float32 -> double, then
 * normalised in double), `f a b c` or `f a//na b//nb c//nc` (1-based; only the position indices are kept), `#` and every
 * other line skipped, lines cut at 511 characters.  n_vertices / n_normals / n_faces always receive the counts. */
int mvs_obj_read(const char* path, int64_t* n_vertices, int64_t* n_normals, int64_t* n_faces,
                 double* points /*V*3 or NULL*/, double* normals /*N*3 or NULL*/, int32_t* faces /*F*3 or NULL*/);

/* Mesh::WriteObjCore — R/PlyObj/PlyObj.cpp:77-137.  The 11-line header, then `vn`/`v` pairs when normals are given for
 * every vertex (else `v` only), the "# V vertices, N vertices normals" line, an empty line, `f a//a b//b c//c` (or
 * `f a b c`).  normals may be NULL. */
int mvs_obj_write(const char* path, int64_t n_vertices, const double* points, const double* normals,
                  int64_t n_faces, const int32_t* faces);

/* mvs_obj_write with every `v` line extended to `v x y z r g b`: r, g, b are colour / 255 as float32, printed by the same %g writer —
 * the convention MeshLab and CloudCompare read.  colours holds V * 3 bytes in the channel order `order` (MVS_JPEG_BGR or MVS_JPEG_RGB of
 * include/mvs.h: what mvs_colour_vertices returned for images of that order).  mvs_obj_read ignores what follows the third number of a
 * `v` line, so it reads the geometry of such a file unchanged.  This library's convention; the reference writes no colours. */
int mvs_obj_write_coloured(const char* path, int64_t n_vertices, const double* points, const double* normals /*or NULL*/,
                           const uint8_t* colours, uint32_t order, int64_t n_faces, const int32_t* faces);

/* The colours of a file mvs_obj_write_coloured wrote, in the channel order `order`: colours (n_vertices * 3 bytes) receives, per `v`
 * line and channel, (uint8)((double)c * 255.0 + 0.5) of the float32 c read, clamped to 0 .. 255 — every byte value survives the round
 * trip.  n_vertices must be the file's count of `v` lines (mvs_obj_read gives it), else MVS_E_INVALID_ARG.  A `v` line with fewer than
 * six numbers is MVS_E_IO, naming the line. */
int mvs_obj_read_colours(const char* path, int64_t n_vertices, uint8_t* colours, uint32_t order);

/* oriented point list `x y z nx ny nz` per line — written at R/Processor/Processor.cpp:1033-1040 (doubles, 6 significant
 * digits), read at :958-963 (`ifs >> float`). */
int mvs_npts_read(const char* path, int64_t* n, double* points /*n*3 or NULL*/, double* normals /*n*3 or NULL*/);
int mvs_npts_write(const char* path, int64_t n, const double* points, const double* normals);

/* ./Result/SRT.txt — written at R/Processor/Processor.cpp:855-871 (per sequence: scale, the 3x3 rotation in Eigen's
 * default column-aligned format, the translation as one row), read at :1145-1165 through float32.
 * R is row-major 3x3 per sequence. */
int mvs_srt_txt_read(const char* path, int64_t n_seq, double* scales /*n*/, double* R /*n*9*/, double* t /*n*3*/);
int mvs_srt_txt_write(const char* path, int64_t n_seq, const double* scales, const double* R, const double* t);

/* raw float32 rasters — LoadDepth / SaveDepth, R/Common/Utils.h:166-185 (w*h floats, no header). */
int mvs_depth_raw_read(const char* path, int32_t w, int32_t h, float* raster /*w*h*/);
int mvs_depth_raw_write(const char* path, int64_t n, const double* raster /*n, narrowed to float32*/);

/* PartRecognition::LoadParts — R/PartRecognition/PartRecognition.cpp:7-48.  Lines `Name=i;j;k;...` with the 16 names of
 * enum PART (PartRecognition.h:13-30); labels[v] = part of vertex v, vertices never listed keep 0 (HEAD) as the
 * value-initialised vector does; an index outside [0, n_vertices) is MVS_E_INVALID_ARG (the reference writes out of
 * bounds). */
int mvs_parts_read(const char* path, int64_t n_vertices, int32_t* labels /*n_vertices*/);

/* Processor::Deform — R/Processor/Processor.cpp:1111-1138:
 *   ReadObj(model) ; ReadObj(template) ; viewRay = R^T.col(2) of the first camera ; Alignment::Align ;
 *   Deformation(src, normals, facets).Deform(tgt, tgt_normals, 100, 100) ; exportOBJ(out)
 * with the part labels read from `parts_path` (the reference hard-codes ./Template/part/parts inside Align,
 * R/Alignment/Alignment.cpp:40).  cam_R = row-major rotation of cameras[0][0].  params may be NULL (defaults).
 * stats (optional) receives the statistics of the deformation.  out_obj is written with exportOBJ's normals
 * (normalised sum of unit facet normals, R/Deformation/Deformation.h:86-150). */
int mvs_processor_deform(const char* model_obj, const char* template_obj, const char* parts_path, const double cam_R[9],
                         double dist_thres, const mvs_deform_params* params, const char* out_obj, mvs_deform_stats* stats);

/* The tail of Processor::AlignmentSeq before Poisson (R/Processor/Processor.cpp:952-1040): for each sequence k, read
 * npts_paths[k] (mvs_npts_read: float32 like `ifs >> float`, :958-963), cull it (mvs_visibility_cull, MVS_CULL_SEQUENCES,
 * :966-1004), compact it and map it forward (s_k R_k p + t_k, R_k n, :1021-1027), then write out_dir/PSR%d.obj (points and
 * normals, no facets, :1029-1030) and out_dir/PSR.npts (every sequence in order, :1033-1040).  The reference compacts in place and
 * never resizes (:969-1003, :1022), so by default sequence k writes all P_k points: the kept ones in order, then the originals at
 * [n_keep, P_k) as they were; flags MVS_STITCH_TRUNCATE writes the kept points only.  scales / R / t are the doubles AlignmentSeq
 * holds in memory (mvs_srt_txt_read would pass them through float32, :1145-1165); cam_off / cams as mvs_visibility_cull.
 * n_keep (n_seq, may be NULL) receives the kept counts. */
#define MVS_STITCH_TRUNCATE 1u
int mvs_processor_stitch_points(int32_t n_seq, const char* const* npts_paths, const double* scales, const double* R,
                                const double* t, const int32_t* cam_off, const mvs_camera* cams, uint32_t flags,
                                const char* out_dir, int64_t* n_keep);

/* mvs_srt_refine on files, between mvs_processor_point_sample and mvs_processor_stitch_points: read npts_paths[k] (mvs_npts_read) as
 * sequence k's points and normals and the chain of n_seq entries from srt_in (mvs_srt_txt_read: float32, as the reference reads
 * SRT.txt), refine, and write the chain to srt_out (mvs_srt_txt_write; srt_out may be srt_in) — also when no step was made.  The
 * files are read before a device is needed: a missing or short file is MVS_E_IO naming it.  p may be NULL (the defaults); iters_done
 * and history (optional, iters*2) as mvs_srt_refine.  MVS_E_INVALID_ARG under this entry's name: a NULL path, n_seq < 2, and what
 * mvs_srt_refine refuses. */
int mvs_processor_refine_srt(int32_t n_seq, const char* const* npts_paths, const char* srt_in, const mvs_srt_refine_params* p,
                             const char* srt_out, int32_t* iters_done, double* history);

/* The trim of the Poisson model after GeometryRec (R/Processor/Processor.cpp:1057-1105): ReadObj(model_obj) — normals from the
 * `vn` lines, computed as mvs_mesh_vertex_normals when the file has none (R/PlyObj/PlyObj.cpp:3-16) —, then with all_seq_proj
 * (ParamParser::isAllSeqProj) the cull MVS_CULL_ALL_SEQ and the facet remap (a facet stays iff its three vertices do,
 * :1064-1100), then Alignment::RetainConnectRegion (:1102-1103), then WriteObj(out_obj) (:1104).  V_out / F_out (may be NULL)
 * receive the sizes written.  The SRT and cameras are validated as for mvs_visibility_cull even when all_seq_proj is 0. */
int mvs_processor_cull_model(const char* model_obj, int32_t n_seq, const double* scales, const double* R, const double* t,
                             const int32_t* cam_off, const mvs_camera* cams, int32_t all_seq_proj, const char* out_obj,
                             int64_t* V_out, int64_t* F_out);

/* Processor::Render (R/Processor/Processor.cpp:1140-1192), the second half of `main -a 0`: read srt_txt for n_seq sequences through
 * float32 (mvs_srt_txt_read, :1145-1165) and ReadObj(deform_obj) (:1170; normals from the `vn` lines, or computed as
 * mvs_mesh_vertex_normals when the file has none); for each sequence k map the mesh into k's frame, p' = 1/s_k R_k^T (p - t_k),
 * n' = R_k^T n (:1176-1185, mvs_srt_apply with inverse = 1) and write result_dir/render%d.obj (WriteObj, :1186-1188); then
 * Model2Depth::SetInput + Run (mvs_render_depth_views): each camera i of sequence k writes seq_dirs[k]/DATA/Render/_depth<i>.raw
 * (SaveDepth of RenderDepth's raster, Model2Depth.cpp:119-153; w0 x h0 floats of cams[0]'s size), creating the directories as
 * CreateDir does (a '/' is inserted after seq_dirs[k] when it lacks one).  A sequence without cameras renders nothing; its
 * render%d.obj is still written.  The reference uses znear = 0.01f, zfar = 2000.0f.  Not written: the _depth%d.jpg previews
 * (RenderDepthMap, an image encode).  cam_off / cams as mvs_render_depth_views.  A missing or bad input file is reported before
 * any file is written.  n_views_out (may be NULL) receives cam_off[n_seq]. */
int mvs_processor_render(const char* deform_obj, const char* srt_txt, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams,
                         const char* result_dir, const char* const* seq_dirs, float znear, float zfar, int64_t* n_views_out);

/* DepthOptimizer::RefineAllDepthMaps on files (DepthRecovery/DepthOptimizer.cpp:20-43; the rules: mvs_refine_depth_maps, this library's
 * definition): for each sequence k read seq_dirs[k]/DATA/Render/_depth<i>.raw for its cameras i (mvs_depth_raw_read: what
 * mvs_processor_render wrote), refine all sequences in one call, and write seq_dirs[k]/DATA/Refine/_depth<i>.raw, creating the directory
 * as CreateDir does (a '/' is inserted after seq_dirs[k] when it lacks one).  imgs holds the RGB base images of all cameras back to back
 * in camera order, each h x w x 3 bytes, in memory; mvs_processor_refine_depths_files reads them from the sequence directories.  params may be NULL (defaults).  A missing or short raster is reported before anything is written.  Not
 * written: the _depth<i>.jpg previews; mvs_processor_depth_previews writes them. */
int mvs_processor_refine_depths(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                const uint8_t* imgs, const mvs_depth_refine_params* params);

/* The base images of every sequence from where the reference takes them (R/Processor/Processor.cpp:532): camera i = 0.. of sequence k is
 * seq_dirs[k]%05d.jpg (a '/' is inserted after seq_dirs[k] when it lacks one).  The files are read on up to 16 host threads and decoded by
 * mvs_jpeg_decode (rules J1-J8 of include/mvs.h: this library's definition), all sequences that share a size in one call; flags as there
 * (MVS_JPEG_BGR / MVS_JPEG_RGB).  The decoded size must be the cameras' w x h (MVS_E_INVALID_ARG).  imgs receives all cameras back to
 * back in camera order, each h x w x 3 bytes.  A missing or rejected file is reported before anything is written to imgs. */
int mvs_processor_load_images(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams, uint32_t flags,
                              uint8_t* imgs /*all cameras back to back, host*/);

/* mvs_processor_refine_depths with the RGB frames read by mvs_processor_load_images from the same seq_dirs. */
int mvs_processor_refine_depths_files(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                      const mvs_depth_refine_params* params);

/* mvs_recover_depth_maps on files: the first rasters of every sequence, seq_dirs[k]/DATA/_depth<i>.raw for its cameras i — what
 * Processor::CheckConsistency reads (Processor.cpp:37-38) and no program of the reference writes.  All sequences are recovered in one
 * call and written with mvs_depth_raw_write; the directory is created as CreateDir does (a '/' is inserted after seq_dirs[k] when it
 * lacks one).  imgs holds the RGB base images of all cameras back to back in camera order, each h x w x 3 bytes, in memory.  params may
 * be NULL (defaults).  Nothing is written when the call fails.  Not written: the _depth<i>.jpg previews. */
int mvs_processor_recover_depths(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                 const uint8_t* imgs, const mvs_depth_recover_params* params);
/* mvs_processor_recover_depths with the RGB frames read by mvs_processor_load_images from the same seq_dirs. */
int mvs_processor_recover_depths_files(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                       const mvs_depth_recover_params* params);
/* The two entries above with mvs_recover_depth_maps_aggregated (rules S1-S6 of include/mvs.h) in place of the plain sweep: the same
 * files DATA/_depth<i>.raw.  params and aggregate may each be NULL (defaults).  Nothing is written when the call fails.
 * Every argument check of mvs_recover_depth_maps_aggregated, the budget included, is made before a device is needed and, in the _files
 * form, before a frame is read: MVS_E_INVALID_ARG under the entry's name. */
int mvs_processor_recover_depths_aggregated(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                            const uint8_t* imgs, const mvs_depth_recover_params* params,
                                            const mvs_depth_aggregate_params* aggregate);
int mvs_processor_recover_depths_aggregated_files(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                                                  const mvs_depth_recover_params* params, const mvs_depth_aggregate_params* aggregate);

/* mvs_colour_vertices on files (rules C1-C8 of include/mvs.h: this library's definition; the reference has no such stage): the coloured
 * model of a run.  model_obj (Model.obj, PSR%d.obj, deform.obj) is read as ReadObj reads it, its normals from the `vn` lines or, when it
 * has none, computed as mvs_mesh_vertex_normals; srt_txt is read through float32 as mvs_processor_render reads it; the frames
 * seq_dirs[k]%05d.jpg are loaded and decoded as mvs_processor_load_images does (RGB); the mesh is rendered from every camera with
 * mvs_render_depth_views_dev (znear, zfar as there; cams[0]'s size for every view) and those rasters are the occlusion test C4 — a file
 * without facets (PSR%d.obj) has no rasters and C4 is skipped; then every vertex is coloured and out_obj written with
 * mvs_obj_write_coloured in RGB (normals as read; computed ones are written when the file has facets).  Every camera must have cams[0]'s
 * size.  params may be NULL (defaults).  Any bad input is reported before a file is written.  n_coloured (may be NULL) receives the number
 * of vertices at least one view accepted. */
int mvs_processor_colour_model(const char* model_obj, const char* srt_txt, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams,
                               const char* const* seq_dirs, const mvs_colour_params* params, float znear, float zfar, const char* out_obj,
                               int64_t* n_coloured);

/* cv::imwrite of the generated views (R/Image3D/Image3D.cpp:218-219): view j of frame i of `views` (what mvs_gen_new_views returned:
 * n_frames x view_count x h x w x 3 bytes, host; flags MVS_JPEG_BGR or MVS_JPEG_RGB say their order) goes to <seq_dir>Views/proj<i>_<j>.jpg
 * (a '/' is inserted after seq_dir when it lacks one; the directory is created).  All views are encoded in one mvs_jpeg_encode (rules
 * E1-E9 of include/mvs.h: this library's definition; params NULL: quality 95, 4:2:0, as cv::imwrite), the files written on up to 16 host
 * threads.  Nothing is written when the encode fails. */
int mvs_processor_save_views(const char* seq_dir, int32_t n_frames, int32_t view_count, int32_t w, int32_t h, const uint8_t* views, uint32_t flags,
                             const mvs_jpeg_encode_params* params);

/* RenderDepthMap on files (R/Common/Utils.h:189-217; call sites Processor.cpp:60, Model2Depth.cpp:146, DepthOptimizer.cpp:33): read
 * <seq_dir>DATA/<sub>/_depth<i>.raw for i = 0 .. n - 1 (mvs_depth_raw_read; sub is "CHECK", "Render" or "Refine"), make the grey images
 * (mvs_depth_preview), encode them in one mvs_jpeg_encode (MVS_JPEG_GREY; params NULL: the defaults) and write _depth<i>.jpg beside each
 * raster.  A missing or short raster is reported before anything is written. */
int mvs_processor_depth_previews(const char* seq_dir, const char* sub, int32_t n, int32_t w, int32_t h, const mvs_jpeg_encode_params* params);

/* The match pictures of one sequence pair k (R/Processor/Processor.cpp:767-793): the canvases of mvs_match_overlays (rules O1-O6 of
 * include/mvs.h: this library's definition; arguments as there, host arrays) encoded by mvs_jpeg_encode (rules E1-E9; params NULL:
 * quality 95, 4:2:0, as cv::imwrite) and written to <match_dir>match<k>_<i>_<j>.jpg (a '/' is inserted after match_dir when it lacks
 * one; the directory is created; the reference's is "./Match/").  flags: MVS_JPEG_BGR or MVS_JPEG_RGB, the order of the images; with
 * MVS_JPEG_RGB the colours are written the other way round, so the picture is the same.  The base images are uploaded once; the
 * canvases are worked off in batches under a byte budget (MVS_OVERLAY_BATCH_BYTES in the environment, read at every call; default
 * 512 MiB of canvases: the 256 canvases of 640 x 960 of a 16 x 16 sequence pair are one batch), each batch one draw launch into HBM and
 * one encoder call; only the streams are downloaded, and written on up to 16 host threads.  The generator (rng_state in / out; NULL: a
 * fresh default one, as :768) runs on across the batches: the files do not depend on the budget.  Every argument is checked before a
 * device is looked for and before anything is created; nothing of a batch is written when its encode fails. */
int mvs_processor_match_overlays(const char* match_dir, int32_t k, int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1,
                                 const uint8_t* imgs2, const int64_t* match_offsets, const int32_t* matches, uint32_t flags, uint64_t* rng_state,
                                 const mvs_jpeg_encode_params* params);

/* The SIFT pictures of one sequence (R/FeatureProc/FeatureProc.cpp:67-73 with sub = "Sift"; after the background cull,
 * Processor.cpp:604-615, with sub = "Sift1"): view j of frame i of `views` (n_frames x view_count x h x w x 3 bytes, host; what
 * mvs_gen_new_views returned, or those pixels after mvs_jpeg_roundtrip as the reference reads them back) with the marks of
 * mvs_sift_overlays for list i * view_count + j goes to <seq_dir>Views/<sub>/proj<i>_<j>.jpg.  Batches, budget, params, flags and the
 * order of checks as mvs_processor_match_overlays (the marks are (0,255,0) in either order). */
int mvs_processor_sift_overlays(const char* seq_dir, const char* sub, int32_t n_frames, int32_t view_count, int32_t w, int32_t h,
                                const uint8_t* views, const int64_t* key_offsets, const float* keys, uint32_t flags,
                                const mvs_jpeg_encode_params* params);

/* GeometryRec::RunPointSample on files (R/Processor/Processor.cpp:919-949; the rules: mvs_point_sample, this library's definition):
 * for each sequence k read seq_dirs[k]/DATA/CHECK/_depth<i>.raw for its cameras i (mvs_depth_raw_read: the checked rasters that the file
 * shuffle of :919-931 puts in front of GeoRec), sample all sequences in one call, and write seq_dirs[k]/Rec/PointSample.npts
 * (mvs_npts_write), creating Rec/ as CreateDir does (a '/' is inserted after seq_dirs[k] when it lacks one).  npts_paths (may be NULL, and
 * so may an entry): the file sequence k writes instead.  params may be NULL (defaults).  A missing or short raster is reported before
 * anything is written.  n_points (n_seq, may be NULL) receives the rows written. */
int mvs_processor_point_sample(int32_t n_seq, const char* const* seq_dirs, const int32_t* cam_off, const mvs_camera* cams,
                               const mvs_point_sample_params* params, const char* const* npts_paths, int64_t* n_points);

/* GeometryRec::RunPoisson on files (R/Processor/Processor.cpp:1042-1058; the rules: mvs_poisson_reconstruct, this library's definition):
 * read psr_npts (mvs_npts_read: Result/PSR.npts, what mvs_processor_stitch_points wrote), reconstruct, compute the vertex normals
 * (mvs_mesh_vertex_normals_dev) and write model_obj (mvs_obj_write: `v`, `vn` and `f` lines), the file mvs_processor_cull_model reads.
 * params may be NULL (defaults).  Nothing is written when the reconstruction fails.  V / F (may be NULL) receive the sizes written. */
int mvs_processor_poisson(const char* psr_npts, const mvs_poisson_params* params, const char* model_obj, int64_t* V, int64_t* F);

/* mvs_processor_poisson with the sampling density (rules 14-18 of include/mvs.h: this library's definition, NOT VERIFIED against GeoRec):
 * mvs_poisson_reconstruct_density with dparams (NULL: the defaults, flags = 0: no weighting; set MVS_POISSON_WEIGHT_NORMALS to weight),
 * then, when trim_ratio > 0, mvs_mesh_trim_by_value of the mesh by its vertex density at the threshold trim_ratio * mean_density
 * (trim_ratio <= 0: no trim; NaN: MVS_E_INVALID_ARG).  The vertex normals are computed after the trim, from the trimmed mesh.  With
 * dparams = NULL and trim_ratio = 0 the file holds the bytes mvs_processor_poisson writes.  V / F (may be NULL) receive the sizes
 * written. */
int mvs_processor_poisson_density(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_density_params* dparams,
                                  double trim_ratio, const char* model_obj, int64_t* V, int64_t* F);

/* mvs_processor_poisson_density through mvs_poisson_reconstruct_screened (rules 19-23 of include/mvs.h: this library's definition, NOT
 * VERIFIED against GeoRec): sparams NULL means the defaults (alpha = 4).  With alpha = 0 the file holds the bytes
 * mvs_processor_poisson_density writes for the same dparams and trim_ratio. */
int mvs_processor_poisson_screened(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_density_params* dparams,
                                   const mvs_poisson_screen_params* sparams, double trim_ratio, const char* model_obj, int64_t* V, int64_t* F);

/* mvs_processor_poisson through mvs_poisson_reconstruct_band (rules 24-31 of include/mvs.h: this library's definition, NOT VERIFIED
 * against GeoRec): the way to PsnDptMax 10.  bparams NULL: the defaults (base_depth 8, band 2).  Model.obj carries `vn` lines as that of
 * mvs_processor_poisson does; where the depth stays at or below base_depth the file holds the bytes mvs_processor_poisson writes at that
 * depth.  n_open_edges (may be NULL) receives rule 31's count. */
int mvs_processor_poisson_band(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_band_params* bparams,
                               const char* model_obj, int64_t* V, int64_t* F, int64_t* n_open_edges);

/* mvs_processor_poisson_band through mvs_poisson_reconstruct_band_density (rules 32-35 of include/mvs.h: this library's definition, NOT
 * VERIFIED against GeoRec): the band levels with the sampling density.  bparams and dparams NULL: their defaults (flags = 0: no
 * weighting).  It reconstructs, then, when trim_ratio > 0, trims the mesh by its vertex density at the threshold trim_ratio *
 * mean_density (mvs_mesh_trim_by_value_dev; trim_ratio <= 0: no trim; NaN: MVS_E_INVALID_ARG), then computes the vertex normals of
 * the trimmed mesh, then writes.  n_open_edges (may be NULL) receives rule 31's count on the untrimmed mesh.  With dparams = NULL and
 * trim_ratio = 0 the file holds the bytes mvs_processor_poisson_band writes. */
int mvs_processor_poisson_band_density(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_band_params* bparams,
                                       const mvs_poisson_density_params* dparams, double trim_ratio, const char* model_obj, int64_t* V,
                                       int64_t* F, int64_t* n_open_edges);

/* mvs_processor_poisson_band_density through mvs_poisson_reconstruct_band_screened (rules 36-41 of include/mvs.h: this library's
 * definition, NOT VERIFIED against GeoRec): the band levels with the sampling density and screening on every level.  bparams, dparams
 * and sparams NULL: their defaults (alpha = 4).  Reconstruct, trim by trim_ratio, normals, write, as that call does; with alpha = 0 the
 * file holds the bytes it writes. */
int mvs_processor_poisson_band_screened(const char* psr_npts, const mvs_poisson_params* params, const mvs_poisson_band_params* bparams,
                                        const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams, double trim_ratio,
                                        const char* model_obj, int64_t* V, int64_t* F, int64_t* n_open_edges);

#ifdef __cplusplus
}
#endif
#endif
