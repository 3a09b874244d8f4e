/* mvs_test.h — test hooks of libmvs_hip.so.  NOT part of the drop-in ABI (include/mvs.h): a host of the reference never
 * calls these.  They exist so that tests/ can force paths that timing alone rarely takes and look at tables the library
 * builds on the device.  Every piece of state they set lives in the handle they are given — nothing is process-wide. */
#ifndef MVS_TEST_H_
#define MVS_TEST_H_
#include "mvs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The handle's solver control block (csrc/engine.h, MVS_CTL_*): [0..7] escalation flag, worst rel^2, misses, solves, passes
 * finalized, pending prediction, prediction safety factor; then the ring of the last 32 passes x 8 solves: rel^2 of each solve's
 * result (-1: did not run), and the sweeps it ran (negative: no spare launch was left; a fractional quarter: it stopped on a
 * prediction).  n <= 8 + 2 * 256 + 16 doubles. */
int mvs_test_ctl(mvs_deform_t h, double* out, int n);

/* Cold start: mvs_set_device (or the first entry that needs a device) starts a helper thread that loads the library's code
 * objects and creates the first stream; this waits for it (measurements of the warm / cold first call). */
int mvs_test_preload_wait(void);

/* Tail loop of the patch solver's last launch (csrc/schwarz.hip), for THIS handle:
 *   maxspin  : polls a workgroup waits at the device-wide barrier before it abandons the solve (<= 0: default, 65536);
 *   plan_cap : at most this many launches per global solve, its remaining sweeps run inside the last one (0: no cap);
 *   skip_wg  : the workgroup of every tail launch that never arrives at the barrier, so that the bounded wait of every
 *              other workgroup expires and the solve is abandoned — deterministically (-1: none). */
int mvs_test_tail(mvs_deform_t h, int maxspin, int plan_cap, int skip_wg);

/* Geometry of the handle's target grid: out[0..2] = origin, [3] = cell edge, [4..6] = fine cells per axis, [7] = target points. */
int mvs_test_grid(mvs_deform_t h, double* out /*8*/);

/* mvs_deform_group_iterate re-checks between its batches (32 outer iterations) whether every handle still qualifies for group
 * launches and otherwise finishes the call handle by handle: this makes THIS handle stop qualifying once it has been harvested
 * `after_batches` times inside group calls (0: never). */
int mvs_test_group_leave(mvs_deform_t h, int after_batches);

/* Chebyshev steps every patch ran in the launch of sweep slot `slot` of the handle's last pass (slots are numbered through the
 * pass, solve 0's launches first) -> out[patches].  Equal numbers in every patch = every patch stopped at the same sweep. */
int mvs_test_sweep_steps(mvs_deform_t h, int slot, int32_t* out);

/* The heavy list of the handle's last association: entries, and how many had their coarse nearest-distance walk deferred. */
int mvs_test_heavy_count(mvs_deform_t h, int* n, int* flagged);

/* Tables the device mesh build left (csrc/meshbuild.hip), copied to the host.  what = 0: dims as int64[8] {NP, LS, W,
 * nslices, ne, single_pass, has_patches, total local rows}; 1 slice_off, 2 col, 3 opp0, 4 opp1, 5 vf_ptr, 6 vf, 7 pnloc,
 * 8 pown, 9 pnh, 10 l2g, 11 hl2g, 12 lcol (int16), 13 gent, 14 gcol.  out == NULL: only *bytes. */
int mvs_test_mesh_table(mvs_deform_t h, int what, void* out, int64_t* bytes);

/* mvs_sift_match's scores for one list pair, apart from its thresholds (rules 3 and 4 of mvs_sift_match_lists): best, bestidx and
 * second of every descriptor of list 1 against list 2 (the first min(n1, max_sift) entries of the *12 arrays) and of list 2 against
 * list 1 (min(n2, max_sift) entries of the *21 arrays).  With an empty other list: best = 0, bestidx = -1, second = 0. */
int mvs_test_sift_scores(int64_t n1, const float* descs1, int64_t n2, const float* descs2, int32_t max_sift, int32_t* best12, int32_t* idx12,
                         int32_t* second12, int32_t* best21, int32_t* idx21, int32_t* second21);

/* mvs_sift_detect's Gaussian level `level` (0..S+2) of octave `octave` for ONE image (rules 1-4): out receives ow x oh floats
 * (out_floats = its capacity; too small gives MVS_E_INVALID_ARG with ow, oh set). */
int mvs_test_sift_level(int32_t w, int32_t h, const uint8_t* img, const mvs_sift_params* p, int32_t octave, int32_t level, float* out,
                        int64_t out_floats, int32_t* ow, int32_t* oh);

/* mvs_sift_detect's candidates after rule 6 (the key filter included), before orientation, in the order of rule 9: cand_offsets
 * (n_lists + 1), ci[total][4] = {octave, level, xi, yi}, cf[total][3] = {x, y, s}.  A total above capacity (rows) gives
 * MVS_E_INVALID_ARG after cand_offsets is written. */
int mvs_test_sift_candidates(int32_t n_lists, int32_t w, int32_t h, const uint8_t* imgs, const mvs_sift_params* p, int64_t* cand_offsets,
                             int32_t* ci, float* cf, int64_t capacity);

/* mvs_point_sample's candidate table of rule 6, before coverage (rule 7): cell_offsets (cameras + 1: the cells in front of every
 * camera's frame, camera order) and cand[total] = per cell, row-major over ceil(h / r) x ceil(w / r), the candidate's pixel index or -1.
 * A total above capacity (entries) gives MVS_E_INVALID_ARG after cell_offsets is written. */
int mvs_test_point_sample_candidates(int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths,
                                     const mvs_point_sample_params* p, int64_t* cell_offsets, int32_t* cand, int64_t capacity);

/* mvs_poisson_reconstruct up to rule 9: info (n_vertices and n_faces stay 0), the right-hand side of rule 6 and chi, (2^depth + 1)^3
 * doubles each in node order.  A node count above node_capacity gives MVS_E_INVALID_ARG after info's depth, origin and h are written.
 * MVS_E_SOLVER still hands out the field the cycles reached. */
int mvs_test_poisson_field(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p, mvs_poisson_info* info,
                           double* rhs, double* chi, int64_t node_capacity);

/* mvs_poisson_reconstruct_density up to rule 6: info (depth, origin, h, n_used), dinfo, the int64 node sums of rule 14 ((2^Dd + 1)^3 in
 * node order), rho_p of rule 15 and s_p of rule 16 per row (n each; an unused row holds 0) and the right-hand side of rule 6 ((2^depth +
 * 1)^3 doubles), weighted when dparams sets MVS_POISSON_WEIGHT_NORMALS.  chi (may be NULL: the call stops after rule 6) receives the
 * field of that right-hand side as mvs_test_poisson_field hands it out, and info the iso value, the cycles and the residual.  Node
 * counts above density_node_capacity or node_capacity give MVS_E_INVALID_ARG after info's depth and dinfo's density_depth are written. */
int mvs_test_poisson_density(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                             const mvs_poisson_density_params* dparams, mvs_poisson_info* info, mvs_poisson_density_info* dinfo,
                             int64_t* node_sums, int64_t density_node_capacity, double* rho, double* gain, double* rhs, double* chi,
                             int64_t node_capacity);

/* mvs_poisson_reconstruct_screened up to rule 23's iso value: info, dinfo and sinfo as that call writes them (n_vertices and n_faces stay
 * 0); stencil: the int64 sums of rule 20 on the finest level, dense, [(2^depth + 1)^3][27] in node order and the offset order of rule 20
 * (zero where no point touches; all zero for alpha = 0); f of rule 21 (b for alpha = 0), chi0 and the screened chi (chi0 for alpha = 0),
 * (2^depth + 1)^3 doubles each.  A node count above node_capacity gives MVS_E_INVALID_ARG after info's depth is written.  MVS_E_SOLVER
 * of the screened solve still hands out the field it reached.  diagonal selects the diagonal of the cycle's Jacobi smoother: 0 the public
 * call's 6 + rs_i / 2, 1 the plain 6 + S_{i,0}, 2 the row sum 6 + rs_i — the measurement behind the choice, not a mode of the public call;
 * another value gives MVS_E_INVALID_ARG. */
int mvs_test_poisson_screened(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                              const mvs_poisson_density_params* dparams, const mvs_poisson_screen_params* sparams, mvs_poisson_info* info,
                              mvs_poisson_density_info* dinfo, mvs_poisson_screen_info* sinfo, int64_t* stencil, double* f, double* chi0,
                              double* chi, int64_t node_capacity, int32_t diagonal);

/* mvs_poisson_reconstruct_band up to rule 29 (info with the iso value, binfo; n_vertices, n_faces and n_open_edges stay 0), with band
 * level `level` expanded to the dense layout of its grid, node order [iz][iy][ix], n1 = 2^level + 1: active [(2^level / 4)^3] (1: the
 * block is active), cls [n1^3] (0 no value, 1 fixed, 2 free), b [n1^3] (rule 6 at the free nodes, 0 at the fixed ones) and chi [n1^3];
 * b and chi hold NaN where a node has no value.  For small levels: the expansion runs on the host.  MVS_E_INVALID_ARG: what the call
 * refuses, a NULL array, a level outside base_depth + 1 .. D (after info's depth and binfo's base_depth are written), n1^3 above
 * node_capacity.  MVS_E_SOLVER of that level still hands out what the iterations reached; of a level below it, nothing. */
int mvs_test_poisson_band_level(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                const mvs_poisson_band_params* bparams, mvs_poisson_info* info, mvs_poisson_band_info* binfo, int32_t level,
                                uint8_t* active, uint8_t* cls, double* b, double* chi, int64_t node_capacity);

/* mvs_poisson_reconstruct_band_density up to rule 29: what mvs_test_poisson_band_level takes and hands out — the level's b weighted
 * when dparams sets MVS_POISSON_WEIGHT_NORMALS (rule 33) —, plus dparams and dinfo, and of rule 32 node_sums, the int64 sums of the
 * density grid expanded on the host to the dense layout (2^Dd + 1)^3 in node order (0 at a node without storage), and rho_p and s_p per
 * row (n each; an unused row holds 0) as mvs_test_poisson_density hands them out.  MVS_E_INVALID_ARG as that hook and the call; a
 * node count of the density grid above density_node_capacity after dinfo's density_depth is written. */
int mvs_test_poisson_band_density_level(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                        const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                        mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo, int32_t level,
                                        uint8_t* active, uint8_t* cls, double* b, double* chi, int64_t node_capacity, int64_t* node_sums,
                                        int64_t density_node_capacity, double* rho, double* gain);

/* mvs_poisson_reconstruct_band_screened up to rule 41's iso value: what mvs_test_poisson_band_density_level takes and hands out (b is
 * rule 28's, before T_l rs is taken off; chi the screened field of the level), plus sparams, sinfo and bsinfo and, of rules 38-40 on
 * that level, all expanded on the host to the dense layout n1^3 in node order: stencil [n1^3][27], the int64 sums of rule 38 (0 at a
 * node without a row); f, rule 40's b - T_l rs (NaN at a node without a value, 0 at a fixed node); start, the start values of rule 39
 * (NaN at a node without a value).  With alpha = 0 the stencil is zero, f is b and start what the solve began from.
 * MVS_E_INVALID_ARG as that hook and the call, or a NULL array. */
int mvs_test_poisson_band_screened_level(int64_t n, const double* points, const double* normals, const mvs_poisson_params* p,
                                         const mvs_poisson_band_params* bparams, const mvs_poisson_density_params* dparams,
                                         mvs_poisson_info* info, mvs_poisson_band_info* binfo, mvs_poisson_density_info* dinfo, int32_t level,
                                         uint8_t* active, uint8_t* cls, double* b, double* chi, int64_t node_capacity, int64_t* node_sums,
                                         int64_t density_node_capacity, double* rho, double* gain, const mvs_poisson_screen_params* sparams,
                                         mvs_poisson_screen_info* sinfo, mvs_poisson_band_screen_info* bsinfo, int64_t* stencil, double* f,
                                         double* start);

/* mvs_grabcut_masks (host form) with its steps handed out, N = (w / 2) * (h / 2); every array but mask may be NULL:
 *   S [n] int64 (rule 7) and ncap [n][8][N] int32 (rule 8, the layout of mvs_grid_mincut's cap), once per call;
 *   labels [iters + 1][n][N] uint8 and sums [iters + 1][n][2][5][10] int64 (model 0 = foreground; per component c | s0 s1 s2 | p00 p01
 *   p02 p11 p12 p22): entry 0 the components of rule 4 and their learn, entry i the assign and learn of iteration i;
 *   excess [iters][n][N] int32, half_mask [iters][n][N] uint8 (1 / 0) and rounds [iters] int32 (rounds of the cut): iteration i at i - 1.
 * MVS_E_SOLVER still hands out what the steps before the failed cut produced. */
int mvs_test_grabcut_trace(int32_t n, int32_t w, int32_t h, const uint8_t* imgs, const mvs_grabcut_params* p, uint8_t* mask, int64_t* S,
                           int32_t* ncap, uint8_t* labels, int64_t* sums, int32_t* excess, uint8_t* half_mask, int32_t* rounds);

/* closest_rotation (rule 0) or kabsch_rotation (rule 1) of svd3_dev.h for n row-major 3x3 matrices, one thread each:
 * R [n][9]; U, Vm [n][9] as svd3_dev hands them out (may be NULL).  n == 0 launches nothing. */
int mvs_test_rotations(int64_t n, const double* a, int32_t rule, double* R, double* U, double* Vm);

/* mvs_jpeg_decode_dev with its parts timed (scripts/bench_jpeg.py): ms [5] receives the milliseconds of the header walk (host), of the
 * allocation and upload (host clock, synchronised), and of the three launch sets (HIP events): entropy, inverse DCT, pixels. */
int mvs_test_jpeg_decode_timed(int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs_dev, void* hip_stream,
                               double* ms);

/* mvs_jpeg_encode_dev with its parts timed (scripts/bench_jpeg_encode.py): ms [4] receives the milliseconds of the plan and the header
 * (host) and of the three launch sets (HIP events; the host reads two totals in between and those waits are inside): transform, entropy
 * up to the unstuffed bytes, stuffing and headers. */
int mvs_test_jpeg_encode_timed(int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                               int64_t* offsets, uint8_t* data_dev, int64_t capacity, void* hip_stream, double* ms);

/* mvs_jpeg_encode from quantised coefficients in place of pixels: E1 as that entry, then coef (host, [n][n_coef] int16: component by
 * component, the blocks row-major over the padded plane of whole MCUs, natural order inside a block) is uploaded in place of the
 * transform's output and the rest of the call runs unchanged: bit counts, scans, restart intervals, the bit writer, FF count, offsets,
 * stuffing, markers, headers.  For the entropy coder on contents no pixels produce (tests/jpeg_coef_cases.py).  What stands at a dummy
 * block (E6) is never read.  Of flags only MVS_JPEG_GREY matters.  MVS_E_INVALID_ARG before any upload, with the index in the message: a
 * DC of a real block outside -1024 .. 1023 (so that every difference fits category 11) or an AC outside -1023 .. 1023; E7 has no code for
 * more.  offsets, data and capacity as mvs_jpeg_encode. */
int mvs_test_jpeg_encode_coef(int32_t n, int32_t w, int32_t h, const int16_t* coef, uint32_t flags, const mvs_jpeg_encode_params* p,
                              int64_t* offsets, uint8_t* data, int64_t capacity);

/* mvs_match_overlays_dev with its parts timed (scripts/bench_overlay.py): ms [2] receives the milliseconds of building the lists (host)
 * and of the draw launch alone (HIP events around it; the upload of the lists is in front of the first). */
int mvs_test_match_overlays_timed(int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1_dev, const uint8_t* imgs2_dev,
                                  const int64_t* match_offsets, const int32_t* matches, uint64_t* rng_state, uint8_t* out_dev, void* hip_stream,
                                  double* ms);

/* ONE search-and-sum launch of mvs_srt_refine for the given chain, and nothing else: host arrays and argument checks as that entry
 * (the chain is only read); sums [n_seq*n_seq*121] int64 receives the sums of I6, slot a*n_seq+b, in the order count | J_i J_j, i <= j,
 * row by row | J_i r | r r; c_D [4] (may be NULL) the c and D of I2. */
int mvs_test_srt_refine_sums(const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq, const double* scales,
                             const double* R, const double* t, const mvs_srt_refine_params* p, int64_t* sums, double* c_D);
/* ... with the reduction of the 121 sums chosen (form 0: a butterfly per term over the wave, what the entry runs; 1: LDS atomics of
 * every accepted lane) and, when ms is given, `reps` further launches of that form timed by HIP events around them: ms [3] receives
 * the milliseconds of one launch, of one host solve of I7 on the sums (every sequence but the fixed one free; -1 when it fails) and of
 * the set-up in front of the first search (I2 and the grids, host clock, synchronised) (scripts/bench_srt_refine.py). */
int mvs_test_srt_refine_timed(const double* points, const double* normals, const int64_t* seg_off, int32_t n_seq, const double* scales,
                              const double* R, const double* t, const mvs_srt_refine_params* p, int64_t* sums, double* c_D, int32_t form,
                              int32_t reps, double* ms);

#ifdef __cplusplus
}
#endif
#endif
