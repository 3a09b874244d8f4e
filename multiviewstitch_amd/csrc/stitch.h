// stitch.h — launchers of stitch.hip (the tail of Processor::AlignmentSeq and general-mesh vertex normals); see stitch.hip.
#ifndef MVS_STITCH_H_
#define MVS_STITCH_H_
#include "engine.h"
#include <functional>

// visibility cull of the points of n_seg segments (seg_off: host, n_seg + 1, from 0); mode = enum mvs_cull_mode; the keep mask goes
// to keep_u8 or, when it is not NULL, keep_i32 (device, P entries); n_keep (host, n_seg) receives the kept counts.  Synchronises s.
int vis_cull_dev(const double* pts_dev, const int64_t* seg_off, int n_seg, int n_seq, const double* scales, const double* R,
                 const double* t, const int32_t* cam_off, const mvs_camera* cams, int mode, uint8_t* keep_u8, int32_t* keep_i32,
                 int64_t* n_keep, hipStream_t s);
// compaction of every segment by its int32 keep mask (reference layout, or the kept points only when truncate) followed by the
// forward map of sequence g (s R p + t, R n).  out_off (host, n_seg + 1) receives the output offsets.  Synchronises s.
int stitch_compact_dev(const double* pts, const double* nrm, const int32_t* keep, const int64_t* seg_off, int n_seg, const int64_t* n_keep,
                       int truncate, const double* scales, const double* R, const double* t, double* out_pts, double* out_nrm,
                       int64_t* out_off, hipStream_t s);
// PlyObj vertex normals of a triangle list (device arrays); MVS_E_BAD_MESH for a facet index outside [0, V).  Synchronises s.
int mesh_vertex_normals_dev(const double* pts, int64_t V, const int32_t* faces, int64_t F, double* out, hipStream_t s);
// Poisson model trim on device arrays (align.hip): compaction by keep (int32, V + 1, or NULL: none) with the facet remap, then
// RetainConnectRegion.  V, F in/out.
int cull_retain_dev(double* pts, double* nrm, int64_t* V, int32_t* faces, int64_t* F, const int32_t* keep);
// Model2Depth::Run over every camera of every sequence (render_views.hip), arguments validated by the caller: mesh (device) in the
// world frame, mapped into sequence k's frame by the inverse SRT of k (scales == NULL: not mapped); out (device) = cam_off[n_seq]
// rasters of cams[0].w x cams[0].h floats in camera order.  Views are rendered in chunks of mvs_render_chunk_views().  Synchronises s.
int render_views_dev(const double* pts, int64_t V, const int32_t* faces, int64_t F, int n_seq, const double* scales, const double* R,
                     const double* t, const int32_t* cam_off, const mvs_camera* cams, float znear, float zfar, float* out, hipStream_t s);
// mvs_point_sample's host form (pointsample.hip) with outputs that size themselves: points / normals receive seq_offsets[n_seq] rows.
// Validates like mvs_point_sample, reporting under the name fn.
int point_sample_vectors(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const float* depths,
                         const mvs_point_sample_params* p, int64_t* seq_offsets, std::vector<double>* points, std::vector<double>* normals);
// mvs_refine_depth_maps's host form (depth_refine.hip), validating and reporting under the name fn
int refine_depth_maps_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                           const mvs_depth_refine_params* p, float* out, int8_t* k_out, int32_t* sum_out, uint8_t* cnt_out);
// mvs_recover_depth_maps's host form (depth_recover.hip), validating and reporting under the name fn
int recover_depth_maps_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                            const mvs_depth_recover_params* p, float* out, int16_t* level_out, int32_t* sum_out, uint8_t* cnt_out);
// mvs_recover_depth_maps_aggregated's host form (depth_sgm.hip), validating and reporting under the name fn; ap may be NULL (defaults)
int recover_depth_maps_aggregated_host(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs,
                                       const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* ap, float* out, int16_t* level_out,
                                       int32_t* sum_out, uint8_t* cnt_out, int32_t* agg_out);
// its argument checks alone, but for the NULL tests of imgs and out: no device, no image is needed
int recover_depth_maps_aggregated_check(const char* fn, int32_t n_seq, const int32_t* cam_off, const mvs_camera* cams,
                                        const mvs_depth_recover_params* p, const mvs_depth_aggregate_params* ap);
// mvs_colour_vertices_dev (colour.hip) under the name fn: validates, needs a device, colours; complete on return.  The two checks it
// starts with are there for the file form, which has to fail before it reads a frame
int colour_check_params(const char* fn, const mvs_colour_params* p);
int colour_check_views(const char* fn, int32_t n_seq, const double* scales, const double* R, const double* t, const int32_t* cam_off,
                       const mvs_camera* cams);
int colour_vertices_dev(const char* fn, const double* pts, const double* nrm, int64_t V, int32_t n_seq, const double* scales, const double* R,
                        const double* t, const int32_t* cam_off, const mvs_camera* cams, const uint8_t* imgs, const float* depths,
                        const mvs_colour_params* prm, uint8_t* colours, int32_t* n_views, hipStream_t s);
// mvs_jpeg_decode's host form (jpeg.hip) under the name fn; w / h (may be NULL) receive the size; imgs == NULL: the header walk and the
// checks only, no device needed
int jpeg_decode_host(const char* fn, int32_t n, const int64_t* offsets, const uint8_t* data, uint32_t flags, uint8_t* imgs, int32_t* w, int32_t* h);
// the decoder's dequantise / IDCT and pixel launches on coefficient blocks in HBM (jpeg.hip; mvs_jpeg_roundtrip): n images of layout L,
// image i's blocks at i * n_coef, the quantisers in natural order.  Synchronises s
struct JpegLayout;
int jpeg_coef_to_pixels_dev(int32_t n, const JpegLayout& L, int64_t n_coef, const uint16_t* q_luma, const uint16_t* q_chroma, const int16_t* coef_dev,
                            int rgb, uint8_t* imgs_dev, hipStream_t s);
// mvs_jpeg_encode's host form (jpeg_enc.hip) under the name fn with an output that sizes itself: data receives offsets[n] bytes
int jpeg_encode_host(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs, uint32_t flags, const mvs_jpeg_encode_params* p,
                     int64_t* offsets, std::vector<uint8_t>* data);
// mvs_depth_preview's host form (jpeg_enc.hip) under the name fn
int depth_preview_host(const char* fn, int32_t n, int32_t w, int32_t h, const float* depths, uint8_t* out);
// E1 of mvs_jpeg_encode for images of w x h under the name fn, nothing else (jpeg_enc.hip): no device needed
int jpeg_encode_check(const char* fn, int32_t w, int32_t h, uint32_t flags, const mvs_jpeg_encode_params* p);
// mvs_jpeg_encode_dev under the name fn with an output that sizes itself (jpeg_enc.hip): dout receives a device block of offsets[n] bytes
// that holds the streams.  Complete on return
int jpeg_encode_dev_own(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* imgs_dev, uint32_t flags, const mvs_jpeg_encode_params* p,
                        int64_t* offsets, Scratch* dout, hipStream_t s);
// The overlay pictures as JPEG streams (overlay.hip), validating and reporting under the name fn: the canvases are drawn and encoded in
// batches under the byte budget MVS_OVERLAY_BATCH_BYTES, each batch one draw launch into HBM and one encoder call; sink(first, count, off,
// data) receives the streams of canvases first .. first + count - 1 (host: canvas first + i at data[off[i] .. off[i + 1])) and returns a
// status that ends the call when it is not MVS_OK.  Nothing of a batch reaches the sink when its encode fails.  Arguments as
// mvs_processor_match_overlays / mvs_processor_sift_overlays (n = n_frames * view_count)
using OverlaySink = std::function<int(int32_t first, int32_t count, const int64_t* off, const uint8_t* data)>;
int match_overlay_streams(const char* fn, int32_t n1, int32_t n2, int32_t w, int32_t h, const uint8_t* imgs1, const uint8_t* imgs2, const int64_t* moff,
                          const int32_t* matches, uint32_t flags, uint64_t* rng_state, const mvs_jpeg_encode_params* params, const OverlaySink& sink);
int sift_overlay_streams(const char* fn, int32_t n, int32_t w, int32_t h, const uint8_t* views, const int64_t* koff, const float* keys, uint32_t flags,
                         const mvs_jpeg_encode_params* params, const OverlaySink& sink);
// One call of the Poisson stage (poisson.hip), whichever entry made it: `rules` says which of mvs_poisson_reconstruct (PN_PLAIN),
// _density (PN_DENSITY: dp and dinfo) and _screened (PN_SCREENED: sp and sinfo too) it is; the parts it does not have are NULL.  The
// points are the entry's own, host or device.
enum { PN_PLAIN, PN_DENSITY, PN_SCREENED };
struct PnCall {
    const char* fn;                       // the name errors are reported under
    int rules;
    int64_t n;
    const double *points, *normals;
    const mvs_poisson_params* p;
    mvs_poisson_info* info;
    const mvs_poisson_density_params* dp;
    mvs_poisson_density_info* dinfo;
    const mvs_poisson_screen_params* sp;
    mvs_poisson_screen_info* sinfo;
};
// the device form of the call (points on the device) with outputs that size themselves: vertices / faces and, with rules above
// PN_PLAIN, density (d_v of rule 17 per vertex) are allocated once info holds the counts.  Validates like the public entry; the caller
// has a device.  Default stream.
int poisson_blocks(const PnCall& c, Scratch* vertices, Scratch* density, Scratch* faces);
// A call of mvs_poisson_reconstruct_band or — density set — mvs_poisson_reconstruct_band_density (poisson_band.hip), whichever entry made it
struct BdCall {
    const char* fn;
    int64_t n;
    const double *points, *normals;
    const mvs_poisson_params* p;
    const mvs_poisson_band_params* bp;
    mvs_poisson_info* info;
    mvs_poisson_band_info* binfo;
    const mvs_poisson_density_params* dp = nullptr;      // rules 32-35; the band call has neither
    mvs_poisson_density_info* dinfo = nullptr;
    bool density = false;
    const mvs_poisson_screen_params* sp = nullptr;        // rules 36-41 (mvs_poisson_reconstruct_band_screened); the other two calls have none
    mvs_poisson_screen_info* sinfo = nullptr;
    mvs_poisson_band_screen_info* bsinfo = nullptr;
    bool screen = false;
};
// poisson_blocks for the band calls, the points on the device; density (used when c.density) receives d_v of rule 34 per vertex
int poisson_band_blocks(const BdCall& c, Scratch* vertices, Scratch* density, Scratch* faces);
// mvs_mesh_trim_by_value_dev (mesh_trim.hip, rule 18) with arguments the caller has validated.  Synchronises s.
int mesh_trim_dev(int64_t V, const double* vertices, const double* normals, int64_t F, const int32_t* faces, const double* values, double thr,
                  double* vertices_out, double* normals_out, int32_t* faces_out, int64_t* V_out, int64_t* F_out, hipStream_t s);
#endif
