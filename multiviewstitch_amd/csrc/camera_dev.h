// camera_dev.h — Camera's four maps as device inlines (R/Camera/Camera.cpp:40-72), shared by geom.hip, srt.hip, consist.hip,
// matchpairs.hip, views.hip.
// Operation order is the reference's (and the oracle's); the library is built with -ffp-contract=off.
#ifndef MVS_CAMERA_DEV_H_
#define MVS_CAMERA_DEV_H_
#include "dev_common.h"
#include "geom.h"

// THE double -> int conversion of every port of reference code ((int)x, an int parameter, an int initialiser): a finite x with
// |x| < 2^31 truncates toward zero; anything else (NaN, +-inf, out of range) gives INT_MIN, x86 cvttsd2si's answer, which CheckRange
// rejects.  A bare (int)x on the GPU saturates and turns NaN into 0.  A float converts through double (exact).
__host__ __device__ inline int32_t cvt_i32(double x) {
    return (x > -2147483649.0 && x < 2147483648.0) ? (int32_t)x : (int32_t)0x80000000;
}
// GetCamCoordFromImg (:40-44) then GetWorldCoordFromCam (:61-67)
__device__ inline d3 world_from_img(const CamDev& c, int u, int v, double d) {
    const d3 pc = mk3((u - c.cx) * d / c.fx, (v - c.cy) * d / c.fy, d);
    const d3 tmp = mk3(pc.x - c.t[0], pc.y - c.t[1], pc.z - c.t[2]);
    return mulMtv(c.R, tmp);
}
// Image3D::GetPoint of pixel (u, v) from the frame's float32 inverse-depth raster: what k_depth_unproject (geom.hip) writes for
// the pixel, (0,0,0) outside [mn, mx] (Image3D.cpp:98-104); the lift of matchpairs.hip and the key-point cull of views.hip
__device__ inline d3 point_from_raster(const float* __restrict__ dsp, const CamDev& c, int u, int v, double mn, double mx) {
    const double d = (double)dsp[(int64_t)v * c.w + u];
    if (d < mn || d > mx) return mk3(0, 0, 0);
    return world_from_img(c, u, v, 1.0 / d);
}
// GetCamCoordFromWorld (:68-72) then GetImgCoordFromCam (:45-48): C truncation toward zero, no z > 0 test
__device__ inline void img_from_world(const CamDev& c, d3 pw, int32_t* u, int32_t* v) {
    const d3 p = mk3(((c.R[0] * pw.x + c.R[1] * pw.y) + c.R[2] * pw.z) + c.t[0],
                     ((c.R[3] * pw.x + c.R[4] * pw.y) + c.R[5] * pw.z) + c.t[1],
                     ((c.R[6] * pw.x + c.R[7] * pw.y) + c.R[8] * pw.z) + c.t[2]);
    *u = cvt_i32(c.fx * p.x / p.z + c.cx + 0.5);
    *v = cvt_i32(c.fy * p.y / p.z + c.cy + 0.5);
}
// The same maps for bodies that host code shares (pointsample_rules.h), operation for operation those above: GetCamCoordFromWorld
// alone (the camera coordinates img_from_world divides by), GetImgCoordFromCam of a camera point, and world_from_img
__host__ __device__ inline d3 cam_from_world(const CamDev& c, d3 pw) {
    return mk3(((c.R[0] * pw.x + c.R[1] * pw.y) + c.R[2] * pw.z) + c.t[0],
               ((c.R[3] * pw.x + c.R[4] * pw.y) + c.R[5] * pw.z) + c.t[1],
               ((c.R[6] * pw.x + c.R[7] * pw.y) + c.R[8] * pw.z) + c.t[2]);
}
__host__ __device__ inline void img_from_cam(const CamDev& c, d3 p, int32_t* u, int32_t* v) {
    *u = cvt_i32(c.fx * p.x / p.z + c.cx + 0.5);
    *v = cvt_i32(c.fy * p.y / p.z + c.cy + 0.5);
}
__host__ __device__ inline d3 world_from_img_hd(const CamDev& c, int u, int v, double d) {
    const d3 pc = mk3((u - c.cx) * d / c.fx, (v - c.cy) * d / c.fy, d);
    const d3 tmp = mk3(pc.x - c.t[0], pc.y - c.t[1], pc.z - c.t[2]);
    return mulMtv(c.R, tmp);
}
// the point half of the similarity map (geom.hip k_srt_apply, stitch.hip k_vis_cull)
__device__ inline d3 map34_point(const Map34& m, d3 p) {
    const d3 tt = mk3(m.t[0], m.t[1], m.t[2]);
    return m.inverse ? mulMv(m.M, p - tt) : mulMv(m.M, p) + tt;
}
#endif
