// render.hip — mesh -> per-camera inverse-depth raster: the z-buffer pass that Model2Depth runs through GLUT/OpenGL
// (R/Model2Depth/Model2Depth.cpp:58-156, R/Camera/Camera.cpp:6-38), as three kernels:
//
//   k_rd_project : the fixed-function vertex stage in float32 — modelview [R|t] with rows 1,2 negated
//                  (GetObjAbsTransformGL), the glFrustum matrix of GetFrustumGL/GetProjectGL, perspective divide,
//                  viewport (0,0,w,h), depth range [0,1]
//   k_rd_raster  : one thread per triangle over its pixel bounding box; pixel centres (i+.5, j+.5), top-left fill
//                  rule on exact edge functions (float32 window coordinates evaluated in double), window-space
//                  linear depth, GL_LEQUAL against a float32 depth buffer = atomicMin on the bit pattern
//   k_rd_convert : RenderDepth (:119-142): rows flipped, z_b -> z_n -> z_e -> 1/z_e with the clipping planes
//                  recovered from the projection matrix as GetClippingPlane does
//
// What OpenGL leaves to the implementation (fill-rule ties, 24-bit depth quantisation, clipping of triangles that
// cross the near plane) is fixed here and in the oracle as stated above; triangles with a vertex at or behind the
// eye plane are dropped.  Parity with a particular GL driver is therefore unpinned by construction; parity with the
// oracle is bit-exact.  The arithmetic of the three stages is render_dev.h, shared with render_views.hip.
#include "engine.h"
#include "trace.h"
#include "dev_common.h"
#include "geom.h"
#include "render_dev.h"
#include <algorithm>

namespace {

constexpr int TPB = 256;

// window coordinates of one vertex: (x_w, y_w, z_w, w_clip)
__global__ void k_rd_project(const double* __restrict__ pts, int64_t V, GlCam g, float4* __restrict__ win) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    win[i] = rd_window(g, (float)pts[3 * i], (float)pts[3 * i + 1], (float)pts[3 * i + 2]);     // glVertex3f
}

__global__ void k_rd_raster(const float4* __restrict__ win, const int32_t* __restrict__ faces, int64_t F, int w, int h,
                            uint32_t* __restrict__ zbuf) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    RdTri t;
    if (!rd_setup(win[faces[3 * f]], win[faces[3 * f + 1]], win[faces[3 * f + 2]], w, h, t)) return;
    for (int j = t.j0; j <= t.j1; ++j)
        for (int i = t.i0; i <= t.i1; ++i) {
            const uint32_t z = rd_pixel(t, i, j);
            if (z != 0xffffffffu) atomicMin(&zbuf[(int64_t)j * w + i], z);
        }
}

__global__ void k_rd_convert(const uint32_t* __restrict__ zbuf, int w, int h, double znear, double zfar, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= w * h) return;
    const int i = idx % w, j = idx / w;
    out[idx] = rd_convert(__uint_as_float(zbuf[(int64_t)(h - j - 1) * w + i]), znear, zfar);     // Model2Depth.cpp:134
}

}  // namespace

extern "C" {

int mvs_render_depth_dev(const double* pts_dev, int64_t V, const int32_t* faces_dev, int64_t F, const mvs_camera* cam, float znear,
                         float zfar, float* out_dev, void* hip_stream) {
    MVS_TRACE();
    if (!pts_dev || V <= 0 || F < 0 || (F && !faces_dev) || !cam || cam->w <= 0 || cam->h <= 0 || !(znear > 0) || !(zfar > znear) ||
        !out_dev || cam->cx == 0.0 || cam->cy == 0.0) { mvs_set_error("mvs_render_depth: bad arguments"); return MVS_E_INVALID_ARG; }
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const GlCam g = make_glcam(cam, znear, zfar);
    const int npx = cam->w * cam->h;
    Scratch win, zb;
    if ((rc = win.alloc(sizeof(float4) * (size_t)V, s)) || (rc = zb.alloc(sizeof(uint32_t) * (size_t)npx, s))) return rc;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)zb.p, 0x3f800000, (size_t)npx, s));           // glClearDepth(1.0f)
    k_rd_project<<<dim3((unsigned)((V + TPB - 1) / TPB)), dim3(TPB), 0, s>>>(pts_dev, V, g, win.as<float4>());
    if (F) k_rd_raster<<<dim3((unsigned)((F + TPB - 1) / TPB)), dim3(TPB), 0, s>>>(win.as<float4>(), faces_dev, F, cam->w, cam->h, zb.as<uint32_t>());
    k_rd_convert<<<dim3((npx + TPB - 1) / TPB), dim3(TPB), 0, s>>>(zb.as<uint32_t>(), cam->w, cam->h, g.znear, g.zfar, out_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

int mvs_render_depth(const double* pts, int64_t V, const int32_t* faces, int64_t F, const mvs_camera* cam, float znear, float zfar,
                     float* out) {
    MVS_TRACE();
    if (!pts || V <= 0 || F < 0 || (F && !faces) || !cam || !out) { mvs_set_error("mvs_render_depth: bad arguments"); return MVS_E_INVALID_ARG; }
    for (int64_t k = 0; k < 3 * F; ++k)
        if (faces[k] < 0 || faces[k] >= V) { mvs_set_error("mvs_render_depth: facet index out of range"); return MVS_E_BAD_MESH; }
    int rc = need_device();
    if (rc) return rc;
    Scratch dp, df, dout;
    const size_t npx = (size_t)std::max(cam->w, 0) * (size_t)std::max(cam->h, 0);
    if ((rc = up(dp, pts, 3 * (size_t)V)) || (rc = up(df, faces, 3 * (size_t)F)) || (rc = dout.alloc(sizeof(float) * npx))) return rc;
    if ((rc = mvs_render_depth_dev(dp.as<double>(), V, df.as<int32_t>(), F, cam, znear, zfar, dout.as<float>(), nullptr))) return rc;
    return down(out, dout, npx);
}

}  // extern "C"

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_render() { return (const void*)k_rd_project; }
