// render_dev.h — the GL pipeline of Model2Depth (R/Model2Depth/Model2Depth.cpp:58-156, R/Camera/Camera.cpp:6-38) as inlines shared
// by render.hip (one camera per call) and render_views.hip (every view of every sequence in one call).  Both kernels run the
// same expressions on the same values: the vertex stage, the triangle set-up with its rejects and clamped pixel range, the
// per-pixel edge test and depth, and RenderDepth's conversion.  The library is built with -ffp-contract=off.
#ifndef MVS_RENDER_DEV_H_
#define MVS_RENDER_DEV_H_
#include "engine.h"

struct GlCam {                  // everything float32, as the GL pipeline holds it
    float mv[12];               // rows of the modelview (3x4)
    float p00, p11, p02, p12, p22, p23;
    int w, h;                   // viewport (0, 0, w, h): the camera's own size, or the shared window of Model2Depth::Run
    double znear, zfar;         // GetClippingPlane of the float projection matrix
};

inline GlCam make_glcam(const mvs_camera* c, float znear, float zfar) {
    GlCam g;
    for (int r = 0; r < 3; ++r) {
        const float sgn = r == 0 ? 1.0f : -1.0f;                                    // Camera.cpp:10-11
        for (int k = 0; k < 3; ++k) g.mv[4 * r + k] = sgn * (float)c->R[3 * r + k];
        g.mv[4 * r + 3] = sgn * (float)c->t[r];
    }
    const float cx = (float)c->cx, cy = (float)c->cy, fx = (float)c->fx, fy = (float)c->fy;
    float left = cx / fx * znear, top = cy / fy * znear;                            // Camera.cpp:15-26
    const float right = ((float)c->w - cx) / cx * left, bottom0 = ((float)c->h - cy) / cy * top;
    left = -left;
    const float bottom = -bottom0;
    g.p00 = 2 * znear / (right - left); g.p11 = 2 * znear / (top - bottom);         // Camera.cpp:28-38
    g.p02 = (right + left) / (right - left); g.p12 = (top + bottom) / (top - bottom);
    g.p22 = -(zfar + znear) / (zfar - znear); g.p23 = -2 * zfar * znear / (zfar - znear);
    g.w = c->w; g.h = c->h;
    const double m22 = (double)g.p22, m32 = (double)g.p23;                          // Model2Depth.cpp:186-191
    g.znear = m32 / (m22 - 1.0f); g.zfar = m32 / (m22 + 1.0f);
    return g;
}

// window coordinates of one glVertex3f: (x_w, y_w, z_w, w_clip)
__device__ inline float4 rd_window(const GlCam& g, float x, float y, float z) {
    const float xe = ((g.mv[0] * x + g.mv[1] * y) + g.mv[2] * z) + g.mv[3];
    const float ye = ((g.mv[4] * x + g.mv[5] * y) + g.mv[6] * z) + g.mv[7];
    const float ze = ((g.mv[8] * x + g.mv[9] * y) + g.mv[10] * z) + g.mv[11];
    const float xc = g.p00 * xe + g.p02 * ze, yc = g.p11 * ye + g.p12 * ze, zc = g.p22 * ze + g.p23, wc = -ze;
    const float xn = xc / wc, yn = yc / wc, zn = zc / wc;
    return make_float4((xn + 1.0f) * (0.5f * (float)g.w), (yn + 1.0f) * (0.5f * (float)g.h), (zn + 1.0f) * 0.5f, wc);
}

__device__ inline bool top_left(double ex, double ey) {     // edge direction (ex, ey), y up: left edges go down, top edges go left
    return ey < 0.0 || (ey == 0.0 && ex < 0.0);
}

// one triangle in window space, counter-clockwise, with the pixel range whose centres can be inside it
struct RdTri {
    double ax, ay, bx, by, cx, cy, za, zb, zc, area;
    int i0, i1, j0, j1;
    bool tl0, tl1, tl2;
};

// false: the triangle draws nothing (a vertex at or behind the eye plane, zero or NaN area, bounding box off the w x h screen)
__device__ inline bool rd_setup(float4 A, float4 B, float4 C, int w, int h, RdTri& t) {
    if (!(A.w > 0.0f && B.w > 0.0f && C.w > 0.0f)) return false;             // at or behind the eye plane (also NaN)
    double ax = A.x, ay = A.y, bx = B.x, by = B.y, cx = C.x, cy = C.y;
    double za = A.z, zb = B.z, zc = C.z;
    double area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    if (area == 0.0 || !(area == area)) return false;
    if (area < 0.0) {                                                         // make it counter-clockwise (no culling in the reference)
        double s = bx; bx = cx; cx = s; s = by; by = cy; cy = s; s = zb; zb = zc; zc = s;
        area = -area;
    }
    const double minx = fmin(ax, fmin(bx, cx)), maxx = fmax(ax, fmax(bx, cx));
    const double miny = fmin(ay, fmin(by, cy)), maxy = fmax(ay, fmax(by, cy));
    if (!(maxx >= 0.0 && minx <= (double)w && maxy >= 0.0 && miny <= (double)h)) return false;
    // pixel range whose centres can be inside (clamped before the conversion: coordinates may be huge near the eye plane)
    t.i0 = (int)fmax(0.0, floor(fmax(minx, 0.0) - 0.5)); t.i1 = (int)fmin((double)(w - 1), ceil(fmin(maxx, (double)w) - 0.5));
    t.j0 = (int)fmax(0.0, floor(fmax(miny, 0.0) - 0.5)); t.j1 = (int)fmin((double)(h - 1), ceil(fmin(maxy, (double)h) - 0.5));
    t.tl0 = top_left(cx - bx, cy - by); t.tl1 = top_left(ax - cx, ay - cy); t.tl2 = top_left(bx - ax, by - ay);
    t.ax = ax; t.ay = ay; t.bx = bx; t.by = by; t.cx = cx; t.cy = cy; t.za = za; t.zb = zb; t.zc = zc; t.area = area;
    return true;
}

// the bit pattern GL_LEQUAL would store at pixel (i, j), or 0xffffffff when the triangle leaves it alone (centre outside under the
// top-left rule, or window depth outside (0, 1)); positive floats order as their bit patterns, so atomicMin is the depth test
__device__ inline uint32_t rd_pixel(const RdTri& t, int i, int j) {
    const double px = i + 0.5, py = j + 0.5;
    const double e0 = (t.cx - t.bx) * (py - t.by) - (t.cy - t.by) * (px - t.bx);     // weight of A
    const double e1 = (t.ax - t.cx) * (py - t.cy) - (t.ay - t.cy) * (px - t.cx);     // weight of B
    const double e2 = (t.bx - t.ax) * (py - t.ay) - (t.by - t.ay) * (px - t.ax);     // weight of C
    if ((e0 > 0.0 || (e0 == 0.0 && t.tl0)) && (e1 > 0.0 || (e1 == 0.0 && t.tl1)) && (e2 > 0.0 || (e2 == 0.0 && t.tl2))) {
        const float z = (float)(((e0 * t.za + e1 * t.zb) + e2 * t.zc) / t.area);
        if (z > 0.0f && z < 1.0f) return __float_as_uint(z);
    }
    return 0xffffffffu;
}

// RenderDepth (:119-142) for one depth-buffer value: z_b -> z_n -> z_e -> 1/z_e, 0 where nothing was drawn
__device__ inline float rd_convert(float z_b, double znear, double zfar) {
    float r = 0.0f;
    if (!(z_b >= 1 || z_b <= 0)) {
        const float z_n = 2 * z_b - 1.0f;
        const float z_e = (float)(2.0 * znear * zfar / (zfar + znear - z_n * (zfar - znear)));
        if (z_e > 1e-6) r = (float)(1.0 / z_e);                                  // SaveDepth narrows to float32
    }
    return r;
}
#endif
