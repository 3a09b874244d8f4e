// pointsample_rules.h — the per-pixel rules of mvs_point_sample (include/mvs.h): validity (1), the four neighbours (2), the edge test
// and the normal (3), the agreement of a point with another frame (4), the confidence over the neighbour frames (5) and the candidate
// of a cell (6).  One body for the kernels of pointsample.hip and for host code: tests/pointsample_rules.cpp runs it as a program of
// its own, tests/ref_pointsample.py restates it operation for operation.  Every operation is an fp64 + - * / sqrt in the order
// written; the library is built with -ffp-contract=off.
#ifndef MVS_POINTSAMPLE_RULES_H_
#define MVS_POINTSAMPLE_RULES_H_
#include "camera_dev.h"
#include "frontend_dev.h"

struct PsRules {                       // mvs_point_sample_params without its padding
    double mn, mx, err, conf, edge;
    int32_t r, nbr, step;
};

// rule 1 (a NaN is not valid)
__host__ __device__ inline bool ps_valid(double d, double mn, double mx) { return d >= mn && d <= mx; }

// rule 4: does the point P agree with frame g (camera c, raster ras of c.w x c.h)?  (*u, *v) receive the pixel P lands on whenever
// Xc.z > 0 — in range or not —, *in_img whether that pixel is inside the raster
__host__ __device__ inline bool ps_agrees(d3 P, const CamDev& c, const float* __restrict__ ras, const PsRules& q, int32_t* u, int32_t* v,
                                          bool* in_img) {
    *in_img = false;
    const d3 xc = cam_from_world(c, P);
    if (!(xc.z > 0.0)) return false;
    img_from_cam(c, xc, u, v);
    if (!in_range(*u, *v, c.w, c.h)) return false;
    *in_img = true;
    const double dg = (double)ras[(int64_t)*v * c.w + *u];
    if (!ps_valid(dg, q.mn, q.mx)) return false;
    return fabs(dg - 1.0 / xc.z) <= q.err;
}

// rules 1-3 for pixel (u, v) of a frame: its point and its unit normal, turned towards the camera; false when a rule drops the pixel
__host__ __device__ inline bool ps_point_normal(const CamDev& c, const float* __restrict__ ras, int u, int v, const PsRules& q, d3* P, d3* N) {
    if (!(u >= 1 && u <= c.w - 2 && v >= 1 && v <= c.h - 2)) return false;                       // rule 2, asked first: no read outside
    const int64_t i = (int64_t)v * c.w + u;
    const double d = (double)ras[i], dl = (double)ras[i - 1], dr = (double)ras[i + 1], du = (double)ras[i - c.w], dd = (double)ras[i + c.w];
    if (!ps_valid(d, q.mn, q.mx)) return false;                                                  // rule 1
    if (!ps_valid(dl, q.mn, q.mx) || !ps_valid(dr, q.mn, q.mx) || !ps_valid(du, q.mn, q.mx) || !ps_valid(dd, q.mn, q.mx)) return false;
    const double z0 = 1.0 / d;
    const d3 p = world_from_img_hd(c, u, v, z0);
    const d3 pl = world_from_img_hd(c, u - 1, v, 1.0 / dl), pr = world_from_img_hd(c, u + 1, v, 1.0 / dr);
    const d3 pu = world_from_img_hd(c, u, v - 1, 1.0 / du), pd = world_from_img_hd(c, u, v + 1, 1.0 / dd);
    const double lim_x = q.edge * (z0 / fabs(c.fx)), lim_y = q.edge * (z0 / fabs(c.fy));        // rule 3
    if (norm3(pl - p) > lim_x || norm3(pr - p) > lim_x || norm3(pu - p) > lim_y || norm3(pd - p) > lim_y) return false;
    d3 n = cross3(pr - pl, pd - pu);
    const double len = norm3(n);
    if (!(len > 0.0)) return false;
    n = n / len;
    const d3 centre = world_from_img_hd(c, 0, 0, 0.0);
    if (dot3(n, p - centre) > 0.0) n = mk3(-n.x, -n.y, -n.z);
    *P = p;
    *N = n;
    return true;
}

// rules 1-3 and 5 for pixel (u, v) of frame f of a sequence of n frames (cameras cams[n], rasters ras back to back, all of one size)
__host__ __device__ inline bool ps_pixel_passes(const CamDev* __restrict__ cams, const float* __restrict__ ras, int n, int f, int u, int v,
                                                const PsRules& q, d3* P, d3* N) {
    const CamDev& c = cams[f];
    const int64_t npx = (int64_t)c.w * c.h;
    if (!ps_point_normal(c, ras + f * npx, u, v, q, P, N)) return false;
    // N(f) lies inside the sequence: no j above (n - 1) / step can give a frame, whatever nbr_frm_num is
    const int jmax = q.nbr < (n - 1) / q.step ? q.nbr : (n - 1) / q.step;
    int count = 0, agree = 0;
    for (int j = 1; j <= jmax; ++j)
        for (int side = -1; side <= 1; side += 2) {
            const int g = f + side * j * q.step;                         // j * step <= n - 1
            if (g < 0 || g >= n) continue;
            int32_t gu, gv;
            bool in_img;
            ++count;
            if (ps_agrees(*P, cams[g], ras + g * npx, q, &gu, &gv, &in_img)) ++agree;
        }
    return count == 0 || (double)agree >= q.conf * (double)count;
}

// rule 6: the candidate of cell (cx, cy) of frame f: the passing pixel of lowest row-major index, or -1
__host__ __device__ inline int32_t ps_cell_candidate(const CamDev* __restrict__ cams, const float* __restrict__ ras, int n, int f, int cx, int cy,
                                                     const PsRules& q) {
    const int w = cams[f].w, h = cams[f].h;
    const int64_t u1 = (int64_t)(cx + 1) * q.r, v1 = (int64_t)(cy + 1) * q.r;                    // r may be as large as INT32_MAX
    const int ue = u1 < w ? (int)u1 : w, ve = v1 < h ? (int)v1 : h;
    d3 P, N;
    for (int v = cy * q.r; v < ve; ++v)
        for (int u = cx * q.r; u < ue; ++u)
            if (ps_pixel_passes(cams, ras, n, f, u, v, q, &P, &N)) return v * w + u;
    return -1;
}

// cells per row / column of a w x h raster cut into r x r cells (partial cells at the right and bottom)
__host__ __device__ inline int ps_cells(int extent, int r) { return (int)(((int64_t)extent + r - 1) / r); }

#endif
