// sift_rules.h — the pieces of mvs_sift_detect (include/mvs.h) that are host code or one body for host and device: the octave
// count and sizes, the Gaussian tap tables (every transcendental of rules 1-6 is evaluated here, on the host, in double), and the
// edge test and 3x3 refinement of rule 6.  sift.hip runs them; tests/sift_rules.cpp runs the host side as a program of its own;
// tests/ref_sift.py restates them operation for operation.
#ifndef MVS_SIFT_RULES_H_
#define MVS_SIFT_RULES_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <vector>

constexpr int SIFT_MAX_OCT = 16;          // w, h <= 65535 doubled: at most 13 octaves
constexpr int SIFT_MAX_LEVELS = 8;        // dog_levels <= 5: S + 3 Gaussian levels
constexpr int SIFT_RMAX = 51;             // largest blur radius the tile kernel stages (see sift.hip)

// rule 4: n_oct = max(1, floor(log2(min(W0, H0))) - 3), without a floating-point logarithm
inline int sift_octaves(int W0, int H0) {
    int m = W0 < H0 ? W0 : H0, lg = 0;
    while (m > 1) { m >>= 1; ++lg; }
    return lg - 3 > 1 ? lg - 3 : 1;
}

// rule 3: r = ceil(4 sigma); taps exp(-i^2 / 2 sigma^2), i = -r..r, in double, divided by their sum over ascending i, rounded to
// float32.  A sigma that is not positive and finite gives an empty table.
inline int sift_taps(double sigma, std::vector<float>& taps) {
    taps.clear();
    if (!(sigma > 0.0) || !(sigma < 1e6)) return -1;
    const int r = (int)ceil(4.0 * sigma);
    std::vector<double> t((size_t)(2 * r + 1));
    double sum = 0.0;
    for (int i = -r; i <= r; ++i) {
        t[(size_t)(i + r)] = exp(-((double)i * (double)i) / (2.0 * sigma * sigma));
        sum += t[(size_t)(i + r)];
    }
    taps.resize(t.size());
    for (size_t k = 0; k < t.size(); ++k) taps[k] = (float)(t[k] / sum);
    return r;
}

// rule 4: the blur that makes Gaussian level l of an octave from level l - 1 (l >= 1), or level 0 of the first octave from the
// base image (l == 0); NaN when the base is already smoother than sigma0
inline double sift_level_sigma(int l, int S, double sigma0, double sigma_in, int first_octave) {
    if (l == 0) {
        const double sb = sigma_in * (first_octave < 0 ? 2.0 : 1.0);
        return sqrt(sigma0 * sigma0 - sb * sb);
    }
    const double a = sigma0 * pow(2.0, (double)l / S), b = sigma0 * pow(2.0, (double)(l - 1) / S);
    return sqrt(a * a - b * b);
}

// rule 6 on the 27 DoG values D[s][y][x] around a candidate (centre D[1][1][1]): the edge test, ONE solve of H delta = -g by
// Cramer's rule and the contrast test of the refined value.  Every operation is a float32 + - * / in the order written; the
// library is built with -ffp-contract=off.  -> kept?, delta = (dx, dy, ds), vr = the refined value
struct SiftRefined { float dx, dy, ds, vr; };
__host__ __device__ inline bool sift_refine(const float D[3][3][3], float T, float e, SiftRefined* out) {
    const float v = D[1][1][1];
    const float gx = 0.5f * (D[1][1][2] - D[1][1][0]), gy = 0.5f * (D[1][2][1] - D[1][0][1]), gs = 0.5f * (D[2][1][1] - D[0][1][1]);
    const float dxx = (D[1][1][2] + D[1][1][0]) - 2.0f * v, dyy = (D[1][2][1] + D[1][0][1]) - 2.0f * v, dss = (D[2][1][1] + D[0][1][1]) - 2.0f * v;
    const float dxy = 0.25f * ((D[1][2][2] - D[1][2][0]) - (D[1][0][2] - D[1][0][0]));
    const float dxs = 0.25f * ((D[2][1][2] - D[2][1][0]) - (D[0][1][2] - D[0][1][0]));
    const float dys = 0.25f * ((D[2][2][1] - D[2][0][1]) - (D[0][2][1] - D[0][0][1]));
    const float tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy;
    if (!(det2 > 0.0f) || !((tr * tr) * e < ((e + 1.0f) * (e + 1.0f)) * det2)) return false;
    const float b0 = -gx, b1 = -gy, b2 = -gs;
    const float det = (dxx * (dyy * dss - dys * dys) - dxy * (dxy * dss - dys * dxs)) + dxs * (dxy * dys - dyy * dxs);
    if (!(det != 0.0f)) return false;
    const float dx = ((b0 * (dyy * dss - dys * dys) - dxy * (b1 * dss - dys * b2)) + dxs * (b1 * dys - dyy * b2)) / det;
    const float dy = ((dxx * (b1 * dss - dys * b2) - b0 * (dxy * dss - dys * dxs)) + dxs * (dxy * b2 - b1 * dxs)) / det;
    const float ds = ((dxx * (dyy * b2 - b1 * dys) - dxy * (dxy * b2 - b1 * dxs)) + b0 * (dxy * dys - dyy * dxs)) / det;
    if (!(fabsf(dx) < 1.0f) || !(fabsf(dy) < 1.0f) || !(fabsf(ds) < 1.0f)) return false;
    const float vr = v + 0.5f * ((gx * dx + gy * dy) + gs * ds);
    if (!(fabsf(vr) > T)) return false;
    out->dx = dx; out->dy = dy; out->ds = ds; out->vr = vr;
    return true;
}

#endif
