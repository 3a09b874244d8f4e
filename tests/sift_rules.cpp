// Stand-alone host program for the host rules of mvs_sift_detect (csrc/sift_rules.h): the octave count, the Gaussian tap tables, the
// level sigmas and sift_refine's host side.  tests/test_sift_host.py builds it with -fsanitize=address,undefined and runs it: every
// table is a heap block of exactly its size, so a read or write one element outside it ends the program.
#include "sift_rules.h"
#include <cmath>
#include <cstdio>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int octave_counts() {
    CHECK(sift_octaves(8, 8) == 1 && sift_octaves(15, 400) == 1 && sift_octaves(16, 16) == 1 && sift_octaves(31, 99) == 1);
    CHECK(sift_octaves(32, 32) == 2 && sift_octaves(40, 24) == 1 && sift_octaves(128, 96) == 3 && sift_octaves(1280, 960) == 6);
    CHECK(sift_octaves(131070, 131070) == 13 && sift_octaves(131070, 131070) <= SIFT_MAX_OCT);
    for (int w = 8; w < 3000; ++w) {                          // the smallest octave keeps at least 8 pixels a side
        int m = w;
        for (int o = 1; o < sift_octaves(w, 70000); ++o) m /= 2;
        CHECK(m >= 8);
    }
    return 0;
}

static int tap_tables() {
    std::vector<float> t;
    CHECK(sift_taps(0.0, t) == -1 && t.empty());
    CHECK(sift_taps(-1.0, t) == -1 && sift_taps(NAN, t) == -1 && sift_taps(INFINITY, t) == -1);
    for (double sigma : {0.05, 0.25, 1.0, 1.2262735, 3.0927, 11.085, 12.75}) {
        const int r = sift_taps(sigma, t);
        CHECK(r == (int)ceil(4.0 * sigma) && (int)t.size() == 2 * r + 1);
        double sum = 0.0;
        for (int i = 0; i <= 2 * r; ++i) {
            CHECK(t[(size_t)i] == t[(size_t)(2 * r - i)] && t[(size_t)i] >= 0.0f);
            if (i < r) CHECK(t[(size_t)i] <= t[(size_t)i + 1]);
            sum += t[(size_t)i];
        }
        CHECK(fabs(sum - 1.0) < 1e-6);
    }
    // the default parameters: S + 3 levels, all radii inside the tile kernel's limit; S = 1 is the widest blur of the defaults
    for (int S = 1; S <= 5; ++S)
        for (int fo = -1; fo <= 0; ++fo)
            for (int l = 0; l < S + 3; ++l) {
                const double s = sift_level_sigma(l, S, 1.6f, 0.5f, fo);
                CHECK(s > 0.0 && sift_taps(s, t) >= 1 && sift_taps(s, t) <= SIFT_RMAX);
            }
    CHECK(std::isnan(sift_level_sigma(0, 3, 0.9f, 0.5f, -1)));          // sigma0 below the doubled input blur
    return 0;
}

static int refinement() {
    // a separable quadratic bump with its top at (0.25, -0.125, 0.375) from the centre sample
    float D[3][3][3];
    for (int s = 0; s < 3; ++s)
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) {
                const float fx = (float)(x - 1) - 0.25f, fy = (float)(y - 1) + 0.125f, fs = (float)(s - 1) - 0.375f;
                D[s][y][x] = 0.5f - 0.0625f * (fx * fx + fy * fy + fs * fs);
            }
    SiftRefined r;
    CHECK(sift_refine(D, 0.02f / 3.0f, 10.0f, &r));
    CHECK(fabsf(r.dx - 0.25f) < 1e-5f && fabsf(r.dy + 0.125f) < 1e-5f && fabsf(r.ds - 0.375f) < 1e-5f && fabsf(r.vr - 0.5f) < 1e-5f);
    CHECK(!sift_refine(D, 0.6f, 10.0f, &r));                  // contrast
    float E[3][3][3];
    for (int s = 0; s < 3; ++s)
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 3; ++x) E[s][y][x] = 0.5f - 0.0625f * (float)((x - 1) * (x - 1)) - 0.001f * (float)((y - 1) * (y - 1) + (s - 1) * (s - 1));
    CHECK(!sift_refine(E, 0.001f, 10.0f, &r));                // an edge: curvature ratio 62
    float Z[3][3][3] = {};
    CHECK(!sift_refine(Z, 0.0f, 10.0f, &r));                  // flat: det2 = 0
    float N[3][3][3];
    for (auto& a : N) for (auto& b : a) for (float& c : b) c = NAN;
    CHECK(!sift_refine(N, 0.0f, 10.0f, &r));
    return 0;
}

int main() {
    if (octave_counts() || tap_tables() || refinement()) return 1;
    std::printf("sift rules ok\n");
    return 0;
}
