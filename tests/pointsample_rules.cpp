// Stand-alone host program for the per-pixel rules of mvs_point_sample (csrc/pointsample_rules.h), the body the kernels of
// pointsample.hip run.  tests/test_pointsample_host.py builds it with -fsanitize=address,undefined and runs it: every raster is a heap
// block of exactly w * h floats, so a read one element outside it ends the program.  With two arguments it runs rules 1-6 on a sequence
// the test wrote (`in`: int32 {n, w, h, r, nbr, step}, double {dsp_min, dsp_max, max_dsp_err, min_conf, edge}, n cameras of 16 doubles
// {fx, fy, cx, cy, R[9], t[3]}, n * w * h floats) and writes `out`: the int32 candidate of every cell, frame by frame, then point and
// normal (6 doubles) of every candidate in that order — what the test compares with tests/ref_pointsample.py.
#include "pointsample_rules.h"
#include <climits>
#include <cmath>
#include <cstdio>
#include <memory>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

constexpr int W = 7, H = 5;                                   // r = 3: cells of 3 + 3 + 1 columns and 3 + 2 rows

static CamDev camera() {                                      // at the origin, looking down +z
    CamDev c = {};
    c.fx = c.fy = 10.0; c.cx = 3.0; c.cy = 2.0;
    c.R[0] = c.R[4] = c.R[8] = 1.0;
    c.w = W; c.h = H;
    return c;
}
static std::unique_ptr<float[]> raster(int frames, float d) {
    std::unique_ptr<float[]> r(new float[(size_t)frames * W * H]);
    for (int i = 0; i < frames * W * H; ++i) r[(size_t)i] = d;
    return r;
}
static PsRules rules(int r, int nbr) { return PsRules{0.0025, 0.75, 0.0, 1.0, 4.0, r, nbr, 1}; }

static int validity_and_normals() {
    CHECK(!ps_valid(NAN, 0.1, 0.5) && !ps_valid(0.0, 0.1, 0.5) && ps_valid(0.1, 0.1, 0.5) && ps_valid(0.5, 0.1, 0.5) && !ps_valid(INFINITY, 0.1, 0.5));
    const CamDev c = camera();
    const PsRules q = rules(3, 0);
    auto ras = raster(1, 0.5f);                                // the plane z = 2
    d3 P, N;
    for (int v = 0; v < H; ++v)                                // every border pixel is dropped, and none reads outside the block
        for (int u = 0; u < W; ++u) {
            const bool border = u == 0 || v == 0 || u == W - 1 || v == H - 1;
            CHECK(ps_point_normal(c, ras.get(), u, v, q, &P, &N) == !border);
        }
    CHECK(ps_point_normal(c, ras.get(), 4, 3, q, &P, &N));
    CHECK(P.x == (4 - 3.0) * 2.0 / 10.0 && P.y == (3 - 2.0) * 2.0 / 10.0 && P.z == 2.0);
    CHECK(N.x == 0.0 && N.y == 0.0 && N.z == -1.0);            // a x b points away from the camera: turned round
    for (float bad : {NAN, 0.0f, 0.8f}) {                      // a NaN, a zero or an out-of-range disparity, in the pixel and in each neighbour
        for (int at : {3 * W + 4, 3 * W + 3, 3 * W + 5, 2 * W + 4}) {
            auto r2 = raster(1, 0.5f);
            r2[(size_t)at] = bad;
            CHECK(!ps_point_normal(c, r2.get(), 4, 3, q, &P, &N));
        }
        auto r2 = raster(1, 0.5f);
        r2[(size_t)(4 * W + 4)] = bad;                         // the neighbour below (4, 3) lies in the last row
        CHECK(!ps_point_normal(c, r2.get(), 4, 3, q, &P, &N));
    }
    auto step = raster(1, 0.5f);                               // a depth step right of (3, 2): |Pr - P| = 2 against 4 * (2 / 10)
    step[(size_t)(2 * W + 4)] = 0.25f;
    CHECK(!ps_point_normal(c, step.get(), 3, 2, q, &P, &N));
    return 0;
}

static int agreement() {
    const CamDev c = camera();
    PsRules q = rules(3, 1);
    auto ras = raster(1, 0.5f);
    int32_t u, v;
    bool in_img;
    CHECK(ps_agrees(world_from_img_hd(c, 4, 3, 2.0), c, ras.get(), q, &u, &v, &in_img) && u == 4 && v == 3 && in_img);   // max_dsp_err = 0: <=
    // u' = W and v' = -1, one past each side: fx x / z + cx + 0.5 = 7.25, fy y / z + cy + 0.5 = -1.5 (truncated toward zero)
    CHECK(!ps_agrees(mk3(0.75, -0.8, 2.0), c, ras.get(), q, &u, &v, &in_img) && u == W && v == -1 && !in_img);
    CHECK(!ps_agrees(mk3(0.75, 0.0, 2.0), c, ras.get(), q, &u, &v, &in_img) && u == W && v == 2 && !in_img);
    CHECK(!ps_agrees(mk3(0.0, -0.8, 2.0), c, ras.get(), q, &u, &v, &in_img) && u == 3 && v == -1 && !in_img);
    // a coordinate in (-1, 0) truncates to 0: the pixel is inside
    CHECK(ps_agrees(mk3(-0.8, -0.58, 2.0), c, ras.get(), q, &u, &v, &in_img) && u == 0 && v == 0 && in_img);
    CHECK(!ps_agrees(mk3(0.2, 0.2, -2.0), c, ras.get(), q, &u, &v, &in_img) && !in_img);                               // behind the camera
    CHECK(!ps_agrees(mk3(0.2, 0.2, 0.0), c, ras.get(), q, &u, &v, &in_img) && !in_img);
    CHECK(!ps_agrees(mk3(NAN, 0.2, 2.0), c, ras.get(), q, &u, &v, &in_img) && !in_img);                               // 0 * NaN: Xc.z is NaN
    img_from_cam(c, mk3(NAN, 0.2, 2.0), &u, &v);
    CHECK(u == INT_MIN && v == 3 && !in_range(u, v, W, H));
    CHECK(!ps_agrees(mk3(0.2, 0.2, 2.5), c, ras.get(), q, &u, &v, &in_img) && in_img);                                 // 0.5 against 1 / 2.5
    q.err = 0.1;
    CHECK(ps_agrees(mk3(0.2, 0.2, 2.5), c, ras.get(), q, &u, &v, &in_img));
    for (float bad : {NAN, 0.0f}) {
        auto r2 = raster(1, 0.5f);
        r2[(size_t)(3 * W + 4)] = bad;
        CHECK(!ps_agrees(world_from_img_hd(c, 4, 3, 2.0), c, r2.get(), q, &u, &v, &in_img) && in_img);
    }
    return 0;
}

static int cells() {
    CHECK(ps_cells(W, 3) == 3 && ps_cells(H, 3) == 2 && ps_cells(6, 3) == 2 && ps_cells(INT_MAX, INT_MAX) == 1 && ps_cells(5, INT_MAX) == 1 &&
          ps_cells(INT_MAX, 1) == INT_MAX);
    const std::unique_ptr<CamDev[]> cams(new CamDev[2]);
    cams[0] = cams[1] = camera();
    const int32_t want[2][3] = {{1 * W + 1, 1 * W + 3, -1}, {3 * W + 1, 3 * W + 3, -1}};   // the partial last column holds border pixels only
    auto one = raster(1, 0.5f);
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 3; ++cx) CHECK(ps_cell_candidate(cams.get(), one.get(), 1, 0, cx, cy, rules(3, 2)) == want[cy][cx]);   // count == 0
    CHECK(ps_cell_candidate(cams.get(), one.get(), 1, 0, 0, 0, rules(INT_MAX, 2)) == 1 * W + 1);                                    // one cell, no overflow
    CHECK(ps_cell_candidate(cams.get(), one.get(), 1, 0, 0, 0, rules(1, 2)) == -1 && ps_cell_candidate(cams.get(), one.get(), 1, 0, 1, 1, rules(1, 2)) == W + 1);
    auto two = raster(2, 0.5f);                                // a second frame that sees the same plane: every neighbour agrees
    for (int f = 0; f < 2; ++f) CHECK(ps_cell_candidate(cams.get(), two.get(), 2, f, 1, 1, rules(3, 1)) == 3 * W + 3);
    for (int i = 0; i < W * H; ++i) two[(size_t)(W * H + i)] = 0.0f;                       // ... that sees nothing: 0 of 1 agree
    CHECK(ps_cell_candidate(cams.get(), two.get(), 2, 0, 1, 1, rules(3, 1)) == -1);
    PsRules lax = rules(3, 1);
    lax.conf = 0.0;
    CHECK(ps_cell_candidate(cams.get(), two.get(), 2, 0, 1, 1, lax) == 3 * W + 3);
    PsRules far = rules(3, 1);
    far.step = INT_MAX;                                        // neighbour frames far outside the sequence: count == 0
    CHECK(ps_cell_candidate(cams.get(), two.get(), 2, 0, 1, 1, far) == 3 * W + 3);
    // nbr_frm_num = INT_MAX on pixels that pass rules 1-3: the neighbour loop is bounded by the sequence, not by the parameter
    auto same = raster(2, 0.5f);
    PsRules all = rules(3, INT_MAX);                           // step 1: the other frame is the one neighbour, and it agrees
    for (int f = 0; f < 2; ++f) CHECK(ps_cell_candidate(cams.get(), same.get(), 2, f, 1, 1, all) == 3 * W + 3);
    CHECK(ps_cell_candidate(cams.get(), two.get(), 2, 0, 1, 1, all) == -1);            // ... and here it sees nothing
    all.step = INT_MAX;                                        // no neighbour inside the sequence: count == 0
    CHECK(ps_cell_candidate(cams.get(), two.get(), 2, 0, 1, 1, all) == 3 * W + 3);
    CHECK(ps_cell_candidate(cams.get(), one.get(), 1, 0, 1, 1, rules(3, INT_MAX)) == 3 * W + 3);      // one frame
    return 0;
}

static int run_file(const char* in, const char* out) {
    FILE* fi = std::fopen(in, "rb");
    CHECK(fi);
    int32_t hd[6];
    double pr[5];
    CHECK(std::fread(hd, sizeof hd, 1, fi) == 1 && std::fread(pr, sizeof pr, 1, fi) == 1);
    const int n = hd[0], w = hd[1], h = hd[2];
    const PsRules q = {pr[0], pr[1], pr[2], pr[3], pr[4], hd[3], hd[4], hd[5]};
    const std::unique_ptr<CamDev[]> cams(new CamDev[(size_t)n]);
    for (int f = 0; f < n; ++f) {
        double c[16];
        CHECK(std::fread(c, sizeof c, 1, fi) == 1);
        CamDev& d = cams[(size_t)f];
        d.fx = c[0]; d.fy = c[1]; d.cx = c[2]; d.cy = c[3];
        for (int i = 0; i < 9; ++i) d.R[i] = c[4 + i];
        for (int i = 0; i < 3; ++i) d.t[i] = c[13 + i];
        d.w = w; d.h = h;
    }
    const size_t nf = (size_t)n * w * h;
    const std::unique_ptr<float[]> ras(new float[nf]);
    CHECK(std::fread(ras.get(), sizeof(float), nf, fi) == nf);
    std::fclose(fi);
    const int cw = ps_cells(w, q.r), ch = ps_cells(h, q.r);
    const size_t nc = (size_t)n * cw * ch;
    const std::unique_ptr<int32_t[]> cand(new int32_t[nc]);
    for (int f = 0; f < n; ++f)
        for (int cy = 0; cy < ch; ++cy)
            for (int cx = 0; cx < cw; ++cx) cand[((size_t)f * ch + cy) * cw + cx] = ps_cell_candidate(cams.get(), ras.get(), n, f, cx, cy, q);
    FILE* fo = std::fopen(out, "wb");
    CHECK(fo && std::fwrite(cand.get(), sizeof(int32_t), nc, fo) == nc);
    for (size_t i = 0; i < nc; ++i) {
        if (cand[i] < 0) continue;
        const int f = (int)(i / ((size_t)cw * ch));
        d3 P, N;
        CHECK(ps_point_normal(cams[(size_t)f], ras.get() + (size_t)f * w * h, cand[i] % w, cand[i] / w, q, &P, &N));
        const double row[6] = {P.x, P.y, P.z, N.x, N.y, N.z};
        CHECK(std::fwrite(row, sizeof row, 1, fo) == 1);
    }
    CHECK(std::fclose(fo) == 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    if (validity_and_normals() || agreement() || cells()) return 1;
    std::printf("pointsample rules ok\n");
    return 0;
}
