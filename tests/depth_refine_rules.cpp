// Stand-alone host program for the per-pixel rules of mvs_refine_depth_maps (csrc/depth_refine_rules.h), the body the kernel of
// depth_refine.hip runs.  tests/test_depth_refine_host.py builds it with -fsanitize=address,undefined and runs it: every grey raster is a
// heap block of exactly n * w * h bytes, so a read one element outside it ends the program.  With two arguments it runs rules 1-8 on a
// sequence the test wrote (`in`: int32 {n, w, h, N, refs, K, flags}, double {dsp_min, dsp_max, rel_range, ssd_err}, n cameras of 16
// doubles {fx, fy, cx, cy, R[9], t[3]}, n * w * h * 3 image bytes, n * w * h floats) and writes `out`: per pixel the float of out, then
// the int32 sums, then the int8 k and the uint8 cnt — what the test compares with tests/ref_depth_refine.py.
#include "depth_refine_rules.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

constexpr int W = 16, H = 5;

struct Global {                                               // cur(a, b) from the grey raster itself
    const uint8_t* at;
    int w;
    int operator()(int a, int b) const { return at[a * w + b]; }
};

static CamDev camera(double tx) {                             // looking down +z; tx moves the scene to the right in the image
    CamDev c = {};
    c.fx = c.fy = 10.0; c.cx = 7.5; c.cy = 2.0;
    c.R[0] = c.R[4] = c.R[8] = 1.0;
    c.t[0] = tx;
    c.w = W; c.h = H;
    return c;
}
static int pattern(int x, int v) { return (x * 37 + v * 11) % 251; }

static DrPixel pixel(const CamDev* cams, const uint8_t* grey, int n, int f, int u, int v, float d0, const DrRules& q) {
    const DrPlainSsd<Global> ssd = {{grey + ((size_t)f * H + v) * W + u, W}, grey, W, H, q.N};
    return dr_pixel(cams, n, f, u, v, d0, q, ssd);
}

static int choice_order() {
    CHECK(dr_beats(10, 1, -1, 11, 1, -2) && !dr_beats(11, 1, -1, 10, 1, -2));
    CHECK(dr_beats(10, 2, 0, 11, 2, -1) && dr_beats(10, 1, 0, 21, 2, -3));           // 10 / 1 < 21 / 2
    CHECK(dr_beats(5, 1, 0, 10, 2, -1) && dr_beats(5, 1, 1, 10, 2, -2));             // equal: the smaller |k| wins
    CHECK(!dr_beats(5, 1, 1, 10, 2, -1) && !dr_beats(5, 1, 2, 5, 1, 1));             // equal and |k| == |j|: k < 0 keeps it; larger |k| loses
    CHECK(dr_beats(490000000, 8, 0, 499999999, 7, -1) && !dr_beats(499999999, 7, 0, 490000000, 8, -1));   // 3.43e9 < 4.0e9: the products need 64 bits
    return 0;
}

static int pass_through_and_borders() {
    const std::unique_ptr<CamDev[]> cams(new CamDev[2]);
    cams[0] = camera(0.0); cams[1] = camera(0.0);
    const std::unique_ptr<uint8_t[]> grey(new uint8_t[2 * W * H]);
    for (int f = 0; f < 2; ++f)
        for (int v = 0; v < H; ++v)
            for (int x = 0; x < W; ++x) grey[((size_t)f * H + v) * W + x] = (uint8_t)pattern(x, v);
    const DrRules q = {0.125, 0.5, 0.4, 40.0, 1, 5, 2, 1};
    for (float bad : {NAN, INFINITY, -INFINITY, -0.25f, -0.0f, 0.0f, 0.1249f, 0.5001f}) {
        const DrPixel r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, bad, q);
        CHECK(!r.accepted && r.k == DR_NONE && r.sum == -1 && r.cnt == 0);
    }
    for (int v = 0; v < H; ++v)                                // every border pixel keeps its input, and none reads outside the block
        for (int u = 0; u < W; ++u) {
            const DrPixel r = pixel(cams.get(), grey.get(), 2, 1, u, v, 0.3f, q);
            const bool border = u < 1 || u >= W - 1 || v < 1 || v >= H - 1;
            CHECK(r.accepted == !border);
            // two cameras in one place: every hypothesis lands on the pixel itself, every sum is 0, and the tie goes to k = 0
            if (!border) CHECK(r.k == 0 && r.sum == 0 && r.cnt == 1 && r.d == (double)0.3f);
        }
    DrRules one = q;
    one.refs = 1;                                              // no reference frame at all
    CHECK(!pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.3f, one).accepted);
    CHECK(!pixel(cams.get(), grey.get(), 1, 0, 5, 2, 0.3f, q).accepted);     // a sequence of one frame
    DrRules n0 = q;
    n0.N = 0;                                                  // a window of one pixel reaches the corners
    for (int u : {0, W - 1})
        for (int v : {0, H - 1}) CHECK(pixel(cams.get(), grey.get(), 2, 0, u, v, 0.3f, n0).k == 0);
    // d0 at the bounds: only the hypotheses on one side are live; still k = 0
    const DrPixel lo = pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.125f, q), hi = pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.5f, q);
    CHECK(lo.accepted && lo.k == 0 && lo.d == 0.125 && hi.accepted && hi.k == 0 && hi.d == 0.5);
    return 0;
}

static int shifted_image() {
    // the second camera sees the scene fx * 1.0 * d pixels to the right: u' = int(u + 10 d_k + 0.5).  d0 = 0.3f, step 0.2: d_k =
    // 0.18, 0.24, 0.3, 0.36, 0.42 -> u' - u = 2, 2, 3, 4, 4.  Its image is the first one moved 4 pixels: k = 1 and k = 2 both have sum 0.
    const std::unique_ptr<CamDev[]> cams(new CamDev[2]);
    cams[0] = camera(0.0); cams[1] = camera(1.0);
    const std::unique_ptr<uint8_t[]> grey(new uint8_t[2 * W * H]);
    for (int v = 0; v < H; ++v)
        for (int x = 0; x < W; ++x) {
            grey[(size_t)v * W + x] = (uint8_t)pattern(x, v);
            grey[((size_t)H + v) * W + x] = (uint8_t)(x >= 4 ? pattern(x - 4, v) : 0);
        }
    DrRules q = {0.125, 0.5, 0.4, 40.0, 1, 3, 2, 0};
    const double d0 = (double)0.3f, step = 0.4 / 2.0;
    DrPixel r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.3f, q);
    CHECK(r.accepted && r.k == 1 && r.sum == 0 && r.cnt == 1 && r.d == d0 * (1.0 + 1.0 * step));
    q.flags = 1;                                               // c- > 0 = c0 = c+: den = c-, o = 0.5
    r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.3f, q);
    CHECK(r.accepted && r.k == 1 && r.d == d0 * (1.0 + (1.0 + 0.5) * step));
    q.err = 0.0;                                               // sqrt(0) <= 0: still accepted
    CHECK(pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.3f, q).accepted);
    // u = 11: u' = 13, 13, 14, 15, 15 — only k <= 0 land inside [1, W - 2]; the best of them is not k = 1
    r = pixel(cams.get(), grey.get(), 2, 0, 11, 2, 0.3f, q);
    CHECK(r.cnt == 1 && r.sum > 0 && !r.accepted && r.k == DR_NONE);
    q.err = 1000.0;
    r = pixel(cams.get(), grey.get(), 2, 0, 11, 2, 0.3f, q);
    CHECK(r.accepted && r.k <= 0);
    // u = 13: nothing lands inside: no eligible hypothesis
    r = pixel(cams.get(), grey.get(), 2, 0, 13, 2, 0.3f, q);
    CHECK(!r.accepted && r.sum == -1 && r.cnt == 0);
    // seen from the second frame the first one lies to the left: u' = u - 2 ... u - 4; the match is at the same disparities
    r = pixel(cams.get(), grey.get(), 2, 1, 9, 2, 0.3f, q);
    CHECK(r.accepted && r.k == 1 && r.sum == 0);
    // a camera behind the scene: Xc.z <= 0 never counts
    cams[1].t[2] = -100.0;
    r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, 0.3f, q);
    CHECK(!r.accepted && r.cnt == 0);
    return 0;
}

static int run_file(const char* in, const char* out) {
    FILE* fi = std::fopen(in, "rb");
    CHECK(fi);
    int32_t hd[7];
    double pr[4];
    CHECK(std::fread(hd, sizeof hd, 1, fi) == 1 && std::fread(pr, sizeof pr, 1, fi) == 1);
    const int n = hd[0], w = hd[1], h = hd[2];
    const DrRules q = {pr[0], pr[1], pr[2], pr[3], hd[3], hd[4], hd[5], hd[6]};
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
    const size_t np = (size_t)n * w * h;
    const std::unique_ptr<uint8_t[]> img(new uint8_t[3 * np]), grey(new uint8_t[np]), cnt(new uint8_t[np]);
    const std::unique_ptr<float[]> ras(new float[np]), res(new float[np]);
    const std::unique_ptr<int32_t[]> sum(new int32_t[np]);
    const std::unique_ptr<int8_t[]> kk(new int8_t[np]);
    CHECK(std::fread(img.get(), 3, np, fi) == np && std::fread(ras.get(), sizeof(float), np, fi) == np);
    std::fclose(fi);
    for (size_t i = 0; i < np; ++i) grey[i] = (uint8_t)grey8(img.get() + 3 * i);
    for (int f = 0; f < n; ++f)
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) {
                const size_t i = ((size_t)f * h + v) * w + u;
                const DrPlainSsd<Global> ssd = {{grey.get() + i, w}, grey.get(), w, h, q.N};
                const DrPixel r = dr_pixel(cams.get(), n, f, u, v, ras[i], q, ssd);
                if (r.accepted) res[i] = (float)r.d; else std::memcpy(&res[i], &ras[i], sizeof(float));
                kk[i] = (int8_t)r.k; sum[i] = r.sum; cnt[i] = (uint8_t)r.cnt;
            }
    FILE* fo = std::fopen(out, "wb");
    CHECK(fo && std::fwrite(res.get(), sizeof(float), np, fo) == np && std::fwrite(sum.get(), sizeof(int32_t), np, fo) == np &&
          std::fwrite(kk.get(), 1, np, fo) == np && std::fwrite(cnt.get(), 1, np, fo) == np);
    CHECK(std::fclose(fo) == 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    if (choice_order() || pass_through_and_borders() || shifted_image()) return 1;
    std::printf("depth refine rules ok\n");
    return 0;
}
