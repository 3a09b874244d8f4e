// Stand-alone host program for the per-pixel rules of mvs_recover_depth_maps (csrc/depth_recover_rules.h), the body the kernel of
// depth_recover.hip runs.  tests/test_depth_recover_host.py builds it with -fsanitize=address,undefined and runs it: every grey raster is
// a heap block of exactly n * w * h bytes, so a read one element outside it ends the program.  With two arguments it runs R1-R9 on a
// sequence the test wrote (`in`: int32 {n, w, h, N, refs, L, min_refs, flags}, double {dsp_min, dsp_max, ssd_err, peak}, n cameras of 16
// doubles {fx, fy, cx, cy, R[9], t[3]}, n * w * h * 3 image bytes) and writes `out`: per pixel the float of out, then the int32 sums,
// then the int16 levels and the uint8 cnt — what the test compares with tests/ref_depth_recover.py.
#include "depth_recover_rules.h"
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

struct Table {                                                // a cost curve by landing column, whatever the images hold
    const int32_t* by_u;
    int32_t operator()(int, int u2, int) const { return by_u[u2]; }
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
static uint32_t bits_of(float x) { uint32_t b; std::memcpy(&b, &x, sizeof b); return b; }

static RcPixel pixel(const CamDev* cams, const uint8_t* grey, int n, int f, int u, int v, const RcRules& q) {
    const DrPlainSsd<Global> ssd = {{grey + ((size_t)f * H + v) * W + u, W}, grey, W, H, q.N};
    return rc_pixel(cams, n, f, u, v, q, ssd);
}

static int order_and_value() {
    CHECK(rc_less(10, 1, 11, 1) && !rc_less(11, 1, 10, 1) && rc_less(10, 1, 21, 2));
    CHECK(!rc_less(5, 1, 10, 2) && !rc_less(10, 2, 5, 1) && !rc_less(0, 3, 0, 1));     // equal means: neither is less, the earlier level stays
    CHECK(rc_less(490000000, 8, 499999999, 7) && !rc_less(499999999, 7, 490000000, 8));   // 3.43e9 < 4.0e9: the products need 64 bits
    // R9 at both ends of the default range: (float)0.0025 lies below 0.0025 and (float)0.3 above 0.3
    const double mn = 0.0025, mx = 0.3;
    CHECK((double)(float)mn < mn && (double)(float)mx > mx);
    const float lo = rc_value(mn, mn, mx), hi = rc_value(mx, mn, mx);
    CHECK(lo == std::nextafterf((float)mn, 1.0f) && (double)lo >= mn && hi == std::nextafterf((float)mx, 0.0f) && (double)hi <= mx);
    CHECK(rc_value(0.1, mn, mx) == 0.1f && rc_value(0.125, 0.125, 0.375) == 0.125f && rc_value(0.375, 0.125, 0.375) == 0.375f);
    CHECK(rc_level(mn, mx, 0, 128, (mx - mn) / 127.0) == mn && rc_level(mn, mx, 127, 128, (mx - mn) / 127.0) == mx);
    return 0;
}

static int shifted_image() {
    // the second camera sees the scene fx * 1.0 * d pixels to the right: u' = int(u + 10 d_l + 0.5).  Its image is the first one moved 4
    // pixels.
    const std::unique_ptr<CamDev[]> cams(new CamDev[2]);
    cams[0] = camera(0.0); cams[1] = camera(1.0);
    const std::unique_ptr<uint8_t[]> grey(new uint8_t[2 * W * H]);
    for (int v = 0; v < H; ++v)
        for (int x = 0; x < W; ++x) {
            grey[(size_t)v * W + x] = (uint8_t)pattern(x, v);
            grey[((size_t)H + v) * W + x] = (uint8_t)(x >= 4 ? pattern(x - 4, v) : 0);
        }
    // L = 2 over [0.2, 0.4]: u' - u = 2 and 4.  Level 1 matches; d = dsp_max exactly, and (float)0.4 > 0.4 is moved one float32 down
    RcRules q = {0.2, 0.4, 40.0, 0.9, 1, 3, 2, 1, 1};
    RcPixel r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, q);
    CHECK(r.level == 1 && r.sum == 0 && r.cnt == 1 && (double)(float)0.4 > 0.4 && r.out == std::nextafterf(0.4f, 0.0f) && (double)r.out <= 0.4);
    q.err = 0.0;                                               // sqrt(0) <= 0: still accepted
    CHECK(pixel(cams.get(), grey.get(), 2, 0, 5, 2, q).level == 1);
    q.err = 40.0;
    q.min_refs = 2;                                            // one reference cannot make a level eligible
    r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, q);
    CHECK(r.level == RC_NONE && r.sum == -1 && r.cnt == 0 && bits_of(r.out) == 0);
    q.min_refs = 1;
    // u = 12: u' = 14 is the last interior column, u' = 16 is outside: one eligible level is its own worst, rejected; the winner is reported
    r = pixel(cams.get(), grey.get(), 2, 0, 12, 2, q);
    CHECK(r.level == RC_NONE && r.cnt == 1 && r.sum > 0 && bits_of(r.out) == 0);
    q.err = 1e6; q.peak = 1.0;                                 // not even under the widest parameters
    CHECK(pixel(cams.get(), grey.get(), 2, 0, 12, 2, q).level == RC_NONE);
    q.err = 40.0; q.peak = 0.9;
    // u = 13: u' = 15 = W - N lies one past the interior, u' = 17 outside the image: nothing is eligible, nothing outside the block is read
    r = pixel(cams.get(), grey.get(), 2, 0, 13, 2, q);
    CHECK(r.level == RC_NONE && r.sum == -1 && r.cnt == 0 && bits_of(r.out) == 0);
    // seen from the second frame the first one lies to the left: u' = u - 2 and u - 4
    r = pixel(cams.get(), grey.get(), 2, 1, 9, 2, q);
    CHECK(r.level == 1 && r.sum == 0);
    r = pixel(cams.get(), grey.get(), 2, 1, 4, 2, q);           // u' = 2 and 0: level 1 lands one before the interior
    CHECK(r.level == RC_NONE && r.cnt == 1);
    // L = 5 over [0.18, 0.42]: u' - u = 2, 2, 3, 4, 4.  Levels 3 and 4 land on the match, both with sum 0: the lower one wins.  Its
    // neighbours: c- > 0 = c0 = c+, so den = c-, o = 0.5
    RcRules q5 = {0.18, 0.42, 40.0, 0.9, 1, 3, 5, 1, 0};
    const double step = (0.42 - 0.18) / 4.0;
    r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, q5);
    CHECK(r.level == 3 && r.sum == 0 && r.cnt == 1 && r.out == (float)(0.18 + 3.0 * step));
    q5.flags = 1;
    r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, q5);
    CHECK(r.level == 3 && r.out == (float)(0.18 + (3.0 + 0.5) * step));
    for (int v = 0; v < H; ++v)                                // every border pixel is no candidate, and none reads outside the block
        for (int u = 0; u < W; ++u) {
            r = pixel(cams.get(), grey.get(), 2, 0, u, v, q5);
            if (u < 1 || u >= W - 1 || v < 1 || v >= H - 1) CHECK(r.level == RC_NONE && r.sum == -1 && r.cnt == 0 && bits_of(r.out) == 0);
        }
    RcRules n0 = q5;
    n0.N = 0;                                                  // a window of one pixel reaches the corners
    for (int v : {0, H - 1}) CHECK(pixel(cams.get(), grey.get(), 2, 0, 0, v, n0).cnt == 1);
    CHECK(pixel(cams.get(), grey.get(), 2, 0, W - 1, 0, n0).cnt == 0);        // every level leaves the image to the right
    CHECK(pixel(cams.get(), grey.get(), 1, 0, 5, 2, q5).cnt == 0);            // a sequence of one frame
    RcRules one = q5;
    one.refs = 1;                                              // no reference frame at all
    CHECK(pixel(cams.get(), grey.get(), 2, 0, 5, 2, one).cnt == 0);
    cams[1].t[2] = -100.0;                                     // a camera behind the scene: Xc.z <= 0 never counts
    r = pixel(cams.get(), grey.get(), 2, 0, 5, 2, q5);
    CHECK(r.level == RC_NONE && r.cnt == 0 && r.sum == -1);
    return 0;
}

static int chosen_curves() {
    // cost curves by landing column (Table): L = 5 over [0.18, 0.42] at u = 5 lands on columns 7, 7, 8, 9, 9
    const std::unique_ptr<CamDev[]> cams(new CamDev[2]);
    cams[0] = camera(0.0); cams[1] = camera(1.0);
    RcRules q = {0.18, 0.42, 1e6, 0.9, 1, 3, 5, 1, 1};
    const double step = (0.42 - 0.18) / 4.0;
    int32_t by_u[W] = {};
    auto run = [&](void) { return rc_pixel(cams.get(), 2, 0, 5, 2, q, Table{by_u}); };
    by_u[7] = 90; by_u[8] = 100; by_u[9] = 100;                // best 90 at levels 0 and 1 -> 0; worst 100 at 2, 3, 4; 90 < 0.9 * 100 fails
    RcPixel r = run();
    CHECK(r.level == RC_NONE && r.sum == 90 && r.cnt == 1 && bits_of(r.out) == 0);
    by_u[7] = 89;                                              // 89 < 90: accepted at the lower of the tied levels; it has no level below it
    r = run();
    CHECK(r.level == 0 && r.sum == 89 && r.out == (float)0.18);
    by_u[7] = 100; by_u[8] = 50; by_u[9] = 100;                // a minimum with equal neighbours: den > 0, o = 0
    r = run();
    CHECK(r.level == 2 && r.sum == 50 && r.out == (float)(0.18 + 2.0 * step));
    by_u[9] = 70;                                              // c- = 100, c0 = 50, c+ = 70: o = 0.5 * 30 / 70
    r = run();
    CHECK(r.level == 2 && r.out == (float)(0.18 + (2.0 + 0.5 * (30.0 / 70.0)) * step));
    by_u[7] = 50; by_u[9] = 50;                                // flat: the best and the worst are both level 0
    r = run();
    CHECK(r.level == RC_NONE && r.sum == 50);
    q.peak = 1.0;                                              // m < m_W is strict
    CHECK(run().level == RC_NONE);
    by_u[7] = by_u[8] = by_u[9] = 0;                           // one colour
    r = run();
    CHECK(r.level == RC_NONE && r.sum == 0 && r.cnt == 1 && bits_of(r.out) == 0);
    by_u[7] = 10; by_u[8] = 10; by_u[9] = 9;                   // the best at levels 3 and 4 -> 3, whose upper neighbour ties it: den = 1, o = 0.5
    r = run();
    CHECK(r.level == 3 && r.out == (float)(0.18 + 3.5 * step));
    q.peak = 0.9;
    CHECK(run().level == RC_NONE);                             // 9 < 0.9 * 10 = 9 fails
    by_u[9] = 3; q.err = 0.5;                                  // sqrt(3 / 9) = 0.577 > 0.5
    CHECK(run().level == RC_NONE && run().sum == 3);
    q.err = 0.6;
    CHECK(run().level == 3);
    return 0;
}

static int run_file(const char* in, const char* out) {
    FILE* fi = std::fopen(in, "rb");
    CHECK(fi);
    int32_t hd[8];
    double pr[4];
    CHECK(std::fread(hd, sizeof hd, 1, fi) == 1 && std::fread(pr, sizeof pr, 1, fi) == 1);
    const int n = hd[0], w = hd[1], h = hd[2];
    const RcRules q = {pr[0], pr[1], pr[2], pr[3], hd[3], hd[4], hd[5], hd[6], hd[7]};
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
    const std::unique_ptr<float[]> res(new float[np]);
    const std::unique_ptr<int32_t[]> sum(new int32_t[np]);
    const std::unique_ptr<int16_t[]> lv(new int16_t[np]);
    CHECK(std::fread(img.get(), 3, np, fi) == np);
    std::fclose(fi);
    for (size_t i = 0; i < np; ++i) grey[i] = (uint8_t)grey8(img.get() + 3 * i);
    for (int f = 0; f < n; ++f)
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) {
                const size_t i = ((size_t)f * h + v) * w + u;
                const DrPlainSsd<Global> ssd = {{grey.get() + i, w}, grey.get(), w, h, q.N};
                const RcPixel r = rc_pixel(cams.get(), n, f, u, v, q, ssd);
                res[i] = r.out; lv[i] = (int16_t)r.level; sum[i] = r.sum; cnt[i] = (uint8_t)r.cnt;
            }
    FILE* fo = std::fopen(out, "wb");
    CHECK(fo && std::fwrite(res.get(), sizeof(float), np, fo) == np && std::fwrite(sum.get(), sizeof(int32_t), np, fo) == np &&
          std::fwrite(lv.get(), sizeof(int16_t), np, fo) == np && std::fwrite(cnt.get(), 1, np, fo) == np);
    CHECK(std::fclose(fo) == 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    if (order_and_value() || shifted_image() || chosen_curves()) return 1;
    std::printf("depth recover rules ok\n");
    return 0;
}
