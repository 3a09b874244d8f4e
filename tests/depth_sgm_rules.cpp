// Stand-alone host program for the rules of mvs_recover_depth_maps_aggregated (csrc/depth_sgm_rules.h), the body the kernels of
// depth_sgm.hip run.  tests/test_depth_sgm_host.py builds it with -fsanitize=address,undefined and runs it: every grey raster and every
// volume is a heap block of exact size, so a read one element outside it ends the program.  Without arguments it checks S1's quantised
// cost, S2's step and S4-S6 on chosen numbers.  With two arguments it runs S1-S6 (sg_frame) on a sequence the test wrote (`in`: int32 {n,
// w, h, N, refs, L, min_refs, flags, p1, p2, cost_cap, paths}, double {dsp_min, dsp_max, ssd_err, peak}, n cameras of 16 doubles {fx, fy,
// cx, cy, R[9], t[3]}, n * w * h * 3 image bytes) and writes `out`: per pixel the float of out, then the int32 sums, the int32 agg, the
// int16 levels and the uint8 cnt — what the test compares with tests/ref_depth_sgm.py.
#include "depth_sgm_rules.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Global {                                               // cur(a, b) from the grey raster itself
    const uint8_t* at;
    int w;
    int operator()(int a, int b) const { return at[a * w + b]; }
};

static uint32_t bits_of(float x) { uint32_t b; std::memcpy(&b, &x, sizeof b); return b; }

static int chosen_numbers() {
    // S1: int64 division, the cap, an ineligible level
    CHECK(sg_cost(98, 2, 7, 4095) == 1 && sg_cost(97, 2, 7, 4095) == 0 && sg_cost(0, 3, 1, 4095) == 0);
    CHECK(sg_cost(500000000, 1, 1, 4095) == 4095 && sg_cost(500000000, 8, 31, 4095) == 4095 && sg_cost(499999999, 8, 31, 65535) == 65036);
    CHECK(sg_cost(10, 0, 3, 255) == 255 && sg_cost(2295, 1, 3, 255) == 255 && sg_cost(2294, 1, 3, 255) == 254 && sg_cost(5, 1, 1, 1) == 1);
    // S2: each of the four terms wins once; a level outside [0, L - 1] never does; the bound cost_cap + p2
    CHECK(sg_step(7, 10, 20, 20, 10, 3, 9) == 7 && sg_step(7, 20, 10, 30, 10, 3, 9) == 10 && sg_step(7, 20, 30, 10, 10, 3, 9) == 10);
    CHECK(sg_step(7, 30, 30, 30, 10, 3, 9) == 16 && sg_step(7, 12, SG_FAR, SG_FAR, 10, 3, 9) == 9 && sg_step(4095, 9000, SG_FAR, 9000, 4000, 0, 4095) == 8190);
    CHECK(sg_step(5, 8, 8, 8, 8, 0, 0) == 5 && sg_step(5, 11, 9, 12, 8, 2, 2) == 7);
    // S4-S6 on [0.16, 0.4], L = 5, N = 1 (len * len = 9)
    RcRules q = {0.16, 0.4, 40.0, 0.9, 1, 3, 5, 1, 1};
    const double step = (0.4 - 0.16) / 4.0;
    SgPixel x = sg_finish(q, 2, 100, 50, 70, 45, 1, 100, 1);                    // accepted; o = 0.5 * 30 / 70
    CHECK(x.r.level == 2 && x.r.sum == 45 && x.r.cnt == 1 && x.agg == 50 && x.r.out == (float)(0.16 + (2.0 + 0.5 * (30.0 / 70.0)) * step));
    x = sg_finish(q, 2, 100, 50, 70, 45, 0, 100, 1);                            // l* is not eligible
    CHECK(x.r.level == RC_NONE && x.r.sum == -1 && x.r.cnt == 0 && x.agg == 50 && bits_of(x.r.out) == 0);
    x = sg_finish(q, 2, 100, 50, 70, 90, 1, 100, 1);                            // 90 < 0.9 * 100 fails; the raw pair is still reported
    CHECK(x.r.level == RC_NONE && x.r.sum == 90 && x.r.cnt == 1 && bits_of(x.r.out) == 0);
    x = sg_finish(q, 0, 12345, 50, 70, 45, 1, 100, 1);                          // no level below: no substep
    CHECK(x.r.level == 0 && x.r.out == rc_value(0.16, 0.16, 0.4) && (double)x.r.out >= 0.16);
    x = sg_finish(q, 4, 70, 50, 12345, 45, 1, 100, 1);                          // no level above: d = dsp_max, moved one float32 down
    CHECK(x.r.level == 4 && (double)(float)0.4 > 0.4 && x.r.out == std::nextafterf(0.4f, 0.0f));
    x = sg_finish(q, 2, 50, 50, 50, 45, 1, 100, 1);                             // flat S: den = 0
    CHECK(x.r.level == 2 && x.r.out == (float)(0.16 + 2.0 * step));
    q.flags = 0;
    x = sg_finish(q, 2, 100, 50, 70, 45, 1, 100, 1);
    CHECK(x.r.out == (float)(0.16 + 2.0 * step));
    q.err = 2.0;                                                                // sqrt(45 / 9) = 2.236 > 2
    CHECK(sg_finish(q, 2, 100, 50, 70, 45, 1, 100, 1).r.level == RC_NONE);
    // S3: the lowest level of the smallest S
    const int32_t col[5] = {9, 4, 7, 4, 4};
    const std::unique_ptr<CamDev[]> cams(new CamDev[1]);
    cams[0] = CamDev{};
    cams[0].fx = cams[0].fy = 10.0; cams[0].R[0] = cams[0].R[4] = cams[0].R[8] = 1.0; cams[0].w = 8; cams[0].h = 8;
    x = sg_select(cams.get(), 1, 0, 3, 3, q, [](int, int, int) { return 0; }, [&](int l) { return col[l]; }, 0, 0);
    CHECK(x.agg == 4 && x.r.cnt == 0 && x.r.level == RC_NONE);                  // a sequence of one frame: nothing is eligible
    return 0;
}

static int run_file(const char* in, const char* out) {
    FILE* fi = std::fopen(in, "rb");
    CHECK(fi);
    int32_t hd[12];
    double pr[4];
    CHECK(std::fread(hd, sizeof hd, 1, fi) == 1 && std::fread(pr, sizeof pr, 1, fi) == 1);
    const int n = hd[0], w = hd[1], h = hd[2];
    const RcRules q = {pr[0], pr[1], pr[2], pr[3], hd[3], hd[4], hd[5], hd[6], hd[7]};
    const SgRules g = {hd[8], hd[9], hd[10], hd[11]};
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
    const size_t fp = (size_t)w * h, np = (size_t)n * fp;
    const int rw = w - 2 * q.N, rh = h - 2 * q.N;
    const size_t rect = rw > 0 && rh > 0 ? (size_t)rw * rh : 0;
    const std::unique_ptr<uint8_t[]> img(new uint8_t[3 * np]), grey(new uint8_t[np]), cnt(new uint8_t[np]);
    const std::unique_ptr<float[]> res(new float[np]);
    const std::unique_ptr<int32_t[]> sum(new int32_t[np]), agg(new int32_t[np]), wpair(new int32_t[2 * rect]), line(new int32_t[2 * (size_t)q.L]);
    const std::unique_ptr<int16_t[]> lv(new int16_t[np]);
    const std::unique_ptr<uint16_t[]> vol(new uint16_t[rect * q.L]), acc(new uint16_t[rect * q.L]);
    CHECK(std::fread(img.get(), 3, np, fi) == np);
    std::fclose(fi);
    for (size_t i = 0; i < np; ++i) grey[i] = (uint8_t)grey8(img.get() + 3 * i);
    for (int f = 0; f < n; ++f) {
        const uint8_t* gf = grey.get() + f * fp;
        auto make_ssd = [&](int u, int v) { return DrPlainSsd<Global>{{gf + (size_t)v * w + u, w}, grey.get(), w, h, q.N}; };
        sg_frame(cams.get(), n, f, q, g, make_ssd, vol.get(), acc.get(), wpair.get(), line.get(), res.get() + f * fp, lv.get() + f * fp, sum.get() + f * fp,
                 cnt.get() + f * fp, agg.get() + f * fp);
    }
    FILE* fo = std::fopen(out, "wb");
    CHECK(fo && std::fwrite(res.get(), sizeof(float), np, fo) == np && std::fwrite(sum.get(), sizeof(int32_t), np, fo) == np &&
          std::fwrite(agg.get(), sizeof(int32_t), np, fo) == np && std::fwrite(lv.get(), sizeof(int16_t), np, fo) == np &&
          std::fwrite(cnt.get(), 1, np, fo) == np);
    CHECK(std::fclose(fo) == 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    if (chosen_numbers()) return 1;
    std::printf("depth sgm rules ok\n");
    return 0;
}
