// Stand-alone host program for the rules of mvs_grabcut_masks (csrc/grabcut_rules.h), the body the kernels of grabcut.hip run.
// tests/test_grabcut_host.py builds it with -fsanitize=address,undefined and runs it: every array is a heap block of exact size, so a
// read past the odd last row or column, or past the half mask in rule 12, aborts.
//   grabcut_rules                 its own cases: an odd-sized image, a one-colour component (det <= DBL_EPSILON), an empty model
//   grabcut_rules in.bin out.bin  one frame of a scene through one iteration, for the comparison with tests/ref_grabcut.py.
//     in : int32 w, h, start (1: the foreground mask is the rectangle); double hl, hr, vl, vr, gamma; the image; then, unless start,
//          uint8 fg [hh * hw] (the mask the iteration starts from)
//     out: uint32 half [N]; int64 S; int32 ncap [8][N]; uint8 labels0 [N]; int64 sums0 [100]; uint8 labels1 [N]; int64 sums1 [100];
//          int32 excess [N]; uint8 full [h * w] (rule 12 of fg)
#include "grabcut_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const int DX[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "grabcut_rules.cpp:%d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

struct Frame {
    int w, h, hw, hh, N;
    GcRect r;
    double gamma;
    std::vector<uint32_t> half;
    std::vector<uint8_t> fg, label;
    std::vector<int64_t> sums;              // [2][5][10]
    std::vector<GcComp> comps;              // [2][5]
};

static void make_half(Frame& f, const uint8_t* img) {
    f.hw = f.w / 2; f.hh = f.h / 2; f.N = f.hw * f.hh;
    f.half.resize((size_t)f.N);
    for (int y = 0; y < f.hh; ++y)
        for (int x = 0; x < f.hw; ++x) f.half[(size_t)y * f.hw + x] = gc_half_px(img, f.w, x, y);
}
static void start_labels(Frame& f) {
    std::vector<int32_t> hist(2 * GC_LUMA, 0);
    int64_t m[2] = {0, 0};
    for (int i = 0; i < f.N; ++i) { const int k = f.fg[(size_t)i] ? 0 : 1; ++hist[(size_t)k * GC_LUMA + gc_luma(f.half[(size_t)i])]; ++m[k]; }
    int32_t t[2][4];
    for (int k = 0; k < 2; ++k) gc_thresholds(hist.data() + (size_t)k * GC_LUMA, m[k], t[k]);
    f.label.resize((size_t)f.N);
    for (int i = 0; i < f.N; ++i) f.label[(size_t)i] = (uint8_t)gc_luma_component(gc_luma(f.half[(size_t)i]), t[f.fg[(size_t)i] ? 0 : 1]);
}
static void learn(Frame& f) {
    f.sums.assign(2 * GC_K * GC_SUMS, 0);
    for (int i = 0; i < f.N; ++i) {
        const uint32_t p = f.half[(size_t)i];
        const int64_t c[3] = {gc_ch(p, 0), gc_ch(p, 1), gc_ch(p, 2)};
        int64_t* s = f.sums.data() + (size_t)((f.fg[(size_t)i] ? 0 : 1) * GC_K + f.label[(size_t)i]) * GC_SUMS;
        s[0] += 1; s[1] += c[0]; s[2] += c[1]; s[3] += c[2];
        s[4] += c[0] * c[0]; s[5] += c[0] * c[1]; s[6] += c[0] * c[2]; s[7] += c[1] * c[1]; s[8] += c[1] * c[2]; s[9] += c[2] * c[2];
    }
    f.comps.resize(2 * GC_K);
    for (int k = 0; k < 2 * GC_K; ++k) {
        const int64_t* model = f.sums.data() + (size_t)(k / GC_K) * GC_K * GC_SUMS;
        int64_t m = 0;
        for (int j = 0; j < GC_K; ++j) m += model[j * GC_SUMS];
        gc_fit(model + (k % GC_K) * GC_SUMS, m, &f.comps[(size_t)k]);
    }
}
static void assign(Frame& f) {
    for (int i = 0; i < f.N; ++i) f.label[(size_t)i] = (uint8_t)gc_assign(f.comps.data() + (f.fg[(size_t)i] ? 0 : GC_K), f.half[(size_t)i]);
}
static int64_t beta_sum(const Frame& f) {
    int64_t S = 0;
    for (int y = 0; y < f.hh; ++y)
        for (int x = 0; x < f.hw; ++x)
            for (int d = 0; d < 4; ++d) {
                const int nx = x + DX[d], ny = y + DY[d];
                if (nx >= 0 && nx < f.hw && ny >= 0) S += gc_d2(f.half[(size_t)y * f.hw + x], f.half[(size_t)ny * f.hw + nx]);
            }
    return S;
}
static std::vector<uint8_t> full_mask(const Frame& f, const std::vector<uint8_t>& half_mask) {
    std::vector<uint8_t> out((size_t)f.w * f.h);
    for (int y = 0; y < f.h; ++y)
        for (int x = 0; x < f.w; ++x) out[(size_t)y * f.w + x] = gc_full_px(half_mask.data(), f.hw, f.hh, x, y);
    return out;
}

static void own_cases() {
    // 7 x 5: hw = 3, hh = 2; the last row and column are never read, rule 12 clamps at every border
    Frame f;
    f.w = 7; f.h = 5; f.gamma = 50.0;
    std::vector<uint8_t> img((size_t)f.w * f.h * 3);
    for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)((i * 37) % 251);
    make_half(f, img.data());
    CHECK(f.hw == 3 && f.hh == 2);
    CHECK(gc_ch(f.half[0], 0) == (img[0] + img[3] + img[21] + img[24] + 2) / 4);
    f.r = gc_rect(f.hw, f.hh, 0.0, 0.0, 0.0, 0.0);
    CHECK(f.r.x0 == 0 && f.r.x1 == 3 && f.r.y0 == 0 && f.r.y1 == 2);
    std::vector<uint8_t> hm((size_t)f.N, 0);
    hm[(size_t)f.N - 1] = 1;                                          // the bottom-right half pixel alone
    const std::vector<uint8_t> full = full_mask(f, hm);
    CHECK(full[(size_t)4 * 7 + 6] == 255 && full[(size_t)3 * 7 + 6] == 255 && full[(size_t)4 * 7 + 3] == 255 && full[0] == 0 && full[3] == 0 && full[(size_t)4 * 7 + 1] == 0);
    CHECK(full[(size_t)2 * 7 + 3] == 255);                            // x = 3 (odd): columns 1, 2; y = 2 (even): rows 0, 1
    // the whole image one model of one colour: every covariance is 0, det <= DBL_EPSILON, 0.01 on the diagonal
    f.fg.assign((size_t)f.N, 1);
    std::fill(f.half.begin(), f.half.end(), 0x00203040u);
    start_labels(f);
    learn(f);
    int used = 0;
    for (int k = 0; k < GC_K; ++k) used += f.comps[(size_t)k].used;
    CHECK(used >= 1);
    for (int k = 0; k < GC_K; ++k)
        if (f.comps[(size_t)k].used) { CHECK(f.comps[(size_t)k].det > 9.9e-7 && f.comps[(size_t)k].det < 1.01e-6); CHECK(f.comps[(size_t)k].inv[0] > 99.0); }
    for (int k = 0; k < GC_K; ++k) CHECK(!f.comps[(size_t)(GC_K + k)].used);         // the background has no pixel: every component empty
    CHECK(gc_L(f.comps.data() + GC_K, f.half[0], f.gamma) == 9.0 * f.gamma);
    CHECK(gc_excess(f.comps.data(), f.comps.data() + GC_K, f.half[0], f.gamma, true) == gc_tlink_max(f.gamma));
    CHECK(gc_excess(f.comps.data(), f.comps.data() + GC_K, f.half[0], f.gamma, false) == -gc_tlink_max(f.gamma));
    CHECK(gc_assign(f.comps.data() + GC_K, f.half[0]) == 0);
    CHECK(beta_sum(f) == 0 && gc_beta(0, f.hw, f.hh) == 0.0 && gc_ncap(0.0, 50.0, 0, false) == 51200 && gc_ncap(0.0, 50.0, 0, true) == 36204);
    CHECK(gc_pairs(3, 2) == 11);
    int32_t t[4];
    std::vector<int32_t> hist(GC_LUMA, 0);
    gc_thresholds(hist.data(), 0, t);                                 // an empty model
    hist[10] = 3; hist[700] = 2;
    gc_thresholds(hist.data(), 5, t);                                 // targets 1, 2, 3, 4
    CHECK(t[0] == 10 && t[1] == 10 && t[2] == 10 && t[3] == 700 && gc_luma_component(10, t) == 0 && gc_luma_component(700, t) == 3 && gc_luma_component(765, t) == 4);
    std::printf("grabcut rules ok\n");
}

template <class T> static void put(std::FILE* fh, const T* p, size_t n) { CHECK(std::fwrite(p, sizeof(T), n, fh) == n); }

int main(int argc, char** argv) {
    if (argc < 3) { own_cases(); return 0; }
    std::FILE* in = std::fopen(argv[1], "rb");
    CHECK(in);
    int32_t hd[3];
    double pr[5];
    CHECK(std::fread(hd, sizeof(int32_t), 3, in) == 3 && std::fread(pr, sizeof(double), 5, in) == 5);
    Frame f;
    f.w = hd[0]; f.h = hd[1]; f.gamma = pr[4];
    std::vector<uint8_t> img((size_t)f.w * f.h * 3);
    CHECK(std::fread(img.data(), 1, img.size(), in) == img.size());
    make_half(f, img.data());
    f.r = gc_rect(f.hw, f.hh, pr[0], pr[1], pr[2], pr[3]);
    std::vector<uint8_t> inside((size_t)f.N), fg((size_t)f.N);
    for (int i = 0; i < f.N; ++i) inside[(size_t)i] = gc_inside(f.r, i % f.hw, i / f.hw) ? 1 : 0;
    if (hd[2]) fg = inside; else CHECK(std::fread(fg.data(), 1, fg.size(), in) == fg.size());
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    CHECK(out);
    put(out, f.half.data(), f.half.size());
    const int64_t S = beta_sum(f);
    put(out, &S, 1);
    const double beta = gc_beta(S, f.hw, f.hh);
    std::vector<int32_t> ncap((size_t)8 * f.N, 0);
    for (int d = 0; d < 8; ++d)
        for (int i = 0; i < f.N; ++i) {
            const int nx = i % f.hw + DX[d], ny = i / f.hw + DY[d];
            if (nx >= 0 && nx < f.hw && ny >= 0 && ny < f.hh)
                ncap[(size_t)d * f.N + i] = gc_ncap(beta, f.gamma, gc_d2(f.half[(size_t)i], f.half[(size_t)ny * f.hw + nx]), (d & 1) != 0);
        }
    put(out, ncap.data(), ncap.size());
    f.fg = inside;                                                    // rule 4 and its learn start from the rectangle
    start_labels(f);
    learn(f);
    put(out, f.label.data(), f.label.size());
    put(out, f.sums.data(), f.sums.size());
    f.fg = fg;                                                        // one iteration from the given mask
    assign(f);
    learn(f);
    put(out, f.label.data(), f.label.size());
    put(out, f.sums.data(), f.sums.size());
    std::vector<int32_t> e((size_t)f.N);
    for (int i = 0; i < f.N; ++i) e[(size_t)i] = gc_excess(f.comps.data(), f.comps.data() + GC_K, f.half[(size_t)i], f.gamma, inside[(size_t)i] != 0);
    put(out, e.data(), e.size());
    const std::vector<uint8_t> full = full_mask(f, fg);
    put(out, full.data(), full.size());
    CHECK(std::fclose(out) == 0);
    return 0;
}
