// Stand-alone host program for the rules of mvs_colour_vertices (csrc/colour_rules.h), the body the kernels of colour.hip run.
// tests/test_colour_host.py builds it with -fsanitize=address,undefined and runs it: every image and raster is a heap block of exactly
// N * h * w (* 3) elements, so a read one element outside it ends the program.  With two arguments it runs C1-C8 on a scene the test
// wrote (`in`: int32 {V, N, n_seq, w, h, flags, has_depths, has_chain}, double {min_cos, occ_tol}, 4 bytes {fill[3], 0}, N views of 17
// doubles {fx, fy, cx, cy, R[9], t[3], sequence}, with a chain n_seq records of 13 doubles {s, R[9], t[3]}, V * 3 doubles of points, V * 3
// of normals, N * h * w * 3 image bytes, with depths N * h * w floats) and writes `out`: V * 3 colour bytes, then V int32 counts — what
// the test compares with tests/ref_colour.py.
#include "colour_rules.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static ColView view(double fx, double cx, double cy, int w, int h, double tx = 0.0) {   // looking down +z
    ColView v = {};
    v.c.fx = v.c.fy = fx; v.c.cx = cx; v.c.cy = cy;
    v.c.R[0] = v.c.R[4] = v.c.R[8] = 1.0;
    v.c.t[0] = tx;
    v.c.w = w; v.c.h = h;
    return v;
}

// a 2 x 2 image, the smallest the call takes: every corner of the image is a corner of the one bilinear cell
static int smallest_image() {
    const int w = 2, h = 2;
    std::unique_ptr<uint8_t[]> img(new uint8_t[w * h * 3]);
    for (int i = 0; i < w * h * 3; ++i) img[i] = (uint8_t)(10 + 20 * i);                  // pixel (x, y), channel c: 10 + 20 (3 (2 y + x) + c)
    std::unique_ptr<float[]> ras(new float[w * h]);
    for (int i = 0; i < w * h; ++i) ras[i] = 0.5f;                                       // a surface at z = 2
    const ColView v = view(2.0, 0.5, 0.5, w, h);                                         // x = X + 0.5 at z = 2
    const ColRules q = {0.2, 0.01, 0, {1, 2, 3}};
    const d3 n = mk3(0, 0, -1);
    uint8_t c[3];
    // the four corners: x0 and y0 clamp to 0 and ax, ay are 0 or 256, so the result is the corner's pixel
    for (int y = 0; y < 2; ++y)
        for (int x = 0; x < 2; ++x) {
            CHECK(col_vertex(mk3(x - 0.5, y - 0.5, 2.0), n, &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 1);
            for (int ch = 0; ch < 3; ++ch) CHECK(c[ch] == 10 + 20 * (3 * (2 * y + x) + ch));
        }
    // the centre: the mean of the four pixels, rounded to nearest
    CHECK(col_vertex(mk3(0.0, 0.0, 2.0), n, &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 1);
    CHECK(c[0] == (10 + 70 + 130 + 190 + 2) / 4);
    // outside by one part in 2^40, behind, a NaN normal, a NaN point, facing away: the fill and no view
    const d3 bad_p[] = {mk3(0.5 + 1.0 / 1099511627776.0, 0, 2), mk3(0, 0, -2), mk3(0, 0, 2), mk3(NAN, 0, 2), mk3(0, 0, 2), mk3(0, 0, 0)};
    const d3 bad_n[] = {n, n, mk3(NAN, 0, -1), n, mk3(0, 0, 1), n};
    for (int k = 0; k < 6; ++k) {
        CHECK(col_vertex(bad_p[k], bad_n[k], &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 0);
        CHECK(c[0] == 1 && c[1] == 2 && c[2] == 3);
    }
    // C4: the raster says z = 2; a vertex at z = 2.03 is hidden, one at 2.01 is seen, and a pixel nothing was drawn on hides everything
    CHECK(col_vertex(mk3(0, 0, 2.03), n, &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 0);
    CHECK(col_vertex(mk3(0, 0, 2.01), n, &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 1);
    CHECK(col_vertex(mk3(0, 0, 2.03), n, &v, 1, nullptr, w, h, img.get(), nullptr, q, c) == 1);
    ras[3] = 0.0f;                                                                       // pixel (1, 1)
    CHECK(col_vertex(mk3(0.3, 0.3, 2.0), n, &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 0);
    CHECK(col_vertex(mk3(-0.3, 0.3, 2.0), n, &v, 1, nullptr, w, h, img.get(), ras.get(), q, c) == 1);
    return 0;
}

// two views of equal weight and one of less: the blend, the tie of MVS_COLOUR_BEST and the smallest weight
static int weights_and_ties() {
    const int w = 3, h = 2, N = 3;
    std::unique_ptr<uint8_t[]> img(new uint8_t[N * w * h * 3]);
    for (int v = 0; v < N; ++v)
        for (int i = 0; i < w * h * 3; ++i) img[v * w * h * 3 + i] = (uint8_t)(50 * (v + 1));   // one colour per view: 50, 100, 150
    ColView vs[3] = {view(2.0, 1.0, 0.5, w, h, 0.5), view(2.0, 1.0, 0.5, w, h, -0.5), view(2.0, 1.0, 0.5, w, h, -0.5)};
    ColRules q = {0.2, 0.01, 0, {0, 0, 0}};
    const d3 p = mk3(0, 0, 2), n = mk3(0, 0, -1);
    uint8_t c[3];
    int32_t wq[3], S[3];
    for (int v = 0; v < N; ++v) CHECK(col_view(p, n, vs[v].c, w, h, img.get() + v * w * h * 3, nullptr, q, &wq[v], S) && S[0] == 65536 * 50 * (v + 1));
    CHECK(wq[0] == wq[1] && wq[1] == wq[2] && wq[0] > 3000 && wq[0] < 4096);            // mirrored about x = 0: equal bit for bit
    CHECK(col_vertex(p, n, vs, N, nullptr, w, h, img.get(), nullptr, q, c) == 3 && c[0] == 100);
    q.best = 1;
    CHECK(col_vertex(p, n, vs, N, nullptr, w, h, img.get(), nullptr, q, c) == 3 && c[0] == 50);      // the lowest view index
    CHECK(col_vertex(p, n, vs + 1, 2, nullptr, w, h, img.get() + w * h * 3, nullptr, q, c) == 2 && c[0] == 100);
    // the accumulators of two lanes that shared the views give the same key order as one walk
    ColAcc a = col_acc_zero(), b = col_acc_zero();
    int32_t s50[3] = {50, 50, 50}, s100[3] = {100, 100, 100};
    col_add(a, 1, 5, 7, s50);
    col_add(b, 1, 2, 7, s100);
    CHECK(b.key > a.key && col_key(8, 9) > b.key && a.n == 1);
    // a grazing view: cos just above min_cos gives a small weight, never 0
    q.min_cos = 1e-3; q.best = 0;
    const d3 graze = mk3(2.0, 0.0, -0.51);                                              // q = (0.5, 0, 2): cos = 0.0047
    CHECK(col_view(p, graze, vs[0].c, w, h, img.get(), nullptr, q, &wq[0], S) && wq[0] == 1);
    return 0;
}

// a chain: the vertex mapped by C1 is the vertex mvs_srt_apply(inverse = 1) gives
static int the_map() {
    const double R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t[3] = {1, 2, 3};
    const ColSeq m = col_make_seq(2.0, R, t);
    d3 pm, nm;
    col_map(m, mk3(-7, 8, 13), mk3(0, -1, 0), &pm, &nm);                               // p = 2 R (3, 4, 5) + t
    CHECK(pm.x == 3 && pm.y == 4 && pm.z == 5 && nm.x == -1 && nm.y == 0 && nm.z == 0);
    return 0;
}

static int run_file(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    CHECK(f);
    int32_t hd[8];
    double pr[2];
    uint8_t fill[4];
    CHECK(std::fread(hd, 4, 8, f) == 8 && std::fread(pr, 8, 2, f) == 2 && std::fread(fill, 1, 4, f) == 4);
    const int V = hd[0], N = hd[1], n_seq = hd[2], w = hd[3], h = hd[4];
    std::vector<ColView> views((size_t)N);
    for (int v = 0; v < N; ++v) {
        double c[17];
        CHECK(std::fread(c, 8, 17, f) == 17);
        views[v] = ColView{};
        views[v].c.fx = c[0]; views[v].c.fy = c[1]; views[v].c.cx = c[2]; views[v].c.cy = c[3];
        std::memcpy(views[v].c.R, c + 4, 72);
        std::memcpy(views[v].c.t, c + 13, 24);
        views[v].c.w = w; views[v].c.h = h;
        views[v].seq = (int32_t)c[16];
    }
    std::vector<ColSeq> seqs;
    for (int k = 0; hd[7] && k < n_seq; ++k) {
        double s[13];
        CHECK(std::fread(s, 8, 13, f) == 13);
        seqs.push_back(col_make_seq(s[0], s + 1, s + 10));
    }
    const size_t npx = (size_t)N * w * h;
    std::unique_ptr<double[]> pts(new double[3 * (size_t)V]), nrm(new double[3 * (size_t)V]);
    std::unique_ptr<uint8_t[]> img(new uint8_t[3 * npx]);
    std::unique_ptr<float[]> ras(new float[hd[6] ? npx : 1]);
    CHECK(std::fread(pts.get(), 8, 3 * (size_t)V, f) == 3 * (size_t)V && std::fread(nrm.get(), 8, 3 * (size_t)V, f) == 3 * (size_t)V);
    CHECK(std::fread(img.get(), 1, 3 * npx, f) == 3 * npx);
    if (hd[6]) CHECK(std::fread(ras.get(), 4, npx, f) == npx);
    std::fclose(f);
    const ColRules q = {pr[0], pr[1], hd[5] & 1, {fill[0], fill[1], fill[2]}};
    std::vector<uint8_t> col(3 * (size_t)V);
    std::vector<int32_t> cnt((size_t)V);
    for (int i = 0; i < V; ++i)
        cnt[i] = col_vertex(ld3(pts.get() + 3 * i), ld3(nrm.get() + 3 * i), views.data(), N, seqs.empty() ? nullptr : seqs.data(), w, h, img.get(),
                            hd[6] ? ras.get() : nullptr, q, col.data() + 3 * i);
    FILE* g = std::fopen(out, "wb");
    CHECK(g);
    CHECK(std::fwrite(col.data(), 1, col.size(), g) == col.size() && std::fwrite(cnt.data(), 4, cnt.size(), g) == cnt.size());
    std::fclose(g);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    if (smallest_image() || weights_and_ties() || the_map()) return 1;
    std::printf("colour rules ok\n");
    return 0;
}
