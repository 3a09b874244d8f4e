// srt_refine_rules.cpp — csrc/srt_refine_rules.h on the host, as a stand-alone program for the address and undefined-behaviour
// sanitizers (tests/test_srt_refine_host.py builds and runs it).  `prog in out`: the scene of `in` (written by that test), a brute-force
// float32 nearest point with d2f and the lower-index tie, then I1-I6 of the header for every ordered pair; `out` receives the
// n_seq * n_seq * 121 int64 sums.  Without arguments: a few cases of the header on their own.  Every array is a heap block of exact size.
#include "srt_refine_rules.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fail(const char* what) { std::fprintf(stderr, "srt refine rules: %s\n", what); return 1; }

static int self_test() {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
    d3 u;
    if (srr_unit(mk3(0, 0, 0), &u) || srr_unit(mk3(NAN, 0, 1), &u) || srr_unit(mk3(1e200, 0, 0), &u) || srr_unit(mk3(1e-200, 0, 0), &u)) return fail("unit accepts");
    if (!srr_unit(mk3(0, 3, 4), &u) || u.y != 0.6 || u.z != 0.8) return fail("unit");
    if (srr_usable(mk3(NAN, 0, 0)) || srr_usable(mk3(0, INFINITY, 0)) || srr_usable(mk3(0, 0, 3.5e38)) || !srr_usable(mk3(3.4e38, -1, 0))) return fail("usable");
    if (srr_quant(0.5) != 34359738368LL || srr_quant(-1.0) != -68719476736LL || srr_quant(1.5 / 68719476736.0) != 2 || srr_quant(2.5 / 68719476736.0) != 2)
        return fail("quant");
    const SrrMap A = srr_map(2.0, I, z), B = srr_map(1.0, I, z);
    const SrrFrame f = {{0, 0, 0}, 4.0, 0.25 * 0.25, 0.0};
    double r, J[14];
    if (!srr_match(A, B, f, mk3(0.5, 0, 0), mk3(0, 0, 2), mk3(0, 0, 0), mk3(0, 0, 1), &r, J)) return fail("match at the cap");      // |x_a - x_b| = 1/4
    if (r != 0.0 || J[5] != 1.0 || J[12] != -1.0 || J[1] != -0.25) return fail("match values");
    if (srr_match(A, B, f, mk3(0.5, 0, 1e-7), mk3(0, 0, 2), mk3(0, 0, 0), mk3(0, 0, 1), &r, J)) return fail("beyond the cap");
    if (!srr_match(A, B, f, mk3(0, 0, 0), mk3(1, 0, 0), mk3(0, 0, 0), mk3(0, 0, 1), &r, J)) return fail("cosine 0 meets min_cos 0");
    if (srr_match(A, B, f, mk3(0, 0, 0), mk3(0, 0, -1), mk3(0, 0, 0), mk3(0, 0, 1), &r, J)) return fail("opposite normals");
    if (srr_match(A, B, f, mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 1), &r, J)) return fail("zero normal");
    int seen = 0, last = -1;
    bool ordered = true;
    srr_terms(0.5, J, [&](int k, long long) { ++seen; ordered = ordered && (k == last + 1 || k >= SRR_JR); last = k; });
    if (seen != SRR_TERMS || last != SRR_RR || !ordered) return fail("terms");
    const double Rz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, tb[3] = {1, 2, 3}, ta[3] = {3, 2, 1};
    const SrrMap rel = srr_relative(2.0, Rz, tb, 4.0, I, ta);                      // p -> (1/2) Rz^T (4 p + ta - tb)
    const d3 y = srr_apply(rel, mk3(1, 0, 0));
    if (y.x != 0.0 || y.y != -3.0 || y.z != -1.0) return fail("relative");
    std::puts("srt refine rules ok");
    return 0;
}

template <class T> static bool rd(std::FILE* fp, T* p, size_t n) { return std::fread(p, sizeof(T), n, fp) == n; }

int main(int argc, char** argv) {
    if (argc < 3) return self_test();
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return fail("cannot open the input");
    int32_t head[2];
    double th[2];
    if (!rd(fp, head, 2) || !rd(fp, th, 2)) return fail("short header");
    const int n = head[0], stride = head[1];
    std::vector<int64_t> seg((size_t)n + 1);
    std::vector<double> chain((size_t)13 * n);
    if (!rd(fp, seg.data(), seg.size()) || !rd(fp, chain.data(), chain.size())) return fail("short tables");
    const size_t P = (size_t)seg[n];
    std::vector<double> pts(3 * P), nrm(3 * P);
    if (!rd(fp, pts.data(), pts.size()) || !rd(fp, nrm.data(), nrm.size())) return fail("short arrays");
    std::fclose(fp);
    std::vector<SrrMap> maps;
    for (int k = 0; k < n; ++k) maps.push_back(srr_map(chain[13 * k], &chain[13 * k + 1], &chain[13 * k + 10]));
    // I2
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < n; ++k)
        for (int64_t i = seg[k]; i < seg[k + 1]; ++i) {
            const d3 p = ld3(&pts[3 * i]);
            if (!srr_usable(p)) continue;
            const d3 y = srr_apply(maps[k], p);
            lo[0] = fmin(lo[0], y.x); lo[1] = fmin(lo[1], y.y); lo[2] = fmin(lo[2], y.z);
            hi[0] = fmax(hi[0], y.x); hi[1] = fmax(hi[1], y.y); hi[2] = fmax(hi[2], y.z);
        }
    SrrFrame f;
    for (int c = 0; c < 3; ++c) f.c[c] = (lo[c] + hi[c]) / 2.0;
    f.D = norm3(mk3(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])) / 2.0;
    const double cap = 2.0 * th[0];
    f.cap2 = cap * cap; f.min_cos = th[1];
    if (!(f.D > 0.0)) return fail("no box");
    std::vector<long long> sums((size_t)n * n * SRR_TERMS, 0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            if (a == b) continue;
            const SrrMap rel = srr_relative(chain[13 * b], &chain[13 * b + 1], &chain[13 * b + 10], chain[13 * a], &chain[13 * a + 1], &chain[13 * a + 10]);
            long long* S = &sums[((size_t)a * n + b) * SRR_TERMS];
            for (int64_t i = seg[a]; i < seg[a + 1]; i += stride) {
                const d3 pa = ld3(&pts[3 * i]);
                if (!srr_usable(pa)) continue;
                const d3 yb = srr_apply(rel, pa);
                const float qx = (float)yb.x, qy = (float)yb.y, qz = (float)yb.z;
                if (!((qx - qx == 0.0f) && (qy - qy == 0.0f) && (qz - qz == 0.0f))) continue;
                float best = INFINITY;
                int64_t arg = -1;
                for (int64_t j = seg[b]; j < seg[b + 1]; ++j) {
                    const d3 pb = ld3(&pts[3 * j]);
                    if (!srr_usable(pb)) continue;
                    const float d = d2f(qx, qy, qz, (float)pb.x, (float)pb.y, (float)pb.z);
                    if (d < best) { best = d; arg = j; }              // ascending j: the first of the least stays
                }
                if (arg < 0) continue;
                double r, J[14];
                if (!srr_match(maps[a], maps[b], f, pa, ld3(&nrm[3 * i]), ld3(&pts[3 * arg]), ld3(&nrm[3 * arg]), &r, J)) continue;
                srr_terms(r, J, [&](int k, long long v) { S[k] += v; });
            }
        }
    fp = std::fopen(argv[2], "wb");
    if (!fp || std::fwrite(sums.data(), sizeof(long long), sums.size(), fp) != sums.size()) return fail("cannot write the output");
    std::fclose(fp);
    return 0;
}
