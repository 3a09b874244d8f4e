// Stand-alone host program for the two pieces of host code the front-end entries share: the stage-1 rule of the match filter
// (mp_stage1, csrc/frontend_dev.h — the body k_mp_map runs per thread and mvs_match_filter runs per raw match on the host) and
// check_offsets (csrc/engine.h).  tests/test_match_pairs_host.py builds it with -fsanitize=address,undefined and runs it: every
// table below is a heap block of exactly the documented size, so a read one element outside it ends the program.
#include "engine.h"
#include "frontend_dev.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

static char g_err[256];
void mvs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static unsigned long long key_of(unsigned long long u1, unsigned long long v1, unsigned long long u2, unsigned long long v2) {
    return (u1 << 48) | (v1 << 32) | (u2 << 16) | v2;
}

static int stage1() {
    const int w = 5, h = 4, views = 2, npx = w * h;
    // view 0: the identity; view 1: the pixels in reverse order.  Frame 2's tables differ from frame 1's.
    std::vector<int32_t> tex1((size_t)views * npx), tex2((size_t)views * npx);
    std::vector<uint8_t> valid1((size_t)npx, 1), valid2((size_t)npx, 1);
    for (int px = 0; px < npx; ++px) {
        tex1[px] = px; tex1[npx + px] = npx - 1 - px;
        tex2[px] = npx - 1 - px; tex2[npx + px] = px;
    }
    auto rule = [&](int a1, int u1, int v1, int a2, int u2, int v2) {
        const std::vector<int32_t> q = {a1, u1, v1, a2, u2, v2};          // exactly six values
        return mp_stage1(q.data(), tex1.data(), valid1.data(), tex2.data(), valid2.data(), w, h, views);
    };
    const int us[4] = {-1, 0, w - 1, w}, vs[4] = {-1, 0, h - 1, h};
    int inside = 0;
    for (int a1 = 0; a1 < views; ++a1)
        for (int a2 = 0; a2 < views; ++a2)
            for (int i1 = 0; i1 < 16; ++i1)
                for (int i2 = 0; i2 < 16; ++i2) {
                    const int u1 = us[i1 & 3], v1 = vs[i1 >> 2], u2 = us[i2 & 3], v2 = vs[i2 >> 2];
                    const unsigned long long got = rule(a1, u1, v1, a2, u2, v2);
                    if (u1 < 0 || u1 >= w || v1 < 0 || v1 >= h || u2 < 0 || u2 >= w || v2 < 0 || v2 >= h) { CHECK(got == MP_NONE); continue; }
                    const int px1 = v1 * w + u1, px2 = v2 * w + u2;
                    const int b1 = a1 == 0 ? px1 : npx - 1 - px1, b2 = a2 == 0 ? npx - 1 - px2 : px2;
                    CHECK(got == key_of(b1 % w, b1 / w, b2 % w, b2 / w));
                    ++inside;
                }
    CHECK(inside == views * views * 4 * 4);
    // the view test fires first, whatever the pixel is
    CHECK(rule(-1, 0, 0, 0, 0, 0) == MP_BAD_VIEW && rule(views, 0, 0, 0, 0, 0) == MP_BAD_VIEW && rule(0, 0, 0, views, 0, 0) == MP_BAD_VIEW);
    CHECK(rule(0, -1, h, views, w, -1) == MP_BAD_VIEW && rule(0, 0, 0, -1, 0, 0) == MP_BAD_VIEW);
    // tex = -1 on either side; valid is read at the generated-view pixel, not at the base pixel tex names
    const unsigned long long before = rule(1, 1, 2, 0, 3, 1);
    CHECK(before == key_of((npx - 12) % w, (npx - 12) / w, (npx - 9) % w, (npx - 9) / w));
    tex1[npx + 2 * w + 1] = -1;
    CHECK(rule(1, 1, 2, 0, 3, 1) == MP_NONE && rule(0, 1, 2, 0, 3, 1) != MP_NONE);
    tex1[npx + 2 * w + 1] = npx - 12;
    tex2[1 * w + 3] = -1;
    CHECK(rule(1, 1, 2, 0, 3, 1) == MP_NONE && rule(1, 1, 2, 1, 3, 1) != MP_NONE);
    tex2[1 * w + 3] = npx - 9;
    CHECK(rule(1, 1, 2, 0, 3, 1) == before);
    valid1[2 * w + 1] = 0;
    CHECK(rule(1, 1, 2, 0, 3, 1) == MP_NONE && rule(0, 1, 2, 0, 3, 1) == MP_NONE);
    valid1[2 * w + 1] = 1;
    valid1[npx - 12] = 0;                                                  // the base pixel of view 1's (1, 2): not what is read
    CHECK(rule(1, 1, 2, 0, 3, 1) == before);
    valid2[1 * w + 3] = 0;
    CHECK(rule(1, 1, 2, 0, 3, 1) == MP_NONE);
    // the keys order as (u1,v1,u2,v2) does, and neither marker is a key of an image of at most 65535 x 65535
    CHECK(key_of(1, 0, 0, 0) > key_of(0, 65534, 65534, 65534) && key_of(0, 1, 0, 0) > key_of(0, 0, 65534, 65534));
    CHECK(mp_key(65534, 65534, 65534, 65534) < MP_BAD_VIEW && MP_BAD_VIEW < MP_NONE);
    return 0;
}

template <class T> static int offsets_of_type() {
    auto run = [](std::vector<T> off, int64_t limit) {                     // n + 1 offsets, exactly
        g_err[0] = 0;
        return check_offsets("fn", "offs", off.data(), (int64_t)off.size() - 1, limit);
    };
    CHECK(run({0}, 0) == MVS_OK && !g_err[0]);                             // the empty list
    CHECK(run({0}, 0x7fffffffLL) == MVS_OK);
    CHECK(run({1}, 0) == MVS_E_INVALID_ARG && !std::strcmp(g_err, "fn: offs must start at 0"));
    CHECK(run({0, 2, 2, 5}, 0) == MVS_OK && !g_err[0]);
    CHECK(run({0, 3, 2}, 0) == MVS_E_INVALID_ARG && !std::strcmp(g_err, "fn: offs must ascend"));   // a descending pair
    CHECK(run({1, 3, 2}, 0) == MVS_E_INVALID_ARG && !std::strcmp(g_err, "fn: offs must start at 0"));
    CHECK(run({0, 4, 5, 3}, 100) == MVS_E_INVALID_ARG && !std::strcmp(g_err, "fn: offs must ascend"));
    CHECK(run({0, 7, 99}, 100) == MVS_OK && run({0, 7, 100}, 100) == MVS_E_INVALID_ARG && std::strstr(g_err, "fn: offs "));
    CHECK(run({0, 7, 100}, 0) == MVS_OK);
    return 0;
}

static int offsets() {
    if (offsets_of_type<int64_t>() || offsets_of_type<int32_t>()) return 1;
    // the limit every entry uses: 2^31 - 2 items pass, 2^31 - 1 do not
    const std::vector<int64_t> under = {0, 5, 0x7ffffffeLL}, at = {0, 5, 0x7fffffffLL}, over = {0, 5, 0x100000000LL};
    CHECK(check_offsets("fn", "offs", under.data(), 2, 0x7fffffffLL) == MVS_OK);
    CHECK(check_offsets("fn", "offs", at.data(), 2, 0x7fffffffLL) == MVS_E_INVALID_ARG);
    CHECK(check_offsets("fn", "offs", over.data(), 2, 0x7fffffffLL) == MVS_E_INVALID_ARG);
    const std::vector<int32_t> top = {0, 0x7fffffff};
    CHECK(check_offsets("fn", "offs", top.data(), 1, 0x7fffffffLL) == MVS_E_INVALID_ARG && check_offsets("fn", "offs", top.data(), 1) == MVS_OK);
    CHECK(bad("entry", "what went wrong") == MVS_E_INVALID_ARG && !std::strcmp(g_err, "entry: what went wrong"));
    return 0;
}

int main() {
    if (stage1() || offsets()) return 1;
    std::printf("frontend rules ok\n");
    return 0;
}
