// overlay_rules.h — rules O1-O6 of include/mvs.h (the match and SIFT overlay pictures): every decision as one __host__ __device__
// body — what a primitive must look like (O2, O5), whether it covers a pixel (O3), the record the kernel keeps of it in LDS, the
// conservative test of a primitive against a 16 x 16 tile, cvRound of a float, and the generator of O6 with the three primitives of one
// match.  The kernel of overlay.hip runs this body; tests/overlay_rules.cpp runs it as a host program of its own, tests/ref_overlay.py
// restates O1-O6 by painting primitive after primitive.  The rules are RECALLED from OpenCV 3.0's drawing.cpp and cv::RNG and NOT
// VERIFIED against it.  All coverage arithmetic is int64_t and exact; the bounds stand next to it.
#ifndef MVS_OVERLAY_RULES_H_
#define MVS_OVERLAY_RULES_H_
#include <math.h>
#include <stdint.h>

constexpr int OVL_DISC = 0, OVL_RING = 1, OVL_SEGMENT = 2;           // MVS_DRAW_DISC, MVS_DRAW_RING, MVS_DRAW_SEGMENT
constexpr int OVL_MAX_DIM = 16384;                                    // O1: 1 <= w, h <= 16384
constexpr int OVL_MAX_COORD = 1 << 20;                                // O5: |coordinate| of a disc or ring centre
constexpr int OVL_TILE = 16, OVL_CHUNK = OVL_TILE * OVL_TILE;         // a workgroup's tile; primitives it tests at a time

struct OvlPrim {                       // struct mvs_draw_prim, 24 bytes
    int32_t x0, y0, x1, y1;
    uint8_t kind, size, c[3], pad[3];
};
static_assert(sizeof(OvlPrim) == 24, "mvs_draw_prim is 24 bytes");

// O2, O5: NULL, or what is wrong with q on a w x h canvas
__host__ __device__ inline const char* ovl_prim_error(const OvlPrim& q, int32_t w, int32_t h) {
    if (q.kind == OVL_SEGMENT) {
        if (q.size < 1) return "a segment needs a thickness of 1 .. 255";
        if (q.x0 < 0 || q.x0 >= w || q.x1 < 0 || q.x1 >= w || q.y0 < 0 || q.y0 >= h || q.y1 < 0 || q.y1 >= h)
            return "a segment end lies outside the canvas";
        return nullptr;
    }
    if (q.kind != OVL_DISC && q.kind != OVL_RING) return "kind must be MVS_DRAW_DISC, MVS_DRAW_RING or MVS_DRAW_SEGMENT";
    if (q.x0 < -OVL_MAX_COORD || q.x0 > OVL_MAX_COORD || q.y0 < -OVL_MAX_COORD || q.y0 > OVL_MAX_COORD)
        return "a disc or ring centre lies outside +-2^20";
    return nullptr;
}

// what a pixel test reads of a primitive: the constants of O3 formed once
struct OvlRec {
    int32_t x0, y0, dx, dy;            // A, and d = B - A of a segment
    int64_t L2, lim;                   // segment: d.d and T^2 d.d
    int32_t hi, lo;                    // disc, ring: lo < dx^2 + dy^2 <= hi; segment: hi = T^2
    uint8_t kind, c[3];
    uint8_t pad[4];
};
static_assert(sizeof(OvlRec) == 48, "the LDS record is 48 bytes");

__host__ __device__ inline OvlRec ovl_record(const OvlPrim& q) {
    OvlRec r;
    const int32_t s = q.size;
    r.x0 = q.x0; r.y0 = q.y0;
    r.kind = q.kind; r.c[0] = q.c[0]; r.c[1] = q.c[1]; r.c[2] = q.c[2];
    r.pad[0] = r.pad[1] = r.pad[2] = r.pad[3] = 0;
    r.hi = s * s;                                                      // <= 255^2
    r.lo = (q.kind == OVL_RING && s > 0) ? (s - 1) * (s - 1) : -1;     // ring of r = 0: the centre pixel
    r.dx = r.dy = 0; r.L2 = r.lim = 0;
    if (q.kind == OVL_SEGMENT) {
        r.dx = q.x1 - q.x0; r.dy = q.y1 - q.y0;                        // |d| < 2^14: both ends are inside the canvas (O5)
        r.L2 = (int64_t)r.dx * r.dx + (int64_t)r.dy * r.dy;            // < 2^29
        r.lim = (int64_t)r.hi * r.L2;                                  // < 2^16 2^29 = 2^45
    }
    return r;
}

// O3: does the primitive of r cover pixel (x, y) of its canvas, 0 <= x, y < 16384
__host__ __device__ inline bool ovl_hit(const OvlRec& r, int32_t x, int32_t y) {
    const int64_t ex = (int64_t)x - r.x0, ey = (int64_t)y - r.y0;     // disc, ring: |e| < 2^20 + 2^14; segment: < 2^14
    const int64_t d2 = ex * ex + ey * ey;                             // < 2^43; segment: < 2^29
    if (r.kind != OVL_SEGMENT) return d2 <= r.hi && d2 > r.lo;
    const int64_t s = ex * r.dx + ey * r.dy;                          // |s| < 2^29
    if (s <= 0) return 4 * d2 <= r.hi;                                // the cap at A; A == B ends here: a disc of diameter T
    if (s >= r.L2) {
        const int64_t fx = ex - r.dx, fy = ey - r.dy;                 // p - B
        return 4 * (fx * fx + fy * fy) <= r.hi;
    }
    const int64_t cr = ex * r.dy - ey * r.dx;                         // |cr| < 2^29, so 4 cr^2 < 2^60 < 2^62
    return 4 * cr * cr <= r.lim;
}

// May q cover a pixel of the 16 x 16 tile whose first pixel is (tx0, ty0)?  Never false for a covering primitive: a covered pixel is
// within half a diagonal, hd = 7.5 sqrt 2, of the tile's centre c = (tx0 + 7.5, ty0 + 7.5), so c is within size / 2 + hd of the segment
// (size + hd of a disc's centre).  In doubled coordinates, integers: 2 hd = 15 sqrt 2 and (T + 15 sqrt 2)^2 = T^2 + 30 sqrt 2 T + 450 <=
// T^2 + 43 T + 450; (2 r + 15 sqrt 2)^2 <= 4 r^2 + 85 r + 450.  A ring is also dropped when every pixel of the tile lies in its hole:
// |c - C| + hd <= r - 1, which 2 |c - C| <= 2 (r - 1) - 22 implies.  The test is the exact distance of c to the segment, so a long
// diagonal reaches only the tiles along it, not those of its bounding box.
__host__ __device__ inline bool ovl_tile_may(const OvlPrim& q, int32_t tx0, int32_t ty0) {
    const int64_t cx = 2 * (int64_t)tx0 + 15 - 2 * (int64_t)q.x0, cy = 2 * (int64_t)ty0 + 15 - 2 * (int64_t)q.y0;   // 2 (c - A), |.| < 2^22
    const int64_t s = q.size, D2 = cx * cx + cy * cy;                 // < 2^45
    if (q.kind != OVL_SEGMENT) {
        if (D2 > 4 * s * s + 85 * s + 450) return false;
        if (q.kind == OVL_RING && 2 * (s - 1) >= 22) {
            const int64_t in = 2 * (s - 1) - 22;
            if (D2 <= in * in) return false;
        }
        return true;
    }
    const int64_t R2 = s * s + 43 * s + 450;                          // < 2^17
    const int64_t dx = (int64_t)q.x1 - q.x0, dy = (int64_t)q.y1 - q.y0, L2 = dx * dx + dy * dy;   // |d| < 2^14, L2 < 2^29
    const int64_t dot = cx * dx + cy * dy;                            // 2 (c - A).d; segment ends are inside the canvas: |cx| < 2^16
    if (dot <= 0) return D2 <= R2;
    if (dot >= 2 * L2) {
        const int64_t fx = cx - 2 * dx, fy = cy - 2 * dy;             // 2 (c - B)
        return fx * fx + fy * fy <= R2;
    }
    const int64_t cr = cx * dy - cy * dx;                             // |cr| < 2^31, cr^2 < 2^62
    return cr * cr <= R2 * L2;                                        // R2 L2 < 2^46
}

// cvRound of a cv::Point2f coordinate: round half to even.  NaN and anything outside int32 give INT_MIN, as cvt_i32 (camera_dev.h)
// does for the truncating conversion; a mark there is clipped away
__host__ __device__ inline int32_t ovl_round_i32(float f) {
    const double x = (double)f;
    if (!(x > -2147483649.0 && x < 2147483648.0)) return (int32_t)0x80000000;
    const double fl = floor(x), frac = x - fl;                        // exact: x is a float
    int32_t i = (int32_t)fl;                                          // a float with a fraction is below 2^23: i + 1 cannot overflow
    if (frac > 0.5 || (frac == 0.5 && (i & 1))) ++i;
    return i;
}

// ---------------------------------------------------------------- O6 ----
constexpr uint64_t OVL_RNG_DEFAULT = 0xffffffffull;                   // cv::RNG()
__host__ __device__ inline uint32_t ovl_rng_next(uint64_t* state) {
    *state = (uint64_t)(uint32_t)*state * 4164903690u + (*state >> 32);
    return (uint32_t)*state;
}
__host__ __device__ inline double ovl_rng_double(uint64_t* state) {  // rng.uniform(0.0, 1.0): the high word is drawn first
    const uint64_t hi = ovl_rng_next(state);
    const uint64_t lo = ovl_rng_next(state);
    return (double)((hi << 32) | lo) * 5.4210108624275221700372640043497e-20;
}
// the line colour of one match: r, g, b drawn in this order, each (uchar)(double * 255); bgr receives (b, g, r)
__host__ __device__ inline void ovl_rng_colour(uint64_t* state, uint8_t* bgr) {
    const uint8_t r = (uint8_t)(ovl_rng_double(state) * 255);
    const uint8_t g = (uint8_t)(ovl_rng_double(state) * 255);
    const uint8_t b = (uint8_t)(ovl_rng_double(state) * 255);
    bgr[0] = b; bgr[1] = g; bgr[2] = r;
}

__host__ __device__ inline OvlPrim ovl_prim(int kind, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int size, uint8_t c0, uint8_t c1, uint8_t c2) {
    OvlPrim q;
    q.x0 = x0; q.y0 = y0; q.x1 = x1; q.y1 = y1;
    q.kind = (uint8_t)kind; q.size = (uint8_t)size;
    q.c[0] = c0; q.c[1] = c1; q.c[2] = c2;
    q.pad[0] = q.pad[1] = q.pad[2] = 0;
    return q;
}
// Processor.cpp:783-785 on the stacked canvas (the second image starts at row h): ring, ring, segment of one match (u1, v1, u2, v2) into
// out[0..2].  line: the colour of ovl_rng_colour; swap: the canvas is R G B, so both colours are written the other way round
__host__ __device__ inline void ovl_match_prims(const int32_t* m, int32_t h, const uint8_t* line, bool swap, OvlPrim* out) {
    const uint8_t r0 = swap ? 0 : 255, r2 = swap ? 255 : 0;           // cv::Scalar(255, 255, 0) in B G R
    out[0] = ovl_prim(OVL_RING, m[0], m[1], 0, 0, 1, r0, 255, r2);
    out[1] = ovl_prim(OVL_RING, m[2], h + m[3], 0, 0, 1, r0, 255, r2);
    out[2] = ovl_prim(OVL_SEGMENT, m[0], m[1], m[2], h + m[3], 2, line[swap ? 2 : 0], line[1], line[swap ? 0 : 2]);
}
#endif
