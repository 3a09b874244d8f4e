// render_views.hip — Model2Depth::Run over every camera of every sequence (R/Model2Depth/Model2Depth.cpp:58-190, Model2Depth.h
// SetInput; the call site is Processor::Render, R/Processor/Processor.cpp:1140-1192) as a binned tile rasterizer.  A chunk of
// views takes a fixed number of launches, whatever the number of views in it:
//
//   k_rv_project : one thread per (view, vertex): the sequence's inverse map in fp64 (map34_point, what mvs_srt_apply applies),
//                  narrowed to float as SetInput does, then the vertex stage with the view's own frustum and the shared viewport
//                  w0 x h0 (cameras[0][0]'s size: the window, Reshape's glViewport and glReadPixels of Model2Depth)
//   k_rv_bin     : one thread per (view, triangle): rd_setup's rejects and clamped pixel range; counts (pass 0) or fills
//                  (pass 1, after a scan of the counts) the triangle lists of the RV_TILE x RV_TILE screen tiles the range touches.
//                  A workgroup's entries are counted per tile in LDS first, so a tile's global counter sees one atomic per
//                  workgroup, not one per triangle (the contended form took 2.9 ms per pass at 128 views of 110 k triangles), and
//                  the entries' total goes to a per-view word (one chunk-wide word took 1.1 ms of contended atomics)
//   k_rv_tile    : one workgroup per (view, tile): a float32 depth tile in LDS cleared to 1.0f (glClearDepth), every listed
//                  triangle tested on exactly the pixels of its range inside the tile (rd_pixel), atomicMin on the bit pattern
//                  in LDS (GL_LEQUAL), then RenderDepth's conversion with the row flip, stored a tile row at a time
//
// Bit-exact with render.hip's kernels by construction: the vertex stage, the set-up and each (triangle, pixel) test are the same
// inlines (render_dev.h) over the same pixel set, and the minimum of positive float bit patterns does not depend on the order of
// the lists or of the atomics.  No full-size depth buffer goes to HBM.
#include "engine.h"
#include "dev_common.h"
#include "geom.h"
#include "camera_dev.h"
#include "render_dev.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int TPB = 256;
constexpr int RV_TILE = 32;                          // 32 x 32 pixels: a 4 KiB depth tile, 4 pixels per thread of the output pass
constexpr int64_t RV_LIST_MAX = (int64_t)1 << 28;    // tile-list entries of one chunk (1 GiB; the scan's offsets are int32)
constexpr size_t RV_CHUNK_BYTES = (size_t)256 << 20; // window coordinates + tile counts of one chunk when no bound is set
constexpr int RV_MAX_CHUNK = 65535;                  // grid.y
constexpr int RV_BIN_TILES = 4096;                   // tiles one bin launch counts in LDS (32 KiB with the list bases)

struct ViewDev { GlCam g; int32_t seq, pad; };

__global__ __launch_bounds__(TPB) void k_rv_project(const double* __restrict__ pts, int64_t V, const ViewDev* __restrict__ views,
                                                    const Map34* __restrict__ maps /*NULL: world frame*/, int v0,
                                                    float4* __restrict__ win) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= V) return;
    const ViewDev& vd = views[v0 + (int)blockIdx.y];
    d3 p = ld3(pts + 3 * i);
    if (maps) p = map34_point(maps[vd.seq], p);                                   // Processor.cpp:1183
    win[(int64_t)blockIdx.y * V + i] = rd_window(vd.g, (float)p.x, (float)p.y, (float)p.z);   // SetInput's cast<float>, glVertex3f
}

// The tile lists of the tiles [t_lo, t_lo + t_n) of every view (one launch per such window; one window unless the viewport has more
// than RV_BIN_TILES tiles).  A workgroup first counts its triangles' entries per tile in LDS, then touches the global counter of
// each tile it hit once: FILL == false adds its counts to cnt[view][tile] (and their sum to total[view]); FILL == true (cnt
// zeroed after the scan) reserves a range of the tile's list at off[view][tile] + cnt and places each entry at a slot taken
// from LDS.  A facet with an index outside [0, V) draws nothing (the host entry rejects it; the device entry cannot look).
template <bool FILL>
__global__ __launch_bounds__(TPB) void k_rv_bin(const float4* __restrict__ win, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                                int w, int h, int tx_n, int n_tiles, int t_lo, int t_n, int32_t* __restrict__ cnt,
                                                const int32_t* __restrict__ off, int32_t* __restrict__ list,
                                                unsigned long long* __restrict__ total) {
    extern __shared__ int32_t lds[];                                 // [max(t_n, TPB / 64)] counts, then (FILL) [t_n] list bases
    int32_t* lc = lds;
    int32_t* lb = lds + t_n;
    for (int p = threadIdx.x; p < t_n; p += TPB) lc[p] = 0;
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
    RdTri t;
    bool ok = false;
    if (f < F) {
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const float4* wv = win + (int64_t)blockIdx.y * V;
        ok = a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V && rd_setup(wv[a], wv[b], wv[c], w, h, t);
    }
    const int tx0 = ok ? t.i0 / RV_TILE : 0, tx1 = ok ? t.i1 / RV_TILE : -1, ty0 = ok ? t.j0 / RV_TILE : 0, ty1 = ok ? t.j1 / RV_TILE : -1;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int k = ty * tx_n + tx - t_lo;
            if (k >= 0 && k < t_n) atomicAdd(lc + k, 1);
        }
    __syncthreads();
    int32_t* gc = cnt + (int64_t)blockIdx.y * n_tiles + t_lo;
    if (!FILL) {
        unsigned n = 0;
        for (int p = threadIdx.x; p < t_n; p += TPB) {
            const int32_t c = lc[p];
            if (c) { atomicAdd(gc + p, c); n += (unsigned)c; }
        }
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        __syncthreads();                                             // (lc is read; reuse its first words for the waves' sums)
        if ((threadIdx.x & 63) == 0) lc[threadIdx.x >> 6] = (int32_t)n;
        __syncthreads();
        if (threadIdx.x == 0) {                                      // one atomic per workgroup on its view's total
            unsigned long long sum = 0;
            for (int i = 0; i < TPB / 64; ++i) sum += (unsigned)lc[i];
            if (sum) atomicAdd(total + blockIdx.y, sum);
        }
        return;
    }
    const int32_t* go = off + (int64_t)blockIdx.y * n_tiles + t_lo;
    for (int p = threadIdx.x; p < t_n; p += TPB) {
        const int32_t c = lc[p];
        if (c) lb[p] = go[p] + atomicAdd(gc + p, c);
        lc[p] = 0;
    }
    __syncthreads();
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int k = ty * tx_n + tx - t_lo;
            if (k >= 0 && k < t_n) list[lb[k] + atomicAdd(lc + k, 1)] = (int32_t)f;
        }
}

__global__ __launch_bounds__(TPB) void k_rv_tile(const float4* __restrict__ win, int64_t V, const int32_t* __restrict__ faces,
                                                 const int32_t* __restrict__ off, const int32_t* __restrict__ list,
                                                 const ViewDev* __restrict__ views, int v0, int w, int h, int tx_n, int n_tiles,
                                                 float* __restrict__ out) {
    __shared__ uint32_t zt[RV_TILE * RV_TILE];
    const int tile = blockIdx.x;
    const int x0 = (tile % tx_n) * RV_TILE, y0 = (tile / tx_n) * RV_TILE;
    for (int p = threadIdx.x; p < RV_TILE * RV_TILE; p += TPB) zt[p] = 0x3f800000u;          // glClearDepth(1.0f)
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.y * n_tiles + tile;
    const int32_t e0 = off[k], e1 = off[k + 1];
    const float4* wv = win + (int64_t)blockIdx.y * V;
    for (int32_t e = e0 + (int32_t)threadIdx.x; e < e1; e += TPB) {
        const int64_t f = list[e];
        RdTri t;
        if (!rd_setup(wv[faces[3 * f]], wv[faces[3 * f + 1]], wv[faces[3 * f + 2]], w, h, t)) continue;   // (the bin accepted it)
        const int i0 = max(t.i0, x0), i1 = min(t.i1, x0 + RV_TILE - 1), j0 = max(t.j0, y0), j1 = min(t.j1, y0 + RV_TILE - 1);
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {
                const uint32_t z = rd_pixel(t, i, j);
                if (z != 0xffffffffu) atomicMin(&zt[(j - y0) * RV_TILE + (i - x0)], z);
            }
    }
    __syncthreads();
    const GlCam& g = views[v0 + (int)blockIdx.y].g;
    float* o = out + (int64_t)(v0 + (int)blockIdx.y) * w * h;
    for (int p = threadIdx.x; p < RV_TILE * RV_TILE; p += TPB) {
        const int i = x0 + p % RV_TILE, jz = y0 + p / RV_TILE;
        if (i < w && jz < h) o[(int64_t)(h - 1 - jz) * w + i] = rd_convert(__uint_as_float(zt[p]), g.znear, g.zfar);   // Model2Depth.cpp:134
    }
}

}  // namespace

int render_views_dev(const double* pts, int64_t V, const int32_t* faces, int64_t F, int n_seq, const double* scales, const double* R,
                     const double* t, const int32_t* cam_off, const mvs_camera* cams, float znear, float zfar, float* out, hipStream_t s) {
    const int N = cam_off[n_seq];
    const int w0 = cams[0].w, h0 = cams[0].h;                                        // Model2Depth.h SetInput
    std::vector<ViewDev> hv((size_t)N);
    for (int k = 0; k < n_seq; ++k)
        for (int c = cam_off[k]; c < cam_off[k + 1]; ++c) {
            hv[c].g = make_glcam(cams + c, znear, zfar);                             // the camera's own frustum (Camera.cpp:15-38) ...
            hv[c].g.w = w0; hv[c].g.h = h0;                                          // ... into the shared viewport (Reshape)
            hv[c].seq = k; hv[c].pad = 0;
        }
    std::vector<Map34> hm;
    if (scales)
        for (int k = 0; k < n_seq; ++k) hm.push_back(make_map34(scales[k], R + 9 * k, t + 3 * k, 1));
    const int tx_n = (w0 + RV_TILE - 1) / RV_TILE, ty_n = (h0 + RV_TILE - 1) / RV_TILE, n_tiles = tx_n * ty_n;
    int nv = mvs_render_chunk_views();
    if (nv <= 0) nv = (int)std::max<size_t>(1, RV_CHUNK_BYTES / (sizeof(float4) * (size_t)V + 8 * (size_t)n_tiles));
    nv = std::min(std::min(nv, N), RV_MAX_CHUNK);
    Scratch dv, dm, win, cnt, off, bsum, tot;
    const size_t nslot = (size_t)nv * n_tiles;
    int rc;
    if ((rc = up_async(dv, hv.data(), hv.size(), s)) || (rc = up_async(dm, hm.data(), hm.size(), s)) ||
        (rc = win.alloc(sizeof(float4) * (size_t)nv * V, s)) || (rc = cnt.alloc(sizeof(int32_t) * nslot, s)) ||
        (rc = off.alloc(sizeof(int32_t) * (nslot + 1), s)) || (rc = bsum.alloc(sizeof(int32_t) * ((nslot + 1 + 1023) / 1024), s)) ||
        (rc = tot.alloc(sizeof(unsigned long long) * nv, s))) return rc;
    const Map34* maps = hm.empty() ? nullptr : dm.as<Map34>();
    const unsigned vb = (unsigned)((V + TPB - 1) / TPB), fb = (unsigned)((F + TPB - 1) / TPB);
    for (int v0 = 0; v0 < N;) {
        const int nc = std::min(nv, N - v0);
        const size_t ns = (size_t)nc * n_tiles;
        k_rv_project<<<dim3(vb, nc), dim3(TPB), 0, s>>>(pts, V, dv.as<ViewDev>(), maps, v0, win.as<float4>());
        HIPCHK(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * ns, s));
        HIPCHK(hipMemsetAsync(tot.p, 0, sizeof(unsigned long long) * nc, s));
        for (int t_lo = 0; F && t_lo < n_tiles; t_lo += RV_BIN_TILES) {
            const int t_n = std::min(RV_BIN_TILES, n_tiles - t_lo);
            k_rv_bin<false><<<dim3(fb, nc), dim3(TPB), sizeof(int32_t) * std::max(t_n, TPB / 64), s>>>(win.as<float4>(), V, faces, F, w0, h0, tx_n, n_tiles, t_lo, t_n,
                                                                               cnt.as<int32_t>(), nullptr, nullptr, tot.as<unsigned long long>());
        }
        std::vector<unsigned long long> vt((size_t)nc);
        HIPCHK(hipMemcpyAsync(vt.data(), tot.p, sizeof(unsigned long long) * nc, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        unsigned long long total = 0;
        for (unsigned long long x : vt) total += x;
        if ((int64_t)total > RV_LIST_MAX) {                                          // too many tile entries: halve the chunk, redo it
            if (nc == 1) { mvs_set_error("render_views: one view needs %llu tile entries (at most %lld)", total, (long long)RV_LIST_MAX); return MVS_E_OOM; }
            nv = nc / 2;
            continue;
        }
        scan_exclusive_i32_async(cnt.as<int32_t>(), (int64_t)ns, off.as<int32_t>(), bsum.as<int32_t>(), s);
        Scratch list;
        if ((rc = list.alloc(sizeof(int32_t) * (size_t)total, s))) return rc;
        if (F) HIPCHK(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * ns, s));
        for (int t_lo = 0; F && t_lo < n_tiles; t_lo += RV_BIN_TILES) {
            const int t_n = std::min(RV_BIN_TILES, n_tiles - t_lo);
            k_rv_bin<true><<<dim3(fb, nc), dim3(TPB), 2 * sizeof(int32_t) * t_n, s>>>(win.as<float4>(), V, faces, F, w0, h0, tx_n, n_tiles, t_lo,
                                                                                  t_n, cnt.as<int32_t>(), off.as<int32_t>(), list.as<int32_t>(), nullptr);
        }
        k_rv_tile<<<dim3((unsigned)n_tiles, nc), dim3(TPB), 0, s>>>(win.as<float4>(), V, faces, off.as<int32_t>(), list.as<int32_t>(),
                                                                    dv.as<ViewDev>(), v0, w0, h0, tx_n, n_tiles, out);
        HIPCHK(hipGetLastError());
        v0 += nc;
    }
    HIPCHK(hipStreamSynchronize(s));
    return MVS_OK;
}

// one kernel of this translation unit, for the code-object preload of runtime.cpp (mvs_set_device): asking the runtime for its
// attributes loads the unit's code object without launching anything
const void* mvs_tu_probe_render_views() { return (const void*)k_rv_tile; }
