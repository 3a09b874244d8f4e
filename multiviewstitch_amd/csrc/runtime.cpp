// runtime.cpp — process-wide state of libmvs_hip: the error text, the current device, the cold-start preload, tracing, the device
// queries of the C-ABI, need_device, the stream pool of the deformation handles and the scratch pool of the host-driven entries.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/mvs.h"
#include "engine.h"
#include "knobs.h"
#include "trace.h"

// ------------------------------------------------------------------ errors ----
static thread_local char g_err[512] = "";
static int g_device = 0;

void mvs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
int mvs_check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return MVS_OK;
    mvs_set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
    return e == hipErrorOutOfMemory ? MVS_E_OOM : MVS_E_HIP;
}
int mvs_current_device() { return g_device; }
int mvs_debug_level() {
    static const int level = [] { const char* e = getenv("MVS_DEBUG_CG"); return (e && *e) ? (e[0] == '2' ? 2 : 1) : 0; }();
    return level;
}

// ---- cold start ----
// The reference's process calls Processor::Deform ONCE (R/main.cpp:24-25): what a drop-in caller sees is the COLD call.  Two
// things a first call pays that later ones do not: the runtime loads each translation unit's code object at the first use of one
// of its kernels (twelve units), and the first stream of a process is a new hardware queue (hipStreamCreate: 5.7 ms, measured).
// Both need nothing from the caller: a helper thread does them — once per device — as soon as the device is known
// (mvs_set_device, or the first deformation entry), while the host reads its files; the thread is detached and touches only the
// runtime and the stream pool (mutex).  mvs_preload_wait (mvs_test.h) joins the work, for measurements.
const void* const* mvs_tu_kernels_grid(int*); const void* const* mvs_tu_kernels_assoc(int*); const void* const* mvs_tu_kernels_knn(int*);
const void* const* mvs_tu_kernels_arap(int*); const void* const* mvs_tu_kernels_schwarz(int*); const void* const* mvs_tu_kernels_meshbuild(int*);
const void* const* mvs_tu_kernels_geom(int*); const void* const* mvs_tu_kernels_depth_sgm(int*);
const void* mvs_tu_probe_srt(); const void* mvs_tu_probe_align(); const void* mvs_tu_probe_consist(); const void* mvs_tu_probe_render();
const void* mvs_tu_probe_stitch(); const void* mvs_tu_probe_render_views(); const void* mvs_tu_probe_matchpairs(); const void* mvs_tu_probe_views();
const void* mvs_tu_probe_siftmatch(); const void* mvs_tu_probe_sift(); const void* mvs_tu_probe_pointsample(); const void* mvs_tu_probe_compact();
const void* mvs_tu_probe_grabcut();
// (never destroyed: the helper thread is detached and may outlive the static destructors of an exiting process)
static std::mutex& g_preload_mu = *new std::mutex;
static std::condition_variable& g_preload_cv = *new std::condition_variable;
static std::vector<int>& g_preload_started = *new std::vector<int>;
static std::vector<int>& g_preload_done = *new std::vector<int>;
void mvs_preload(int device) {
    {
        std::lock_guard<std::mutex> lk(g_preload_mu);
        for (int d : g_preload_started) if (d == device) return;
        g_preload_started.push_back(device);
    }
    std::thread([device] {
        if (hipSetDevice(device) == hipSuccess) {
            // the deformation path first, every kernel of it (a kernel's first launch otherwise pays its own resolution: the first
            // outer iteration of a fresh process took 5.6-7.5 ms against 0.8 ms warm with only the code objects loaded), in the
            // order a fit meets the units; then one kernel of each remaining unit; last, behind everything a fit or an older
            // stage waits for, the kernels of the aggregated depth recovery (depth_sgm.hip; what these nine resolutions cost the thread has
            // not been measured)
            stream_pool_prime(device);
            for (auto unit : {mvs_tu_kernels_meshbuild, mvs_tu_kernels_knn, mvs_tu_kernels_grid, mvs_tu_kernels_assoc, mvs_tu_kernels_arap, mvs_tu_kernels_schwarz,
                              mvs_tu_kernels_geom}) {
                int n = 0;
                const void* const* ks = unit(&n);
                for (int i = 0; i < n; ++i) { hipFuncAttributes a; if (hipFuncGetAttributes(&a, ks[i]) != hipSuccess) (void)hipGetLastError(); }
            }
            for (const void* k : {mvs_tu_probe_srt(), mvs_tu_probe_align(), mvs_tu_probe_consist(), mvs_tu_probe_render(),
                                  mvs_tu_probe_stitch(), mvs_tu_probe_render_views(), mvs_tu_probe_matchpairs(), mvs_tu_probe_views(),
                                  mvs_tu_probe_siftmatch(), mvs_tu_probe_sift(), mvs_tu_probe_pointsample(), mvs_tu_probe_compact(), mvs_tu_probe_grabcut()}) {
                hipFuncAttributes a;
                if (hipFuncGetAttributes(&a, k) != hipSuccess) (void)hipGetLastError();
            }
            int n = 0;
            const void* const* ks = mvs_tu_kernels_depth_sgm(&n);
            for (int i = 0; i < n; ++i) { hipFuncAttributes a; if (hipFuncGetAttributes(&a, ks[i]) != hipSuccess) (void)hipGetLastError(); }
        }
        std::lock_guard<std::mutex> lk(g_preload_mu);
        g_preload_done.push_back(device);
        g_preload_cv.notify_all();
    }).detach();
}
void mvs_preload_join(int device) {
    std::unique_lock<std::mutex> lk(g_preload_mu);
    bool started = false;
    for (int d : g_preload_started) started = started || d == device;
    if (!started) return;
    g_preload_cv.wait(lk, [&] { for (int d : g_preload_done) if (d == device) return true; return false; });
}

// ---- tracing (trace.h) ----
static mvs_trace_fn g_trace_fn = nullptr;
static void* g_trace_ctx = nullptr;
static int (*g_roctx_push)(const char*) = nullptr;
static int (*g_roctx_pop)() = nullptr;
static bool g_roctx_on = false;
bool mvs_trace_on() { return g_trace_fn != nullptr || g_roctx_on; }
void mvs_trace_enter(const char* entry) {
    if (g_roctx_on && g_roctx_push) (void)g_roctx_push(entry);
    if (g_trace_fn) g_trace_fn(g_trace_ctx, entry, 0, 0.0);
}
void mvs_trace_leave(const char* entry, double host_ms) {
    if (g_trace_fn) g_trace_fn(g_trace_ctx, entry, 1, host_ms);
    if (g_roctx_on && g_roctx_pop) (void)g_roctx_pop();
}

extern "C" {

int mvs_set_trace(mvs_trace_fn fn, void* ctx) { g_trace_ctx = ctx; g_trace_fn = fn; return MVS_OK; }
int mvs_set_trace_roctx(int on) {
    if (on && !g_roctx_push) {
        void* lib = nullptr;
        for (const char* name : {"libroctx64.so.4", "libroctx64.so", "/opt/rocm/lib/libroctx64.so", "librocprofiler-sdk-roctx.so"}) { lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (lib) { g_roctx_push = (int (*)(const char*))dlsym(lib, "roctxRangePushA"); g_roctx_pop = (int (*)())dlsym(lib, "roctxRangePop"); }
        if (!g_roctx_push || !g_roctx_pop) { g_roctx_push = nullptr; g_roctx_pop = nullptr; mvs_set_error("roctx is not available on this host"); return MVS_E_STATE; }
    }
    g_roctx_on = on != 0;
    return MVS_OK;
}

const char* mvs_last_error(void) { return g_err; }
int mvs_abi_version(void) { return MVS_ABI_VERSION; }
int mvs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
int mvs_set_device(int device) {
    if (device < 0 || device >= mvs_device_count()) { mvs_set_error("no such device %d", device); return MVS_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(device));
    g_device = device;
    mvs_preload(device);
    return MVS_OK;
}
int mvs_device_name(char* buf, int buflen) {
    if (!buf || buflen <= 0) return MVS_E_INVALID_ARG;
    if (mvs_device_count() == 0) { mvs_set_error("no HIP device"); return MVS_E_NO_DEVICE; }
    hipDeviceProp_t pr;
    HIPCHK(hipGetDeviceProperties(&pr, g_device));
    snprintf(buf, buflen, "%s (%s)", pr.name, pr.gcnArchName);
    return MVS_OK;
}

}  // extern "C"

// HIP's current device is per thread: every compute entry selects the library's device on the thread that calls it
int need_device() {
    if (mvs_device_count() == 0) { mvs_set_error("no HIP device: the MI355X engine has no CPU fallback"); return MVS_E_NO_DEVICE; }
    return mvs_check_hip(hipSetDevice(g_device), "hipSetDevice");
}

// ------------------------------------------------------------------ stream pool ----
// Streams of destroyed handles are kept for the next handle: hipStreamCreate is the most expensive call of a cold
// mvs_deform_create on this runtime (5.7 ms for a new hardware queue, measured; the whole device-side mesh build is < 1 ms).
// A released stream has been synchronised by mvs_deform_destroy.  At most 64 idle streams are kept per process.
namespace {
struct PooledStream { int device; hipStream_t s; };
// (never destroyed: the detached preload thread may push into it during process teardown)
std::mutex& g_pool_mutex = *new std::mutex;
std::vector<PooledStream>& g_pool = *new std::vector<PooledStream>;
}  // namespace
int stream_acquire(int device, hipStream_t* out) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        for (size_t i = 0; i < g_pool.size(); ++i)
            if (g_pool[i].device == device) { *out = g_pool[i].s; g_pool.erase(g_pool.begin() + i); return MVS_OK; }
    }
    return mvs_check_hip(hipStreamCreateWithFlags(out, hipStreamNonBlocking), "hipStreamCreate");
}
// (cold start: one stream in the pool before the first handle asks for it)
void stream_pool_prime(int device) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        for (const PooledStream& p : g_pool) if (p.device == device) return;
    }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return; }
    // the runtime's own fill / copy kernels and staging paths are loaded at their first use too (hipMemsetAsync, device-to-device
    // and strided device-to-host copies: what a pass and its harvest enqueue): one use of each on a scratch buffer
    {
        void *d = nullptr, *hp = nullptr;
        if (hipMalloc(&d, 1 << 16) == hipSuccess && hipHostMalloc(&hp, 1 << 12, hipHostMallocDefault) == hipSuccess) {
            (void)hipMemsetAsync(d, 0, 1 << 16, s);
            (void)hipMemsetAsync((char*)d + 4, 0, 4, s);
            (void)hipMemcpyAsync((char*)d + (1 << 15), d, 1 << 14, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpy2DAsync(hp, 64, d, 1024, 64, 32, hipMemcpyDeviceToHost, s);
            (void)hipMemcpyAsync(hp, d, 256, hipMemcpyDeviceToHost, s);
            (void)hipMemcpyAsync(d, hp, 256, hipMemcpyHostToDevice, s);
            char pageable[256] = {0};
            (void)hipMemcpyAsync(pageable, d, sizeof pageable, hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            (void)hipMemcpyAsync(d, pageable, sizeof pageable, hipMemcpyHostToDevice, s);
            (void)hipStreamSynchronize(s);
        }
        if (d) (void)hipFree(d);
        if (hp) (void)hipHostFree(hp);
        (void)hipGetLastError();
    }
    // ... and a second stream: a process that holds two handles at once (bench.py's reference-schedule leg beside its main handle)
    // otherwise meets the 5.7 ms of a new hardware queue at the second handle's creation
    hipStream_t s2 = nullptr;
    if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s2 = nullptr; }
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    g_pool.push_back({device, s});
    if (s2) g_pool.push_back({device, s2});
}
void stream_release(int device, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        if (g_pool.size() < 64) { g_pool.push_back({device, s}); return; }
    }
    (void)hipStreamDestroy(s);
}

// ------------------------------------------------------------------ host table of sample_nodes ----
// The host half of mvs_deform_sample_nodes' kNN table (its device half is a block of the scratch pool below): ordinary (CPU-cached,
// pageable) memory — the greedy pass READS the table on the host, and from hipHostMalloc memory that pass took 1.7 ms instead of
// 0.5 (registering malloc'ed memory did not help: EXPERIMENTS r3-25).  A fresh Deformation per Deform call (the reference's
// pattern) asks for the same size again and again: one idle block, the larger one, is kept.
namespace {
struct HostSlot { std::mutex m; void* p = nullptr; size_t bytes = 0; };
HostSlot& host_slot() { static HostSlot* s = new HostSlot; return *s; }   // (never destroyed, as above)
}  // namespace
int host_table_acquire(size_t bytes, void** out) {
    HostSlot& S = host_slot();
    {
        std::lock_guard<std::mutex> lk(S.m);
        if (S.p && S.bytes >= bytes) { *out = S.p; S.p = nullptr; S.bytes = 0; return MVS_OK; }
    }
    *out = std::malloc(bytes);
    if (!*out) { mvs_set_error("out of host memory"); return MVS_E_OOM; }
    return MVS_OK;
}
void host_table_release(void* p, size_t bytes) {
    if (!p) return;
    HostSlot& S = host_slot();
    {
        std::lock_guard<std::mutex> lk(S.m);
        if (S.bytes < bytes) { std::swap(S.p, p); std::swap(S.bytes, bytes); }     // keep the larger one
    }
    std::free(p);
}

// ------------------------------------------------------------------ scratch pool ----
// Scratch pool of the host-driven entries (Alignment, SRT, depth, files' device halves) and of sample_nodes' kNN table: a call of
// mvs_align on a 2 M-vertex scan makes ~40 device allocations, and hipFree alone was 4.3 of its 10 ms (rocprofv3 --hip-trace,
// profiles/r04/align_dev_hip_stats.csv: 115 us per hipFree).  Blocks handed back are kept per device and given to the next
// request of a similar size.  Entries hold their blocks as a Scratch (engine.h).
//
// Ordering rule (why a cached block can be handed out at once): a block goes back to the pool only behind its last use.  A block
// that was allocated for a caller's stream (`user`) is handed back by mvs_scratch_free(p, user), which synchronises that stream
// first: on an entry's success path the entry has already waited for it and this wait is free, on an early return it is what
// keeps the kernels still queued there off the block.  A block of the LEGACY default stream goes back at once, behind its last
// use in that stream's order (Alignment's stages free scratch whose kernels are still queued there).  The next user on the legacy
// default stream is ordered behind that by the stream itself; a user that names another stream gets that stream ordered behind
// everything the legacy stream has been given so far (one event) before it receives a cached block.  The deformation handles
// have their own arenas.  MVS_SCRATCH_CACHE_MB (default 4096; 0 = no caching) bounds what is kept; mvs_trim() releases it.
namespace {
struct Pool {
    std::mutex m;
    std::multimap<size_t, void*> idle[MVS_MAX_DEVICES];
    struct Info { size_t bytes; int dev; };
    std::unordered_map<void*, Info> out;               // blocks in use
    size_t kept = 0, cap = (size_t)4096 << 20;
    bool cap_read = false;
    hipEvent_t fence[MVS_MAX_DEVICES] = {};             // "everything the legacy stream has been given" (created on first use)
};
Pool& pool() { static Pool* p = new Pool; return *p; }   // (never destroyed: entries may run during process teardown)
size_t round_up(size_t b) {
    if (b < 4096) return 4096;
    size_t g = 4096;                                     // granule = 1/8 of the size's power of two: at most 12.5 % over
    while ((g << 4) <= b) g <<= 1;
    return (b + g - 1) / g * g;
}
}  // namespace

int mvs_scratch_alloc(void** p, size_t bytes, hipStream_t user) {
    Pool& P = pool();
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const size_t need = round_up(bytes);
    {
        std::lock_guard<std::mutex> g(P.m);
        if (!P.cap_read) {
            if (const char* e = std::getenv("MVS_SCRATCH_CACHE_MB")) P.cap = (size_t)std::strtoull(e, nullptr, 10) << 20;
            P.cap_read = true;
        }
        if (dev >= 0 && dev < MVS_MAX_DEVICES) {
            auto it = P.idle[dev].lower_bound(need);
            if (it != P.idle[dev].end() && it->first <= need + need / 4 + ((size_t)1 << 20)) {
                if (user) {                                      // (under the lock: one event per device, recorded and waited for in one go)
                    if (!P.fence[dev]) HIPCHK(hipEventCreateWithFlags(&P.fence[dev], hipEventDisableTiming));
                    HIPCHK(hipEventRecord(P.fence[dev], nullptr));
                    HIPCHK(hipStreamWaitEvent(user, P.fence[dev], 0));
                }
                *p = it->second;
                P.out[*p] = {it->first, dev};
                P.kept -= it->first;
                P.idle[dev].erase(it);
                return MVS_OK;
            }
        }
    }
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) {                               // out of memory with blocks kept: give them back and try once more
        (void)hipGetLastError();
        mvs_trim();
        e = hipMalloc(p, need);
    }
    int rc = mvs_check_hip(e, "hipMalloc");
    if (rc) { *p = nullptr; return rc; }
    std::lock_guard<std::mutex> g(P.m);
    P.out[*p] = {need, dev};
    return MVS_OK;
}

// read at every call, so that a test can bound the chunks of one call (the results do not depend on them)
int mvs_render_chunk_views() {
    const char* e = std::getenv("MVS_RENDER_CHUNK_VIEWS");
    const int n = (e && *e) ? std::atoi(e) : 0;
    return n > 0 ? n : 0;
}

// read at every call, like MVS_RENDER_CHUNK_VIEWS: a test can send small buckets through the workspace path of matchpairs.hip (the
// variable only LOWERS the capacity; the results do not depend on it)
int mvs_match_pairs_lds_cap() {
    const char* e = std::getenv("MVS_MATCH_PAIRS_LDS_CAP");
    const int n = (e && *e) ? std::atoi(e) : 0;
    return (n > 0 && n < MVS_MATCH_PAIRS_LDS_KEYS) ? n : MVS_MATCH_PAIRS_LDS_KEYS;
}

void mvs_scratch_free(void* p, hipStream_t user) {
    if (!p) return;
    if (user && hipStreamSynchronize(user) != hipSuccess) (void)hipGetLastError();   // (the entry has reported its own error)
    Pool& P = pool();
    {
        std::lock_guard<std::mutex> g(P.m);
        auto it = P.out.find(p);
        if (it != P.out.end()) {
            const Pool::Info info = it->second;
            P.out.erase(it);
            if (info.dev >= 0 && info.dev < MVS_MAX_DEVICES && P.kept + info.bytes <= P.cap) {
                P.idle[info.dev].emplace(info.bytes, p);
                P.kept += info.bytes;
                return;
            }
        }
    }
    (void)hipFree(p);
}

extern "C" int mvs_trim(void) {
    Pool& P = pool();
    std::multimap<size_t, void*> take[MVS_MAX_DEVICES];
    {
        std::lock_guard<std::mutex> g(P.m);
        for (int d = 0; d < MVS_MAX_DEVICES; ++d) take[d].swap(P.idle[d]);
        P.kept = 0;
    }
    int cur = 0, rc = MVS_OK;
    bool have = false;
    for (int d = 0; d < MVS_MAX_DEVICES; ++d) {
        if (take[d].empty()) continue;
        if (!have) { (void)hipGetDevice(&cur); have = true; }
        (void)hipSetDevice(d);
        for (auto& kv : take[d]) if (hipFree(kv.second) != hipSuccess) rc = MVS_E_HIP;
    }
    if (have) (void)hipSetDevice(cur);
    return rc;
}
