// host_parts.h — the one host thread fan-out (engine.h includes it; no HIP in it, so tests/jpeg_rules.cpp runs it as a host program):
// how many threads a piece of host work gets, and fn(part) on that many threads.  Users: the text readers and writers of host_io.cpp,
// the header walk of jpeg.hip, the file readers and writers of api_stitch.cpp.
#ifndef MVS_HOST_PARTS_H_
#define MVS_HOST_PARTS_H_
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

// Threads for `items` independent items of `bytes` bytes in all (IO_UNKNOWN: not known): at most 16, at most one per item and at most one
// per MiB, at least 1.  The cap of 16 is deliberate: hardware_concurrency() reports the whole machine, which a job may hold a small share of.
constexpr int64_t IO_UNKNOWN = -1;
inline int io_threads(int64_t items, int64_t bytes) {
    int64_t n = std::min<int64_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    if (items != IO_UNKNOWN) n = std::min(n, items);
    if (bytes != IO_UNKNOWN) n = std::min(n, bytes >> 20);
    return (int)std::max<int64_t>(1, n);
}
// fn(0) .. fn(parts - 1), one thread each (fn(0) on the caller's), all joined on return; a part reports through what fn captures
inline void parallel_parts(int parts, const std::function<void(int)>& fn) {
    if (parts <= 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int t = 1; t < parts; ++t) th.emplace_back(fn, t);
    fn(0);
    for (auto& x : th) x.join();
}

#endif
