// host_threads.h -- how the host-side row routines split their rows over threads (csrc/host_rows.hip, the host twin of
// csrc/rows_remap.hip).  No device code.
#pragma once
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

namespace gsx {

inline int worker_count(int64_t bytes)
{
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t by_size = bytes / (8LL << 20) + 1;  // ~8 MiB of traffic per thread at least
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(hw ? hw : 8), 64, by_size}));
}

template <class F>
void run_threads(int nt, F &&body)  // body(t) for t in [0, nt); the caller is thread 0
{
    std::vector<std::thread> th;
    th.reserve(nt > 1 ? nt - 1 : 0);
    for (int t = 1; t < nt; ++t) th.emplace_back([&body, t] { body(t); });
    body(0);
    for (auto &x : th) x.join();
}

}  // namespace gsx
