// Host worker threads of the pipelines (pipeline.cpp, stack_pipeline.cpp): one rule for how many, one loop that hands out items.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <thread>
#include <vector>

namespace tmat {

// workers for k independent items: the machine's hardware threads, or TMAT_HOST_THREADS when set (compute_branches.py shares the cores
// between the ranks through it), never more than k
inline int n_workers(int k)
{
    int hw = (int)std::thread::hardware_concurrency();
    if (hw <= 0) hw = 4;
    const char *e = getenv("TMAT_HOST_THREADS");
    if (e && atoi(e) > 0) hw = atoi(e);
    return std::max(1, std::min(hw, k));
}

template <class F>
inline void parallel_images(int k, F f)
{
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    const int nt = n_workers(k);
    for (int t = 0; t < nt; t++)
        th.emplace_back([&]() { for (;;) { const int i = next.fetch_add(1); if (i >= k) break; f(i); } });
    for (auto &t : th) t.join();
}

}  // namespace tmat
