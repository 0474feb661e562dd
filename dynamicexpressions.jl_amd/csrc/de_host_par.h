// de_host_par.h — per-tree passes on the pool of host threads (de_api.cpp): what the host-only translation units (de_grad_encode.cpp) and
// the C ABI's (de_api_internal.h) share.  No HIP header, no context: the pool's two entry points and the templates built on them.
#ifndef DE_HOST_PAR_H
#define DE_HOST_PAR_H
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

extern "C" {
// the pool of host threads (de_api.cpp): job(k) for k = 0 .. n - 1 on the pool (false: busy, nothing was run); threads a pass of n items gets
bool host_pool_run(int n, const std::function<void(int)> &job);
unsigned host_threads_for(int64_t n, int64_t grain);
}

constexpr int HOST_RANGES_MAX = 32; // ranges of one parallel pass (per-worker vectors are arrays of this size)

// The trees in contiguous ranges, one per worker: f(k, b, e) with k < HOST_RANGES_MAX — for passes that append to a per-worker vector which is
// concatenated afterwards, or that write disjoint slices of pre-sized vectors.  The partition depends on n and the thread count only.
template <class F> static void parallel_tree_ranges(int64_t n, F f, int64_t grain = 0) {
    const unsigned nt = host_threads_for(n, grain);
    if (nt <= 1) {
        f(0, (int64_t)0, n);
        return;
    }
    const int64_t per = (n + nt - 1) / nt;
    const int n_ranges = (int)((n + per - 1) / per);
    const std::function<void(int)> job = [&](int k) {
        const int64_t b = (int64_t)k * per, e = std::min<int64_t>(n, b + per);
        if (b < e) f(k, b, e);
    };
    if (!host_pool_run(n_ranges, job))
        for (int k = 0; k < n_ranges; k++) job(k);
}
template <class F> static void parallel_for_trees(int64_t n, F f, int64_t grain = 0) {
    parallel_tree_ranges(n, [&](int, int64_t b, int64_t e) { for (int64_t i = b; i < e; i++) f(i); }, grain);
}

// A per-tree pass that APPENDS records: every worker fills a vector of its own over its range of trees (emit(t, &out)), the pieces are
// concatenated in tree order and off[t] .. off[t + 1] names tree t's records — the stream a serial loop over the trees would have built.
template <class Rec, class Emit>
static void build_stream_by_trees(int64_t n_trees, std::vector<Rec> *stream, std::vector<int32_t> *off, Emit emit) {
    std::vector<Rec> parts[HOST_RANGES_MAX];
    int64_t first[HOST_RANGES_MAX], last[HOST_RANGES_MAX];
    for (int k = 0; k < HOST_RANGES_MAX; k++) first[k] = last[k] = 0;
    std::vector<int32_t> cnt((size_t)n_trees, 0);
    parallel_tree_ranges(n_trees, [&](int k, int64_t tb, int64_t te) {
        std::vector<Rec> &out = parts[k];
        first[k] = tb;
        last[k] = te;
        for (int64_t t = tb; t < te; t++) {
            const size_t before = out.size();
            emit(t, &out);
            cnt[(size_t)t] = (int32_t)(out.size() - before);
        }
    });
    off->assign((size_t)n_trees + 1, 0);
    for (int64_t t = 0; t < n_trees; t++) (*off)[(size_t)t + 1] = (*off)[(size_t)t] + cnt[(size_t)t];
    stream->clear();
    stream->resize((size_t)(*off)[(size_t)n_trees]);
    for (int k = 0; k < HOST_RANGES_MAX; k++) // (a few MB: memcpy-bound, kept serial)
        if (last[k] > first[k] && !parts[k].empty())
            std::memcpy(static_cast<void *>(stream->data() + (*off)[(size_t)first[k]]), parts[k].data(), parts[k].size() * sizeof(Rec));
}

#endif
