// dl4ds_amd -- host bookkeeping shared by the 3x3 convolution kernels: the per-stream scratch buffer, the graph-pass state and
// the cache of the operands DERIVED from a layer's filter (Winograd transforms: conv_wino.hip; bf16 fragments: conv_split.hip).
#pragma once
#include "common.h"
#include <algorithm>
#include <mutex>
#include <vector>

// Grow-only scratch, one buffer per stream (launches on a stream are ordered).  A buffer that is too small is replaced, after the
// stream has drained, by one of exactly the requested size; min_floats: the least first allocation.  Every user holds an instance of
// its own: two users on one stream may each have scratch in use at the same time.
class StreamScratch {
  public:
    explicit StreamScratch(size_t min_floats = 0) : min_floats_(min_floats) {}
    float* get(hipStream_t s, size_t floats) {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& e : slots_) {
            if (e.stream != s) continue;
            if (e.floats < floats) {
                HIP_CHECK(hipStreamSynchronize(s));
                HIP_CHECK(hipFree(e.buf));
                HIP_CHECK(hipMalloc((void**)&e.buf, floats * sizeof(float)));
                e.floats = floats;
            }
            return e.buf;
        }
        Slot e{s, nullptr, std::max(floats, min_floats_)};
        HIP_CHECK(hipMalloc((void**)&e.buf, e.floats * sizeof(float)));
        slots_.push_back(e);
        return e.buf;
    }

  private:
    struct Slot { hipStream_t stream; float* buf; size_t floats; };
    std::mutex mu_;
    std::vector<Slot> slots_;
    const size_t min_floats_;
};

// ---- graph passes ----------------------------------------------------------------------------------------------------------------
// Graph::forward / Graph::backward hold a GraphPassGuard (kind 0 = forward, 1 = backward).  Unsynchronised, like the caches below:
// the graph passes of a process run on one thread.
inline int g_graph_pass_depth = 0, g_graph_pass_kind = 0;
struct GraphPassGuard {
    int prev_kind;
    explicit GraphPassGuard(int kind) : prev_kind(g_graph_pass_kind) { ++g_graph_pass_depth; g_graph_pass_kind = kind; }
    ~GraphPassGuard() { --g_graph_pass_depth; g_graph_pass_kind = prev_kind; }
    GraphPassGuard(const GraphPassGuard&) = delete;
};
inline bool graph_pass_active() { return g_graph_pass_depth > 0; }

// ---- derived filters of a GRAPH's layers: one batched launch per pass (round 5) -------------------------------------------------
// Inside a graph pass every layer registers its filter (pointer into the graph's parameter arena W or its derived-weights arena Wt,
// stream, geometry Key) with a buffer of its own.  From the second pass on, refresh(range) rebuilds ALL registered operands of that
// range in ONE launch -- at the start of the forward pass for W, right after the dgrad arrangements have been rebuilt for Wt -- and
// the layers find their entry fresh: 20 launches of wino_filter_kernel per cfg2 step become 2.  Freshness never outlives a forward
// pass: Graph::forward invalidates the graph's ranges first (the optimiser, set_weights, a checkpoint load or a broadcast may have
// touched W).  Outside a graph pass (the op-level API) nothing is registered or trusted: the stream's scratch and one launch per call.
// Key: the geometry of the derived operand (operator==).  Job: what the batched kernel needs per entry; Job::first is its first block.
constexpr int FILTER_JOBS_MAX = 24;
constexpr size_t FILTER_ENTRIES_MAX = 512;
template <class Job> struct FilterJobs { Job j[FILTER_JOBS_MAX]; int n, total; };      // total: blocks

template <class Key, class Job>
class DerivedFilterCache {
  public:
    struct Entry {
        const float* w; hipStream_t stream; Key key; size_t floats; float* buf;
        int kind;          // pass it was registered in (0 forward, 1 backward)
        bool fresh;
    };
    explicit DerivedFilterCache(size_t scratch_min_floats) : scratch_(scratch_min_floats) {}

    // -> the buffer to use and whether its contents still have to be built (by the caller, on s)
    float* lookup(hipStream_t s, const float* w, const Key& key, size_t floats, bool& need, bool enabled = true) {
        need = true;
        if (!graph_pass_active() || !enabled) return scratch_.get(s, floats);
        for (auto& e : entries_)
            if (e.w == w && e.stream == s && e.key == key) {
                need = !e.fresh;
                e.fresh = true;                      // (the caller builds it now if it was not)
                return e.buf;
            }
        if (entries_.size() >= FILTER_ENTRIES_MAX) return scratch_.get(s, floats);
        Entry e{w, s, key, floats, nullptr, g_graph_pass_kind, true};
        HIP_CHECK(hipMalloc((void**)&e.buf, floats * sizeof(float)));
        entries_.push_back(e);
        return e.buf;
    }
    void invalidate(const float* lo, const float* hi) {
        for (auto& e : entries_)
            if (e.w >= lo && e.w < hi) e.fresh = false;
    }
    void release(const float* lo, const float* hi) {
        for (size_t i = 0; i < entries_.size();) {
            if (entries_[i].w >= lo && entries_[i].w < hi) { (void)hipFree(entries_[i].buf); entries_[i] = entries_.back(); entries_.pop_back(); }
            else ++i;
        }
    }
    // the stale entries of [lo, hi), `kind` and s, at most FILTER_JOBS_MAX per launch: fill(entry, job) -> the job's blocks,
    // launch(jobs) runs the batched kernel over jobs.total blocks
    template <class Fill, class Launch>
    void refresh(hipStream_t s, const float* lo, const float* hi, int kind, Fill fill, Launch launch) {
        FilterJobs<Job> jobs;
        jobs.n = 0; jobs.total = 0;
        auto flush = [&]() {
            if (!jobs.n) return;
            launch(jobs);
            jobs.n = 0; jobs.total = 0;
        };
        for (auto& e : entries_) {
            if (e.fresh || e.kind != kind || e.stream != s || e.w < lo || e.w >= hi) continue;
            if (jobs.n == FILTER_JOBS_MAX) flush();
            Job& j = jobs.j[jobs.n++];
            const int blocks = fill(e, j);
            j.first = jobs.total;
            jobs.total += blocks;
            e.fresh = true;
        }
        flush();
    }

  private:
    std::vector<Entry> entries_;
    StreamScratch scratch_;
};
