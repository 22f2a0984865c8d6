// The plumbing of bin/ctucopy's host loop (main.cc): hand-over channels, thread fan-out, the pool of page-locked buffers.  Nothing here knows
// the engine or the options: the pool takes its allocator from its owner, so all of it runs without a GPU (tests/host/host_check.cc).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <deque>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

// bounded hand-over between two stages; close() wakes everybody up (end of the list, or a stage gave up)
template <class T>
struct Chan {
    std::mutex m;
    std::condition_variable cv;
    std::deque<T> q;
    size_t cap;
    bool closed = false;
    explicit Chan(size_t c) : cap(c) {}
    bool push(T v) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return q.size() < cap || closed; });
        if (closed) return false;
        q.push_back(std::move(v));
        cv.notify_all();
        return true;
    }
    bool pop(T &v) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        v = std::move(q.front());
        q.pop_front();
        cv.notify_all();
        return true;
    }
    void close() {
        std::lock_guard<std::mutex> l(m);
        closed = true;
        cv.notify_all();
    }
};
// fn(i) for i in [0, n) on up to `threads` threads; the exception of the lowest failing index is rethrown (what a sequential loop would have hit first)
template <class F>
void parallel_for(int threads, size_t n, F fn) {
    if (n == 0) return;
    const int nt = (int)std::min<size_t>((size_t)std::max(threads, 1), n);
    std::atomic<size_t> next{0};
    std::mutex em;
    size_t err_at = n;
    std::exception_ptr err;
    auto body = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) return;
            try {
                fn(i);
            } catch (...) {
                std::lock_guard<std::mutex> l(em);
                if (i < err_at) {
                    err_at = i;
                    err = std::current_exception();
                }
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(body);
    body();
    for (auto &t : th) t.join();
    if (err) std::rethrow_exception(err);
}
// fn(g) for every GPU ordinal at once, a thread each (an engine call blocks its thread); all are joined, then the lowest failing ordinal's exception is rethrown
template <class F>
void per_gpu(int ngpu, F fn) {
    std::vector<std::exception_ptr> errs(ngpu);
    std::vector<std::thread> th;
    for (int g = 0; g < ngpu; g++)
        th.emplace_back([&, g] {
            try {
                fn(g);
            } catch (...) {
                errs[g] = std::current_exception();
            }
        });
    for (auto &t : th) t.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
}
// page-locked buffers are expensive to make (the runtime pins every page): they go round between the batches.  A PinBuf owns its
// buffer (move-only) and hands it back to the pool when it dies, wherever that is: the pool has to outlive every PinBuf it gave out.
struct PinPool;
struct PinReturn {
    PinPool *pool = nullptr;
    size_t cap = 0;
    inline void operator()(void *p) const;
};
typedef std::unique_ptr<void, PinReturn> PinBuf;
struct PinPool {
    void *(*alloc)(size_t);
    void (*dealloc)(void *);
    std::mutex m;
    std::multimap<size_t, void *> idle;  // by capacity
    PinPool(void *(*a)(size_t), void (*f)(void *)) : alloc(a), dealloc(f) {}
    PinBuf get(size_t bytes) {
        bytes = std::max<size_t>(bytes, 4096);
        {
            std::lock_guard<std::mutex> l(m);
            const auto fit = idle.lower_bound(bytes);  // the smallest idle one that holds it
            if (fit != idle.end()) {
                PinBuf b(fit->second, PinReturn{this, fit->first});
                idle.erase(fit);
                return b;
            }
            if (!idle.empty()) {  // nothing fits: trade the smallest idle one in
                dealloc(idle.begin()->second);
                idle.erase(idle.begin());
            }
        }
        const size_t cap = bytes + bytes / 8;
        void *p = alloc(cap);
        if (!p) throw std::runtime_error("ENGINE: cannot allocate page-locked host memory");
        return PinBuf(p, PinReturn{this, cap});
    }
    void put(void *p, size_t cap) {
        std::lock_guard<std::mutex> l(m);
        idle.emplace(cap, p);
    }
    ~PinPool() {
        for (auto &b : idle) dealloc(b.second);
    }
};
void PinReturn::operator()(void *p) const { pool->put(p, cap); }

// the two threads beside the engine loop.  Its destructor is the pipeline's shutdown order: the reader sees its channel closed and ends, then
// the writer drains what it was handed and ends - at the end of the scope or when it unwinds, so that neither thread is left running.
template <class C>
struct StageThreads {
    C &to_engine, &to_writer;
    std::thread reader, writer;
    ~StageThreads() {
        to_engine.close();
        if (reader.joinable()) reader.join();
        to_writer.close();
        if (writer.joinable()) writer.join();
    }
};
