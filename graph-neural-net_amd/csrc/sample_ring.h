// sample_ring.h -- internal: what the worker threads that draw a sampled training loop's batches (sampler.hip) share with the
// thread that uploads them and enqueues the steps.  The run is cut into chunks; chunk c of every member lives in host slot
// c % slots of that member's pinned ring.  A producer draws ONE member's part of a chunk at a time; the consumer takes chunk c
// when every member's part of it is drawn, and hands a slot back when the upload that read it has completed.  Only counters,
// a stop flag and the first error live here -- no index, no HIP: the hand-over can be checked on the host
// (tests/native/sample_ring_check.cpp).
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace gnn {
namespace host {

// The chunk schedule of a run of `iterations`: 16, 32, 64, ... doubling up to `cap` iterations per chunk, then `cap` each
// (nothing runs on the GPU until the first chunk is sampled, so the first ones are short).  cap: a power of two.
struct ChunkSchedule {
    int iterations = 0, cap = 256;
    int begin(int c) const { // cap 256: 0, 16, 48, 112, 240, 496, 752, ..
        int b = 0, sz = std::min(16, cap);
        for (int i = 0; i < c; i++) { b += sz; sz = std::min(cap, sz * 2); if (sz == cap && i + 1 < c) { b += (c - i - 1) * cap; break; } }
        return b;
    }
    int end(int c) const { return std::min(iterations, begin(c + 1)); }
    int length(int c) const { return end(c) - begin(c); }
    int chunks() const { int n = 0; while (begin(n) < iterations) n++; return n; }
};

class SampleRing {
public:
    SampleRing(int members, int slots, int chunks) : slots_(slots), chunks_(chunks), drawn_((size_t)members, 0) {}
    int members() const { return (int)drawn_.size(); }
    int chunks() const { return chunks_; }

    // -- a producer, for member m and chunks c = 0, 1, .. in order ---------------------------------------------------
    // waits until chunk c's host slot is free (chunk c - slots has been released); false: stop drawing (stop or an error)
    bool acquire(int c) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || rc_ != 0 || c < released_ + slots_; });
        return !stop_ && rc_ == 0;
    }
    void drawn(int m, int c) { // member m's part of chunk c is in its slot
        { std::lock_guard<std::mutex> lk(mu_); drawn_[(size_t)m] = c + 1; }
        cv_.notify_all();
    }
    void failed(int rc, const std::string &msg) { // the FIRST error is kept; every waiter wakes
        { std::lock_guard<std::mutex> lk(mu_); if (rc_ == 0) { rc_ = rc; msg_ = msg; } }
        cv_.notify_all();
    }

    // -- the consumer ------------------------------------------------------------------------------------------------
    // every member's part of chunk c is drawn (or an error is set: look at error())
    bool ready(int c) {
        std::lock_guard<std::mutex> lk(mu_);
        return ready_locked(c);
    }
    // the same, waiting up to `us` microseconds for it
    bool wait_ready(int c, int us) {
        std::unique_lock<std::mutex> lk(mu_);
        // (a deadline on the system clock: the wait is then pthread_cond_timedwait, which thread checkers know)
        return cv_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds(us), [&] { return ready_locked(c); });
    }
    int error(std::string *msg = nullptr) {
        std::lock_guard<std::mutex> lk(mu_);
        if (msg) *msg = msg_;
        return rc_;
    }
    // the host slots of chunks [0, upto) are the producers' again
    void release(int upto) {
        { std::lock_guard<std::mutex> lk(mu_); released_ = std::max(released_, upto); }
        cv_.notify_all();
    }
    void stop() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
    }

private:
    bool ready_locked(int c) const {
        if (rc_ != 0) return true;
        for (int d : drawn_) if (d <= c) return false;
        return true;
    }
    std::mutex mu_;
    std::condition_variable cv_;
    const int slots_, chunks_;
    std::vector<int> drawn_; // per member: chunks drawn
    int released_ = 0;       // chunks whose host slot is free again
    int rc_ = 0;
    bool stop_ = false;
    std::string msg_;
};

// The worker threads: thread t of n draws members t, t + n, t + 2n, .. of every chunk through draw(member, chunk), which
// returns 0 or an error code (msg: its text).  Joined on EVERY exit path, an exception included (a joinable std::thread's
// destructor terminates): the destructor stops the ring first, so a producer ends after the part it is drawing.
class SampleWorkers {
public:
    static int threads_for(int members) { return std::min(members, 8); } // (never sized from the machine's CPU count)
    template <class Draw> SampleWorkers(SampleRing &ring, int n_threads, Draw draw) : ring_(ring) {
        t_.reserve((size_t)n_threads);
        for (int t = 0; t < n_threads; t++) try {
            t_.emplace_back([&ring, t, n_threads, draw]() {
                for (int c = 0; c < ring.chunks(); c++) {
                    if (!ring.acquire(c)) return;
                    for (int m = t; m < ring.members(); m += n_threads) {
                        std::string msg;
                        const int rc = draw(m, c, &msg);
                        if (rc != 0) { ring.failed(rc, msg); return; }
                        ring.drawn(m, c);
                    }
                }
            });
        } catch (...) { join(); throw; } // (a thread could not be started: no destructor runs for this object)
    }
    ~SampleWorkers() { join(); }
    SampleWorkers(const SampleWorkers &) = delete;
    SampleWorkers &operator=(const SampleWorkers &) = delete;

private:
    void join() {
        ring_.stop();
        for (std::thread &t : t_) if (t.joinable()) t.join();
    }
    SampleRing &ring_;
    std::vector<std::thread> t_;
};

} // namespace host
} // namespace gnn
