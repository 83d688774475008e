// host_copy.hpp -- the bounce copy of a host frame into pinned memory, in bands on a few threads.  Host code only (no HIP
// include): tiled_push_host and the mosaic stage call copy_rows, tools/host_copy_check.cpp checks it under the sanitizers.
#pragma once

#include <stddef.h>
#include <string.h>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace mi {

// Persistent helper threads for the bounce copy of big frames: workers sleep on a condition variable and take the bands of
// ONE copy at a time.
class CopyPool {
public:
    static CopyPool& get() {
        static CopyPool p;
        return p;
    }
    // runs fn(k) for k = 0 .. parts-1: k = 0 on the caller, the others on the workers; returns when all are done
    void run(int parts, const std::function<void(int)>& fn) {
        std::lock_guard<std::mutex> serial(call_mu_);   // one copy at a time (several stacks may push from several threads)
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn;
            next_ = 1;
            parts_ = parts;
            pending_ = parts - 1;
        }
        cv_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    CopyPool() {
        for (int i = 0; i < NW; ++i) th_[i] = std::thread([this] { loop(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || (fn_ && next_ < parts_); });
            if (stop_) return;
            const int k = next_++;
            const auto* fn = fn_;
            lk.unlock();
            (*fn)(k);
            lk.lock();
            if (--pending_ == 0) done_.notify_all();
        }
    }
    static constexpr int NW = 3;
    std::thread th_[NW];
    std::mutex mu_, call_mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    int next_ = 0, parts_ = 0, pending_ = 0;
    bool stop_ = false;
};

// One thread copies ~25 GB/s into pinned memory -- half of what the PCIe link then moves; copies from 32 MiB on are made by
// four threads (the caller + the pool's three).
inline int copy_threads(size_t bytes) { return bytes >= ((size_t)32 << 20) ? 4 : 1; }

// `rows` rows of `row_bytes` each, `src_stride` bytes apart in `src`, into the contiguous `dst`, in `nthr` bands (1, or at most
// the pool's threads + 1): bands of rows, or of bytes when there is one row -- a packed span.
inline void copy_rows(void* dst, const void* src, size_t src_stride, size_t row_bytes, size_t rows, int nthr) {
    char* d = (char*)dst;
    const char* s = (const char*)src;
    const std::function<void(int)> band = [&](int k) {
        if (rows == 1) {
            const size_t a = row_bytes * (size_t)k / nthr, b = row_bytes * (size_t)(k + 1) / nthr;
            memcpy(d + a, s + a, b - a);
            return;
        }
        const size_t y0 = rows * (size_t)k / nthr, y1 = rows * (size_t)(k + 1) / nthr;
        if (src_stride == row_bytes) memcpy(d + y0 * row_bytes, s + y0 * row_bytes, row_bytes * (y1 - y0));
        else
            for (size_t y = y0; y < y1; ++y) memcpy(d + y * row_bytes, s + y * src_stride, row_bytes);
    };
    if (nthr == 1) band(0);
    else CopyPool::get().run(nthr, band);
}

}  // namespace mi
