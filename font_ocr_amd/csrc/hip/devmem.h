// devmem.h — the one owner of device memory in libfocr_hip.so.  Nothing else in this directory calls the runtime's
// allocator: every device buffer is a DevArray<T> member (or local), freed when its owner dies, and every allocated
// byte is counted (focr_debug_device_bytes; tests/test_gpu_device_memory.py).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace focr {

inline std::atomic<size_t> g_device_bytes{0};  // live bytes of every DevArray of the process

// How a buffer that is too small grows.  Capacity decides how often a steady stream of batches re-allocates and how much
// memory a context holds, so every reserve call names its rule.
enum class Grow : uint8_t {
    exact,       // `want` elements
    eighth,      // max(want + want / 8, 1024) elements (the match list)
    quarter,     // want + want / 4 + 256 BYTES (scratch re-sized by every scan)
    half,        // want + want / 2 + 256 BYTES (lists that are appended to: reserve's `keep`)
};

template <typename T>
struct DevArray {
    T *p = nullptr;
    size_t cap = 0;  // elements (the byte rules: the allocation's bytes / sizeof(T), rounded down)

    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    DevArray(DevArray &&o) noexcept : p(o.p), cap(o.cap), bytes_(o.bytes_) { o.forget(); }
    DevArray &operator=(DevArray &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap, bytes_ = o.bytes_;
            o.forget();
        }
        return *this;
    }
    ~DevArray() { release(); }  // (the owner of the array has selected the device and waited for its stream)

    operator T *() const { return p; }
    template <typename U>
    U *as() const { return reinterpret_cast<U *>(p); }  // scratch that is re-read as another type

    void release() {
        if (p) (void)hipFree(p);
        g_device_bytes -= bytes_;
        forget();
    }

    // Room for `want` elements.  A buffer that has it stays as it is; otherwise it is replaced by one sized by the rule, after a
    // wait for `*wait` (null: the caller knows the buffer is idle) — the first `keep` elements move to the new buffer, the
    // rest is undefined.  A failed allocation leaves the array empty.
    hipError_t reserve(size_t want, Grow rule, const hipStream_t *wait, size_t keep = 0) {
        if (p && want <= cap) return hipSuccess;
        const size_t wb = want * sizeof(T);
        const size_t bytes = rule == Grow::exact     ? wb
                             : rule == Grow::eighth  ? std::max<size_t>(want + want / 8, 1024) * sizeof(T)
                             : rule == Grow::quarter ? wb + wb / 4 + 256
                                                     : wb + wb / 2 + 256;
        if (!bytes) return hipSuccess;  // (exact, nothing wanted)
        if (wait)
            if (hipError_t e = hipStreamSynchronize(*wait)) return e;  // (the array stays as it was)
        DevArray old(std::move(*this));
        if (!keep) old.release();
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        p = static_cast<T *>(q), cap = bytes / sizeof(T), bytes_ = bytes;
        g_device_bytes += bytes;
        if (keep && old.p && (e = hipMemcpy(p, old.p, keep * sizeof(T), hipMemcpyDeviceToDevice)) != hipSuccess) release();
        return e;
    }

    // A fresh buffer of exactly max(n, at_least) elements holding the n host elements at src.
    hipError_t upload(const T *src, size_t n, size_t at_least = 0) {
        release();
        if (hipError_t e = reserve(std::max(n, at_least), Grow::exact, nullptr)) return e;
        return n ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }

  private:
    size_t bytes_ = 0;
    void forget() { p = nullptr, cap = 0, bytes_ = 0; }
};

}  // namespace focr
