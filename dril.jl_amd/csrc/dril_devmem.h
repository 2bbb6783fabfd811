// dril_devmem.h — the two owners of every allocation a handle holds: DevBuf<T> (device memory) and PinnedBuf<T> (page-locked host memory).
// Move-only; the destructor frees.  Each converts implicitly to T*, so a use site reads as it did with a raw pointer; a raw pointer MEMBER of a handle
// therefore means "not owned": an alias into one of these, or the caller's memory.
// The owners reach the runtime through two pairs of free functions, which also keep the process-wide count of bytes held (dril_debug_device_bytes_live).
// Under hipcc they are defined here; a host compile leaves them to the including file (tests/test_devmem.py drives the owners over malloc / free with g++).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace dril {

#if defined(__HIPCC__)
using devmem_err_t = hipError_t;
#else
using devmem_err_t = int;                             // 0: success
#endif

inline std::atomic<int64_t> g_devmem_live_bytes{0};   // device + pinned bytes the owners hold, process-wide

// *p = `bytes` of device memory (zero: cleared before the call returns) / of pinned host memory; on failure *p stays null and the count unchanged
#if !defined(__HIPCC__)
devmem_err_t devmem_alloc_device(void** p, size_t bytes, bool zero);
void devmem_free_device(void* p, size_t bytes);
devmem_err_t devmem_alloc_pinned(void** p, size_t bytes);
void devmem_free_pinned(void* p, size_t bytes);
#else
inline devmem_err_t devmem_alloc_device(void** p, size_t bytes, bool zero) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess && zero) { e = hipMemset(q, 0, bytes); if (e != hipSuccess) (void)hipFree(q); }
    if (e != hipSuccess) return e;
    *p = q; g_devmem_live_bytes += (int64_t)bytes;
    return hipSuccess;
}
inline void devmem_free_device(void* p, size_t bytes) { (void)hipFree(p); g_devmem_live_bytes -= (int64_t)bytes; }
inline devmem_err_t devmem_alloc_pinned(void** p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    *p = q; g_devmem_live_bytes += (int64_t)bytes;
    return hipSuccess;
}
inline void devmem_free_pinned(void* p, size_t bytes) { (void)hipHostFree(p); g_devmem_live_bytes -= (int64_t)bytes; }
#endif

template <typename T, bool kPinned> class MemBuf {
public:
    MemBuf() = default;
    MemBuf(const MemBuf&) = delete;
    MemBuf& operator=(const MemBuf&) = delete;
    MemBuf(MemBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    MemBuf& operator=(MemBuf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~MemBuf() { release(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }                // elements; 0 when empty (alloc(0) holds one element and reports 1)

    // n elements (0: one, so that the pointer is never null after success); frees what it held first.  On failure the owner is empty
    devmem_err_t alloc(size_t n) { return take(n, false); }
    devmem_err_t alloc_zero(size_t n) { return take(n, true); }
    // grow-only: a buffer of at least n elements is kept; otherwise alloc(n), and *reallocated (where asked for) is set
    devmem_err_t grow(size_t n, bool* reallocated = nullptr) { return regrow(n, false, reallocated); }
    devmem_err_t grow_zero(size_t n, bool* reallocated = nullptr) { return regrow(n, true, reallocated); }
    void release() {
        if (!p_) return;
        if (kPinned) devmem_free_pinned(p_, n_ * sizeof(T)); else devmem_free_device(p_, n_ * sizeof(T));
        p_ = nullptr; n_ = 0;
    }

private:
    devmem_err_t regrow(size_t n, bool zero, bool* reallocated) {
        const bool keep = p_ && n <= n_;
        if (reallocated) *reallocated = !keep;
        return keep ? devmem_err_t{} : take(n, zero);
    }
    devmem_err_t take(size_t n, bool zero) {
        release();
        if (!n) n = 1;
        void* q = nullptr;
        const devmem_err_t e = kPinned ? devmem_alloc_pinned(&q, n * sizeof(T)) : devmem_alloc_device(&q, n * sizeof(T), zero);
        if (e != devmem_err_t{}) return e;
        p_ = (T*)q; n_ = n;
        return e;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <typename T> using DevBuf = MemBuf<T, false>;
template <typename T> using PinnedBuf = MemBuf<T, true>;

}  // namespace dril
