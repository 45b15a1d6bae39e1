// f110_devmem.hpp — who owns the handle's device memory.  Two move-only owners over one allocation seam:
//   DevBuf<T>  one allocation that is replaced or grown on its own (a map table, a render buffer, a noise block).  Converts to
//              T *, so launch sites and pointer arithmetic read as with a raw pointer; frees in reset(), alloc(), a grow() past
//              its capacity, move-assignment and its destructor — all of them a plain free at that point, nothing deferred.
//   DevArena   allocations that live and die together and whose pointers sit, raw, in a struct the kernels take by value
//              (AgentArrays, EpisodeArrays, SamplerJob, ...): alloc() hands the pointer out and remembers it, clear() frees all.
// The seam counts live allocations and bytes process-wide (f110_device_allocs).  With -DF110_DEVMEM_HOST it is malloc / free
// plus "fail the n-th allocation from now", so that the owners can be exercised on a CPU under the sanitizers.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#ifdef F110_DEVMEM_HOST
#include <cstdlib>
#else
#include <hip/hip_runtime.h>
#endif

namespace devmem {

inline std::atomic<int64_t> g_live{0}, g_bytes{0};

// an allocation is never smaller than this, so a zero count still yields a pointer of its own
inline size_t padded(size_t bytes) { return bytes > 0 ? bytes : 8; }

#ifdef F110_DEVMEM_HOST
using err_t = int;
constexpr err_t kOk = 0, kNoMem = 2;
inline std::atomic<long> g_fail_in{0};   // > 0: that many allocations from now, one fails
inline void fail_nth(long n) { g_fail_in = n; }
inline err_t raw_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (g_fail_in > 0 && --g_fail_in == 0) return kNoMem;
    *p = std::malloc(padded(bytes));
    return *p ? kOk : kNoMem;
}
inline void raw_release(void *p) { std::free(p); }
#else
using err_t = hipError_t;
constexpr err_t kOk = hipSuccess;
inline err_t raw_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    return hipMalloc(p, padded(bytes));
}
inline void raw_release(void *p) { (void)hipFree(p); }
#endif

// the seam: every allocation and free of the owners below goes through this pair
inline err_t seam_alloc(void **p, size_t bytes)
{
    const err_t e = raw_alloc(p, bytes);
    if (e != kOk) return e;
    g_live += 1;
    g_bytes += (int64_t)padded(bytes);
    return kOk;
}

inline void seam_free(void *p, size_t bytes)
{
    if (!p) return;
    raw_release(p);
    g_live -= 1;
    g_bytes -= (int64_t)padded(bytes);
}

template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;   // elements

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_)
    {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_;
            cap_ = o.cap_;
            o.p_ = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }

    void reset()
    {
        seam_free(p_, cap_ * sizeof(T));
        p_ = nullptr;
        cap_ = 0;
    }
    // a fresh allocation of `count` elements; what was held is freed first (also when the allocation then fails)
    err_t alloc(size_t count)
    {
        reset();
        void *q = nullptr;
        const err_t e = seam_alloc(&q, count * sizeof(T));
        if (e != kOk) return e;
        p_ = static_cast<T *>(q);
        cap_ = count;
        return kOk;
    }
    // grow-only: nothing happens while the capacity suffices; the contents do not survive a regrow
    err_t grow(size_t count) { return p_ && count <= cap_ ? kOk : alloc(count); }
};

class DevArena {
    struct Rec {
        void *p;
        size_t bytes;
    };
    std::vector<Rec> recs_;

public:
    DevArena() = default;
    DevArena(const DevArena &) = delete;
    DevArena &operator=(const DevArena &) = delete;
    DevArena(DevArena &&o) noexcept : recs_(std::move(o.recs_)) { o.recs_.clear(); }
    DevArena &operator=(DevArena &&o) noexcept
    {
        if (this != &o) {
            clear();
            recs_ = std::move(o.recs_);
            o.recs_.clear();
        }
        return *this;
    }
    ~DevArena() { clear(); }

    size_t size() const { return recs_.size(); }

    template <typename T>
    err_t alloc(T **ptr, size_t count)
    {
        recs_.reserve(recs_.size() + 1);   // (before the allocation: nothing between it and its record can throw)
        void *q = nullptr;
        const err_t e = seam_alloc(&q, count * sizeof(T));
        if (e != kOk) return e;
        recs_.push_back(Rec{q, count * sizeof(T)});
        *ptr = static_cast<T *>(q);
        return kOk;
    }
    void clear()
    {
        for (const Rec &r : recs_) seam_free(r.p, r.bytes);
        recs_.clear();
    }
};

}   // namespace devmem
