// itd_memory.hpp — who owns the library's device and pinned host memory: Buf<T> (hipMalloc) and Pinned<T> (hipHostMalloc) know
// their pointer and their size and free themselves; non-copyable, movable (a moved-from buffer is empty).  No allocator, no pool:
// every call is one hipMalloc / hipFree (hipHostMalloc / hipHostFree) at the moment it is made.  Included behind the HIP runtime's
// header; tests/c_client/memory_host.cpp includes it behind malloc-backed stand-ins for the six runtime calls it uses.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <utility>

#include "../../include/pyitd_hip.h"

namespace itd {

// PYITD_POISON=1 (a debugging switch of the environment, read once): every block of device memory the library allocates is filled
// with 0xFF bytes (NaNs / -1) before its first use, so that a kernel that reads memory nobody wrote fails on every run instead of
// once in ten thousand — what tools/stream_fuzz.py and the suite are run under in the evidence session.
inline bool poison_on() { static const bool on = [] { const char *v = getenv("PYITD_POISON"); return v && *v && *v != '0'; }(); return on; }

enum class Mem { Device, Pinned };

template <class T, Mem K = Mem::Device>
class Buf {
    void *p_ = nullptr;
    size_t bytes_ = 0;

public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { release(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~Buf() { release(); }

    // A block of exactly `bytes`; what the buffer held is freed first, on failure it is empty.  counted: the workspace counter the
    // size is added to (it stays counted when the block is freed or handed on); flags: hipHostMalloc's.  A device block is poisoned
    // here and only here, ahead of any fill of the caller's (both on the null stream, which the engines' streams are not ordered with)
    hipError_t alloc(size_t bytes, int64_t *counted = nullptr, unsigned flags = 0)
    {
        release();
        const hipError_t rc = K == Mem::Pinned ? hipHostMalloc(&p_, bytes, flags) : hipMalloc(&p_, bytes);
        if (rc != hipSuccess) { p_ = nullptr; return rc; }
        bytes_ = bytes;
        if (counted) *counted += (int64_t)bytes;
        if (K == Mem::Device && bytes && poison_on()) { (void)hipMemset(p_, 0xFF, bytes); (void)hipDeviceSynchronize(); }
        return hipSuccess;
    }
    // grow only: nothing when the block holds `want` bytes, else alloc(want); ITD_ERR_NOMEM when that fails (*why: the runtime's error)
    int reserve(size_t want, hipError_t *why = nullptr)
    {
        if (bytes_ >= want) return ITD_OK;
        const hipError_t rc = alloc(want);
        if (why) *why = rc;
        return rc == hipSuccess ? ITD_OK : ITD_ERR_NOMEM;
    }
    void release()
    {
        if (p_) (void)(K == Mem::Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }
    T *get() const { return static_cast<T *>(p_); }
    operator T *() const { return get(); }                                         // read like the pointer the field was
    template <class U> explicit operator U *() const { return static_cast<U *>(p_); }   // ... and cast like it (the untyped arenas)
};
template <class T> using Pinned = Buf<T, Mem::Pinned>;

}  // namespace itd
