// sluamd_devmem.h -- internal: who owns device memory.  Header-only over sluamd_rt.h, so the CPU test build compiles the same code.
//
//   dev_alloc   the one place outside sluamd_devpool.cpp that calls hipMalloc: on failure the process pool of arena chunks gives back what it
//               holds and the allocation is tried once more; a second failure is SLUAMD_ENOMEM with a message that names the buffer.  HIP's
//               sticky error is cleared both times, so a later HIPCHK(hipGetLastError()) does not blame an unrelated launch.
//   DevBuf<T>   owns one allocation (alloc: exact, reserve: grow-only).   DevBag: owns "everything else", hands out raw pointers.
//   PoolBuf     the value arena: like DevBuf, but its memory may come from the pool (devpool_alloc) and always goes back through devpool_free.
//
// Freeing a buffer that queued work still reads or writes relies on hipFree: it synchronises the device before it releases the memory.  No
// owner here synchronises a stream of its own before a free (the batch object's buffers used to; nothing singles them out).
// No sub-allocation, no caching: an owner and a helper.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include <sluamd_rt.h>
#include "superlu_dist_amd.h"

namespace sluamd {

void set_error(const std::string &msg);

// value arenas on a process-level pool of physical device chunks (sluamd_devpool.cpp; the CPU test build: oracle/emul/emul_rt.cpp)
int devpool_alloc(void **p, size_t bytes, int device);   // 0, or SLUAMD_ENOMEM without a message: the pool could not serve it (PoolBuf then asks dev_alloc)
void devpool_free(void *p);               // pool ranges and plain allocations alike
void devpool_trim(int device);            // device < 0: every device
size_t devpool_cached_bytes(int device);

// how many times dev_alloc was asked in this process (sluamd_device_alloc_count): what a test reads to see that a second call allocates nothing
inline std::atomic<int64_t> &dev_alloc_calls() { static std::atomic<int64_t> n{0}; return n; }

inline int dev_alloc(void **p, size_t bytes, int device, const char *what)
{
    ++dev_alloc_calls();
    bytes = std::max<size_t>(bytes, 1);
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        devpool_trim(device);          // what the pool holds may be what is missing
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) return 0;
    (void) hipGetLastError();
    *p = nullptr;
    set_error(std::string("out of device memory: ") + what + " (" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    return SLUAMD_ENOMEM;
}

template <class T> class DevBuf {
public:
    T *p = nullptr;
    int64_t cap = 0;          // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); std::swap(p, o.p); std::swap(cap, o.cap); } return *this; }
    ~DevBuf() { reset(); }
    T *get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
    void reset() { if (p) hipFree(p); p = nullptr; cap = 0; }
    int alloc(int64_t count, int device, const char *what)      // exactly `count` elements; what the buffer held goes first
    {
        reset();
        if (int rc = dev_alloc((void **) &p, sizeof(T) * (size_t) std::max<int64_t>(count, 0), device, what)) return rc;
        cap = count;
        return 0;
    }
    int reserve(int64_t count, int device, const char *what) { return count <= cap ? 0 : alloc(count, device, what); }   // grow-only
};

class DevBag {
    std::vector<void *> v_;
public:
    int device = 0;           // whose pool is trimmed when an allocation fails
    DevBag() = default;
    DevBag(const DevBag &) = delete;
    DevBag &operator=(const DevBag &) = delete;
    DevBag(DevBag &&o) noexcept : v_(std::move(o.v_)), device(o.device) { o.v_.clear(); }
    DevBag &operator=(DevBag &&o) noexcept { if (this != &o) { clear(); v_.swap(o.v_); device = o.device; } return *this; }
    ~DevBag() { clear(); }
    void clear() { for (void *q : v_) hipFree(q); v_.clear(); }
    template <class T> int alloc(T **d, size_t count, const char *what)
    {
        if (int rc = dev_alloc((void **) d, sizeof(T) * count, device, what)) return rc;
        v_.push_back(*d);
        return 0;
    }
};

class PoolBuf {
public:
    double *p = nullptr;
    PoolBuf() = default;
    PoolBuf(const PoolBuf &) = delete;
    PoolBuf &operator=(const PoolBuf &) = delete;
    ~PoolBuf() { reset(); }
    double *get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
    void reset() { if (p) devpool_free(p); p = nullptr; }
    int alloc(size_t bytes, int device, bool pooled, const char *what)
    {
        reset();
        if (pooled && devpool_alloc((void **) &p, bytes, device) == 0) return 0;
        return dev_alloc((void **) &p, bytes, device, what);
    }
};

}  // namespace sluamd
