// Memory a handle owns, freed with the handle (vq_index.hip, vq_preproc.hip).
#pragma once
#include "vq_common.h"
#include <algorithm>
#include <utility>

namespace vq {

// Device memory.  reserve() keeps no contents (free, then allocate); storage that grows by other rules (the index's rows: with a
// copy; ranks and labels: behind a stream synchronise, under their own message) is allocated by the code that grows it, straight
// into p.  `tag` opens the out-of-memory message: the handle's name.
template <class T> struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;               // elements
    const char* const tag;
    explicit DevBuf(const char* tag_) : tag(tag_) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    int reserve(int64_t need) {
        if (need <= cap) return 0;
        release();
        hipError_t e = hipMalloc((void**)&p, (size_t)need * sizeof(T));
        if (e != hipSuccess) return fail(VQ_ERR_OOM, "%shipMalloc(%lld) failed: %s", tag, (long long)(need * sizeof(T)), hipGetErrorString(e));
        cap = need;
        return 0;
    }
};

// Pinned host memory; a mapped one also has a device address (dev) that kernels write through.  Whoever replaces a buffer the
// device may still be using waits for the stream first.
template <class T> struct PinnedBuf {
    T* p = nullptr;
    T* dev = nullptr;              // mapped only
    int64_t cap = 0;               // elements
    const bool mapped;
    explicit PinnedBuf(bool map = false) : mapped(map) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; cap = 0; }
    int reserve(int64_t need, int64_t at_least = 0) {          // no contents kept; a new buffer holds max(need, at_least)
        if (need <= cap) return 0;
        release();
        const int64_t ncap = std::max(need, at_least);
        VQ_HIP(hipHostMalloc((void**)&p, (size_t)ncap * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault));
        if (mapped) VQ_HIP(hipHostGetDevicePointer((void**)&dev, p, 0));
        cap = ncap;
        return 0;
    }
};

}  // namespace vq
