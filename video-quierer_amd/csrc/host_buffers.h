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

// One output array of a search family.  A family states its outputs once, as a list of these, and both of its forms work from
// that list: the empty answer, the host form's device block and its copies back (vq_index.hip, "a family's outputs").
struct OutField {
    void* dst;                     // the caller's array: device memory in a device form, host memory in a host form; null: not asked for
    int64_t count;                 // elements
    int width;                     // bytes per element: 4 or 8
    uint64_t empty;                // bit pattern of an element that holds no result
    bool owned = false;            // host form: the family names device memory it already has (dev) instead of a piece of the block
    void* dev = nullptr;           // where the run writes the field; null while dst is
    size_t bytes() const { return (size_t)count * width; }
};
constexpr uint64_t OUT_NONE = 0xffffffffu;     // int32 -1: no row, no group
constexpr uint64_t OUT_INF = 0x7f800000u;      // float +inf: no distance
constexpr uint64_t OUT_ZERO = 0;               // a count, a length, a 64-bit mass
constexpr int OUT_MAX_FIELDS = 8;

// How a host form's results reach the caller: each field copied straight into the caller's array; or through the pinned result
// buffer and a memcpy, field by field or as one copy of the whole block (the two filtered searches).
enum CopyBack { COPY_TO_CALLER, COPY_PINNED_FIELDS, COPY_PINNED_BLOCK };

struct Outs {
    int n;
    OutField f[OUT_MAX_FIELDS];
    CopyBack how = COPY_TO_CALLER;
    template <class T> T* dev(int i) const { return (T*)f[i].dev; }
    bool given(int first) const {                  // the first `first` fields, the required ones, are all there
        for (int i = 0; i < first; ++i) if (!f[i].dst) return false;
        return true;
    }
};

// memory <- count elements of the field's empty value
inline void out_fill_host(void* p, const OutField& f) {
    if (f.width == 8) std::fill((uint64_t*)p, (uint64_t*)p + f.count, f.empty);
    else std::fill((uint32_t*)p, (uint32_t*)p + f.count, (uint32_t)f.empty);
}

// The host form's device block: the fields that are asked for and not owned, one behind the other at 8-byte aligned offsets (so
// a 64-bit field may stand anywhere in the list).  off[i]: field i's offset, -1 for a field without a piece; returns the bytes.
inline int64_t outs_layout(const Outs& o, int64_t off[OUT_MAX_FIELDS]) {
    int64_t at = 0;
    for (int i = 0; i < o.n; ++i) {
        const bool piece = o.f[i].dst && !o.f[i].owned;
        off[i] = piece ? at : -1;
        if (piece) at += round_up((int64_t)o.f[i].bytes(), 8);
    }
    return at;
}

}  // namespace vq
