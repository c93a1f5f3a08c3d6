// yabpe_devmem.h -- device memory of the host drivers: the per-process block cache every allocation goes through, and
// Scratch, the owner of one call's temporaries (DESIGN.md "Host drivers").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace yb {

inline bool trace_alloc_on() {
    static const bool on = [] { const char *e = getenv("YABPE_TRACE_ALLOC"); return e && *e == '1'; }();
    return on;
}

// Device allocations go through a small per-process cache: a training job allocates a few large buffers (tiles,
// signatures, worklists, retile targets) and frees them at the end, and the next job asks for the same sizes again.
// hipMalloc / hipFree of multi-GB buffers are host-side stalls of anywhere from 1 ms to 100+ ms depending on the state of
// the driver's page tables (measured: 14 ms vs 340 ms for the same yabpe_load_words on two boxes) -- time the GPU idles.
// Freed blocks are kept (up to YABPE_POOL_MAX_GIB, default 24) and handed out again to requests of the same rounded size.
// The cache is shared by every context of the process and each context has a stream of its own, so a block may come back
// only after the stream that used it has been synchronised.
struct DevPool {
    std::mutex m;
    std::multimap<std::pair<int, size_t>, void *> free_blocks;  // (device, bytes) -> block
    std::map<void *, std::pair<int, size_t>> live;              // block -> (device, bytes)
    size_t held = 0;
    size_t cap = [] { const char *e = getenv("YABPE_POOL_MAX_GIB"); return (size_t)(e ? atoll(e) : 24) << 30; }();
};
inline DevPool &pool() {
    static DevPool *p = new DevPool();  // (never destroyed: device memory is released by the runtime at process exit)
    return *p;
}
inline size_t pool_round(size_t bytes) { return bytes >= (1u << 20) ? (bytes + ((2u << 20) - 1)) & ~(size_t)((2u << 20) - 1) : (bytes + 255) & ~(size_t)255; }
inline void pool_trim(int dev, size_t need_free) {  // give cached blocks back to the runtime (largest first)
    DevPool &P = pool();
    size_t freed = 0;
    while (freed < need_free && !P.free_blocks.empty()) {
        auto it = std::prev(P.free_blocks.end());
        (void)dev;
        freed += it->first.second;
        P.held -= it->first.second;
        (void)hipFree(it->second);
        P.free_blocks.erase(it);
    }
}
inline hipError_t pool_alloc(int dev, void **out, size_t bytes) {
    DevPool &P = pool();
    const size_t rb = pool_round(bytes);
    std::lock_guard<std::mutex> g(P.m);
    auto it = P.free_blocks.find({dev, rb});
    if (it != P.free_blocks.end()) {
        *out = it->second;
        P.held -= rb;
        P.free_blocks.erase(it);
        P.live[*out] = {dev, rb};
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, rb);
    if (e != hipSuccess) {  // out of memory with blocks in the cache: release them and try once more
        (void)hipGetLastError();
        pool_trim(dev, ~(size_t)0);
        e = hipMalloc(out, rb);
    }
    if (e == hipSuccess) P.live[*out] = {dev, rb};
    return e;
}
inline void pool_free(void *p) {
    DevPool &P = pool();
    std::lock_guard<std::mutex> g(P.m);
    auto it = P.live.find(p);
    if (it == P.live.end()) {  // not ours (allocated with hipMalloc directly)
        (void)hipFree(p);
        return;
    }
    const auto key = it->second;
    P.live.erase(it);
    if (key.second > P.cap) {
        (void)hipFree(p);
        return;
    }
    if (P.held + key.second > P.cap) pool_trim(key.first, P.held + key.second - P.cap);
    P.free_blocks.insert({key, p});
    P.held += key.second;
}

// YABPE_TRACE_ALLOC=1: every device allocation of the library goes to stderr (address range, size) -- the map that tells
// which buffer a "Memory access fault ... on address X" belongs to or lies next to.  rank: -1 outside a context.
inline hipError_t dev_alloc(int device, int rank, void **p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) bytes = 1;
    const hipError_t e = pool_alloc(device, p, bytes);
    if (e == hipSuccess && trace_alloc_on())
        fprintf(stderr, "[yabpe alloc r%d] %p .. %p  %zu B\n", rank, *p, (void *)((char *)*p + bytes), bytes);
    return e;
}
inline void dev_free(void *p) {
    if (!p) return;
    if (trace_alloc_on()) fprintf(stderr, "[yabpe free] %p\n", p);
    pool_free(p);
}

// The device buffers of one call: whatever is still here when the call returns, by any way out, goes back to the cache.
// A buffer that outlives the call is take()n; one that is dead long before the end is release()d (peak memory).
struct Scratch {
    int device = 0, rank = -1;
    std::vector<void *> bufs;
    Scratch() { if (hipGetDevice(&device) != hipSuccess) device = 0; }  // (a driver without a context: the current device)
    Scratch(int device_, int rank_) : device(device_), rank(rank_) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { release(); }
    template <class T>
    hipError_t get(T **p, uint64_t n) {
        const hipError_t e = dev_alloc(device, rank, (void **)p, n * sizeof(T));
        if (e == hipSuccess) bufs.push_back(*p);
        return e;
    }
    void adopt(void *p) {  // a buffer someone else allocated
        if (p) bufs.push_back(p);
    }
    template <class T>
    T *take(T *p) {  // the caller's from here on; nullptr if p is not one of ours
        auto it = std::find(bufs.begin(), bufs.end(), (const void *)p);
        if (it == bufs.end()) return nullptr;
        bufs.erase(it);
        return p;
    }
    void release(const void *p) {  // (not one of ours: nothing happens)
        dev_free(take(const_cast<void *>(p)));
    }
    void release() {
        for (void *p : bufs) dev_free(p);
        bufs.clear();
    }
};

}  // namespace yb
