// host_mem.hpp -- owners of the HIP resources of a handle: device buffers, pinned host blocks, events, the stream.  Each
// frees what it holds in its destructor, so a new member of reg_handle needs its declaration and nothing else.
// Part of the single translation unit reg_core.hip (included there, ahead of host_handle.hpp; not a standalone header).
#pragma once

// Live resources of the process (reg_debug_live_resources): counted where a HIP create call succeeds and where the destroy
// call is made or the resource is abandoned -- never by a registration on a warm handle.  Events and owned streams share one.
static std::atomic<int64_t> g_live_bufs{0}, g_live_bytes{0}, g_live_pinned{0}, g_live_events{0};

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

struct DevBuf : NoCopy {
    void* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) cap = bytes, g_live_bufs += 1, g_live_bytes += (int64_t)cap;
        return e;
    }
    void release() { if (p) (void)hipFree(p); abandon(); }
    void abandon() {   // forgets the block without freeing it: only where the free would wait for a stuck device (reg_dist_shutdown)
        if (p) g_live_bufs -= 1, g_live_bytes -= (int64_t)cap;
        p = nullptr, cap = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

// The six arrays of "sort the keys, find the runs" (sort_runs, host_prims.hpp): keys and values as written and as sorted,
// the 0 / 1 heads of the runs of equal sorted keys, and the exclusive scan of the heads (the run id at every position).
struct RunArrays {
    uint64_t *keys, *sorted;
    uint32_t *vals, *svals, *heads, *run;
};
struct RunBufs {   // their owner; what sort_runs left in them stays until the next use of the same set
    DevBuf keys, keys2, vals, vals2, heads, run;
    hipError_t reserve(size_t n) {
        hipError_t e = keys.reserve(n * 8);
        if (e == hipSuccess) e = keys2.reserve(n * 8);
        for (DevBuf* b : {&vals, &vals2, &heads, &run})
            if (e == hipSuccess) e = b->reserve(n * 4);
        return e;
    }
    RunArrays arrays() const {
        return RunArrays{keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                         vals2.as<uint32_t>(), heads.as<uint32_t>(), run.as<uint32_t>()};
    }
};

// Pinned host block; a mapped one (hipHostMallocMapped) also holds its device view.  alloc / Event::create: once per owner
template <class T>
struct Pinned : NoCopy {
    T *p = nullptr, *dev = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); abandon(); }
    hipError_t alloc(size_t bytes, unsigned flags) {
        hipError_t e = hipHostMalloc((void**)&p, bytes, flags);
        if (e != hipSuccess) return e;
        g_live_pinned += 1;
        return (flags & hipHostMallocMapped) ? hipHostGetDevicePointer((void**)&dev, p, 0) : hipSuccess;
    }
    void abandon() {   // as DevBuf::abandon
        if (p) g_live_pinned -= 1;
        p = dev = nullptr;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

struct Event : NoCopy {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }   // (for std::vector<Event>)
    ~Event() { if (e) (void)hipEventDestroy(e), g_live_events -= 1; }
    hipError_t create(unsigned flags = hipEventDefault) {
        hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r == hipSuccess) g_live_events += 1;
        return r;
    }
    operator hipEvent_t() const { return e; }
};

// The handle's stream: one it created and destroys, or the caller's (reg_set_stream), which it only borrows
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    bool owned = false;
    ~Stream() { borrow(nullptr); }
    hipError_t create() {
        hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (r == hipSuccess) owned = true, g_live_events += 1;
        return r;
    }
    void borrow(hipStream_t other) {   // an owned stream is destroyed first
        if (owned && s) (void)hipStreamDestroy(s), g_live_events -= 1;
        s = other, owned = false;
    }
    operator hipStream_t() const { return s; }
};
