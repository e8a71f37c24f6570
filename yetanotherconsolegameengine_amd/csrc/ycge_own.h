// ycge_own.h - the owners of what the host side holds on the GPU: device buffers, events, streams, page-locked staging, one word of signal
// memory.  Each is a handle, a destructor and moves - no sharing, no allocator, no base class.  They are the ONLY code of the host
// translation units that creates or frees such a resource (tests/test_host_cpu.py reads the sources for it), so a member of one of these
// types cannot leak, whatever way its holder goes.  What the library holds through them is counted (ycge_debug_live_resources).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ycge_host {

// process-wide: {device allocations, device bytes, events, streams, page-locked allocations, page-locked bytes} held right now
enum { LIVE_DEV = 0, LIVE_DEV_BYTES, LIVE_EVENTS, LIVE_STREAMS, LIVE_PINNED, LIVE_PINNED_BYTES, LIVE_KINDS };
inline std::atomic<int64_t> g_live[LIVE_KINDS];          // (one per library: C++17 inline variable)
inline void live_add(int kind, int64_t n, int64_t bytes) { g_live[kind].fetch_add(n, std::memory_order_relaxed); g_live[kind + 1].fetch_add(bytes, std::memory_order_relaxed); }

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0, cap = 0;          // elements in use / elements allocated
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; cap = o.cap; o.p = nullptr; o.n = o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    static size_t bytes_of(size_t count) { return count * sizeof(T) + 64; }     // records are read with whole 64- / 72-byte fetches: room for the over-read past the last record
    void release() { if (p) { (void)hipFree(p); live_add(LIVE_DEV, -1, -(int64_t)bytes_of(cap)); p = nullptr; } n = cap = 0; }
    hipError_t alloc(size_t count)
    {
        release();
        if (count == 0) return hipSuccess;
        const hipError_t e = hipMalloc((void **)&p, bytes_of(count));
        if (e != hipSuccess) { p = nullptr; return e; }
        live_add(LIVE_DEV, 1, (int64_t)bytes_of(count));
        n = cap = count;
        return hipSuccess;
    }
    // room for `count` elements, contents undefined; the allocation is kept when it is large enough
    hipError_t reserve(size_t count)
    {
        if (count > cap || cap == 0) { const hipError_t e = alloc(count > 0 ? count : 1); if (e != hipSuccess) return e; }
        n = count;
        return hipSuccess;
    }
    // per-frame callers (lights, moved objects) reuse the allocation when the new contents fit
    hipError_t upload(const std::vector<T> &v)
    {
        if (v.size() > cap || (v.empty() && cap == 0)) {
            const hipError_t e = alloc(v.size());
            if (e != hipSuccess) return e;
        }
        n = v.size();
        if (v.empty()) return hipSuccess;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// one word of signal memory (hipExtMallocWithFlags), zeroed: a value a kernel stores and a stream waits for
struct SignalWord {
    uint32_t *p = nullptr;
    SignalWord() = default;
    SignalWord(SignalWord &&o) noexcept : p(o.p) { o.p = nullptr; }
    SignalWord &operator=(SignalWord &&o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~SignalWord() { release(); }
    void release() { if (p) { (void)hipFree(p); live_add(LIVE_DEV, -1, -8); p = nullptr; } }
    hipError_t alloc()
    {
        release();
        hipError_t e = hipExtMallocWithFlags((void **)&p, 8, hipMallocSignalMemory);
        if (e != hipSuccess) { p = nullptr; return e; }
        live_add(LIVE_DEV, 1, 8);
        e = hipMemset(p, 0, 8);
        if (e != hipSuccess) release();
        return e;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { release(); }
    void release() { if (e) { (void)hipEventDestroy(e); g_live[LIVE_EVENTS].fetch_sub(1, std::memory_order_relaxed); e = nullptr; } }
    // the event, made on first use (ordering events carry no timestamps)
    hipError_t ensure(unsigned flags = hipEventDisableTiming)
    {
        if (e) return hipSuccess;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r != hipSuccess) { e = nullptr; return r; }
        g_live[LIVE_EVENTS].fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    operator hipEvent_t() const { return e; }
};

// (the destructor waits for what is queued: a stream is never destroyed under its own work)
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s = o.s; o.s = nullptr; } return *this; }
    ~Stream() { release(); }
    void release() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); g_live[LIVE_STREAMS].fetch_sub(1, std::memory_order_relaxed); s = nullptr; } }
    hipError_t ensure(unsigned flags = hipStreamNonBlocking) { return s ? hipSuccess : made(hipStreamCreateWithFlags(&s, flags)); }
    hipError_t ensure_with_priority(int priority, unsigned flags = hipStreamNonBlocking) { return s ? hipSuccess : made(hipStreamCreateWithPriority(&s, flags, priority)); }
    operator hipStream_t() const { return s; }
private:
    hipError_t made(hipError_t r) { if (r != hipSuccess) s = nullptr; else g_live[LIVE_STREAMS].fetch_add(1, std::memory_order_relaxed); return r; }
};

// grow-only page-locked staging: the block is kept while it is large enough
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~PinnedBuf() { release(); }
    void release() { if (p) { (void)hipHostFree(p); live_add(LIVE_PINNED, -1, -(int64_t)bytes); p = nullptr; } bytes = 0; }
    hipError_t reserve(size_t want, unsigned flags = hipHostMallocDefault)
    {
        if (bytes >= want) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, want, flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        live_add(LIVE_PINNED, 1, (int64_t)want);
        bytes = want;
        return hipSuccess;
    }
    uint8_t *data() const { return static_cast<uint8_t *>(p); }
};

} // namespace ycge_host
