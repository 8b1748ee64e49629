// Internal: the types that own a runtime resource and give it back in their destructor — device memory, page-locked host memory, events, streams — and the base of
// every lazily created module state.  A struct made of these needs no release list: destroying it frees what it holds.  The owner's device must be current, and its
// streams drained, when that happens (lili_ctx_destroy).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <memory>

namespace lili_detail {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes + 256 <= cap) return hipSuccess;      // (every buffer keeps >= 256 bytes of slack behind what was asked for: kernels may read whole 16-byte vectors at the end)
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
    void swap(DevBuf& o) { void* tp = p; p = o.p; o.p = tp; size_t tc = cap; cap = o.cap; o.cap = tc; }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }   // lili_ctx_destroy deletes the context with its device current
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Page-locked host memory.  Grow-only and exact: the call site decides how much more than it needs it asks for.
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipHostFree(p); p = nullptr; cap = 0; d = nullptr; asked = false; if (e != hipSuccess) return e; }
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    // the memory as the device sees it, or nullptr where the runtime has no such address (asked once per allocation)
    void* dev() {
        if (p && !asked) {
            asked = true;
            if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }
        }
        return d;
    }
    void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; d = nullptr; asked = false; } }
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    template <class T> T* dev_as() { return reinterpret_cast<T*>(dev()); }

private:
    void* d = nullptr;
    bool asked = false;
};

// An event created on first use.  Reads as a hipEvent_t wherever one is recorded or waited for.
struct Event {
    hipEvent_t e = nullptr;
    hipError_t get(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    void release() { if (e) { (void)hipEventDestroy(e); e = nullptr; } }
    operator hipEvent_t() const { return e; }
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { release(); }
};

// A non-blocking stream created on first use, with a priority where the caller names one.
struct Stream {
    hipStream_t s = nullptr;
    hipError_t get() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t get(int priority) { return s ? hipSuccess : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
    void release() { if (s) { (void)hipStreamDestroy(s); s = nullptr; } }
    operator hipStream_t() const { return s; }
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { release(); }
};

// A call whose branches run side by side: branch i > 0 on side[i], behind the event begin() records on the main stream, and joined back into the main stream by
// join[i]; branch 0 on the main stream itself — no event, no other stream.  `current` is the owner's "stream the launch helpers enqueue on": it is a side stream
// only between fork(i) and join(i), and the destructor puts the main stream back on whatever path the call leaves.
struct ForkJoin {
    ForkJoin(hipStream_t& current, Event& fork_ev, Stream* side, Event* join_ev) : current(current), home(current), fork_ev(fork_ev), side(side), join_ev(join_ev) {}
    ForkJoin(const ForkJoin&) = delete;
    ForkJoin& operator=(const ForkJoin&) = delete;
    ~ForkJoin() { current = home; }
    hipError_t begin() {
        const hipError_t e = fork_ev.get();
        return e != hipSuccess ? e : hipEventRecord(fork_ev, home);
    }
    hipError_t fork(int i) {
        if (i == 0) return hipSuccess;
        hipError_t e = side[i].get();
        if (e == hipSuccess) e = join_ev[i].get();
        if (e == hipSuccess) e = hipStreamWaitEvent(side[i], fork_ev, 0);
        if (e == hipSuccess) current = side[i];
        return e;
    }
    hipError_t join(int i) {
        if (i == 0) return hipSuccess;
        const hipError_t e = hipEventRecord(join_ev[i], side[i]);
        current = home;
        return e != hipSuccess ? e : hipStreamWaitEvent(home, join_ev[i], 0);
    }

private:
    hipStream_t& current;
    const hipStream_t home;      // the main stream: what `current` was when the call began
    Event& fork_ev;
    Stream* side;
    Event* join_ev;
};

// What a module keeps per context (lili_ctx::ext): created by the module's first call, deleted with the context.
struct ExtState { virtual ~ExtState() = default; };

}  // namespace lili_detail
