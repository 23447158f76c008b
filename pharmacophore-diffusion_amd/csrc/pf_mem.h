// The handle's memory (pf_host.cpp): buffers, events and streams that own what they hold.  Host only.  Every runtime call goes
// through a policy R -- HipRuntime below is the library's; tests/mem_check.cpp substitutes one that counts, and runs without a GPU.
//   Buf        a device or pinned allocation and its capacity in bytes: move-only, freed by its destructor or by release()
//   reserve    the one growth rule: nothing while the capacity suffices, else wait (as told), free, allocate
//   Event      created on its first use, knows whether it was ever recorded;  Stream: created on first get()
//   StagedBlock  a pinned staging buffer, its device copy and the event of the last upload
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace pfmem {

// The HIP runtime, and the count of what is live through it: allocations and bytes, device and pinned memory together, over the
// whole process (pf_debug_live_memory) -- unlike hipMemGetInfo it does not see other processes on the device
struct HipRuntime {
    static inline std::atomic<int64_t> live_allocations{0}, live_bytes{0};
    static hipError_t counted(hipError_t e, size_t bytes) { if (e == hipSuccess) { ++live_allocations; live_bytes += (int64_t)bytes; } return e; }
    static void uncounted(size_t bytes) { --live_allocations; live_bytes -= (int64_t)bytes; }
    static hipError_t device_alloc(void** p, size_t bytes) { return counted(hipMalloc(p, bytes), bytes); }
    static void device_free(void* p, size_t bytes) { (void)hipFree(p); uncounted(bytes); }
    static hipError_t pinned_alloc(void** p, size_t bytes) { return counted(hipHostMalloc(p, bytes, hipHostMallocDefault), bytes); }
    static void pinned_free(void* p, size_t bytes) { (void)hipHostFree(p); uncounted(bytes); }
    static hipError_t sync_device() { return hipDeviceSynchronize(); }
    static hipError_t sync_stream(hipStream_t s) { return hipStreamSynchronize(s); }
    static hipError_t sync_event(hipEvent_t e) { return hipEventSynchronize(e); }
    static hipError_t event_create(hipEvent_t* e, bool timing) { return hipEventCreateWithFlags(e, timing ? hipEventDefault : hipEventDisableTiming); }
    static hipError_t event_record(hipEvent_t e, hipStream_t s) { return hipEventRecord(e, s); }
    static void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
    static hipError_t stream_create(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
    static void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};

// What reserve() waits for before it frees a buffer that something may still read: the device (launches of earlier batches, on
// any stream), one stream (a run's scratch: several lanes share a device), or nothing (the caller has waited, or nobody reads it)
struct Wait {
    enum Kind { NONE, DEVICE, STREAM } kind;
    hipStream_t stream;
    static Wait none() { return {NONE, nullptr}; }
    static Wait device() { return {DEVICE, nullptr}; }
    static Wait on(hipStream_t s) { return {STREAM, s}; }
};

template <class R, bool PINNED>
class Buf {
    void* p_ = nullptr;
    size_t cap_ = 0;
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Buf() { release(); }
    void release() {
        if (p_) { if (PINNED) R::pinned_free(p_, cap_); else R::device_free(p_, cap_); }
        p_ = nullptr; cap_ = 0;
    }
    // Kept while capacity() >= need (no runtime call); else replaced by an allocation of `want` bytes -- the head room that lets
    // the next request of similar size fit -- after the wait `w`, which an empty buffer skips.  *gone is set when the contents are
    // gone (the buffer is new).  A failed allocation leaves the buffer empty.
    hipError_t reserve(size_t need, size_t want, Wait w, bool* gone = nullptr) {
        if (cap_ >= need) return hipSuccess;
        if (p_) {
            const hipError_t e = w.kind == Wait::DEVICE ? R::sync_device() : w.kind == Wait::STREAM ? R::sync_stream(w.stream) : hipSuccess;
            if (e != hipSuccess) return e;
            release();
        }
        const hipError_t e = PINNED ? R::pinned_alloc(&p_, want) : R::device_alloc(&p_, want);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = want;
        if (gone) *gone = true;
        return hipSuccess;
    }
    size_t capacity() const { return cap_; }
    void* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T> T* as() const { return static_cast<T*>(p_); }
};

// A buffer of one element type that reads like the pointer it replaces (h->d_w + offset, kernel arguments)
template <class T, class R, bool PINNED>
struct Arr : Buf<R, PINNED> {
    operator T*() const { return this->template as<T>(); }
};

template <class R>
class EventT {
    hipEvent_t ev_ = nullptr;
    bool timing_ = false, recorded_ = false;
public:
    explicit EventT(bool timing = false) : timing_(timing) {}
    EventT(EventT&& o) noexcept : ev_(o.ev_), timing_(o.timing_), recorded_(o.recorded_) { o.ev_ = nullptr; o.recorded_ = false; }
    EventT& operator=(EventT&&) = delete;
    ~EventT() { if (ev_) R::event_destroy(ev_); }
    hipError_t get(hipEvent_t* out) {
        const hipError_t e = ev_ ? hipSuccess : R::event_create(&ev_, timing_);
        *out = ev_;
        return e;
    }
    hipError_t record(hipStream_t s) {
        hipEvent_t ev;
        hipError_t e = get(&ev);
        if (e == hipSuccess && (e = R::event_record(ev, s)) == hipSuccess) recorded_ = true;
        return e;
    }
    bool recorded() const { return recorded_; }
    void forget() { recorded_ = false; }                                    // what was recorded no longer guards anything
    hipError_t sync() { return recorded_ ? R::sync_event(ev_) : hipSuccess; }
    // `s` goes on once the last record has completed (nothing recorded: nothing to wait for)
    hipError_t hold(hipStream_t s) { return recorded_ ? hipStreamWaitEvent(s, ev_, 0) : hipSuccess; }
};

template <class R>
class StreamT {
    hipStream_t s_ = nullptr;
public:
    StreamT() = default;
    StreamT(const StreamT&) = delete;
    StreamT& operator=(const StreamT&) = delete;
    ~StreamT() { if (s_) R::stream_destroy(s_); }
    hipError_t get(hipStream_t* out) {
        const hipError_t e = s_ ? hipSuccess : R::stream_create(&s_);
        *out = s_;
        return e;
    }
};

// A block of host arrays that goes to the device in one copy: packed into `stage` (pinned) in the device layout, then copied into
// `dev`, which the caller reserves like any run scratch before it enqueues anything.  ev: the last upload out of `stage`.
// (Members are destroyed in reverse order: dev, stage, ev.)
template <class R>
struct StagedBlockT {
    EventT<R> ev;
    Buf<R, true> stage;
    Buf<R, false> dev;
    // the last upload has read the staging buffer, which then holds `bytes` (grown to twice that) for the caller to pack into
    hipError_t reserve(size_t bytes) {
        const hipError_t e = ev.sync();
        return e != hipSuccess ? e : stage.reserve(bytes, bytes * 2, Wait::none());
    }
    hipError_t upload(size_t bytes, hipStream_t s) {
        const hipError_t e = hipMemcpyAsync(dev.get(), stage.get(), bytes, hipMemcpyHostToDevice, s);
        return e != hipSuccess ? e : ev.record(s);
    }
};

using DevBuf = Buf<HipRuntime, false>;
using PinnedBuf = Buf<HipRuntime, true>;
template <class T> using DevArr = Arr<T, HipRuntime, false>;
template <class T> using PinnedArr = Arr<T, HipRuntime, true>;
using Event = EventT<HipRuntime>;
using Stream = StreamT<HipRuntime>;
using StagedBlock = StagedBlockT<HipRuntime>;

}  // namespace pfmem
