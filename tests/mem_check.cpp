// The handle's owning types (csrc/pf_mem.h) as a program of its own: a counting policy stands in for the HIP runtime and logs every
// call, so the growth rule, the moves, the lazy events and streams and the staged block are checked call for call.  Built with the
// address and undefined-behaviour sanitizers by tests/test_mem_host.py; no HIP runtime call, no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "pf_mem.h"

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++failures; } } while (0)

// Every call appends one word to `log` ("dev_alloc:96", "sync_stream", ...); memory comes from malloc, so the sanitizers see a
// double free or a leak; events and streams are small heap objects for the same reason.  fail_at: the k-th allocation from now is refused
struct Counting {
    static inline std::vector<std::string> log;
    static inline long live = 0, live_bytes = 0, live_events = 0, live_streams = 0;
    static inline int fail_at = 0;
    static inline hipStream_t last_stream = nullptr;
    static hipError_t alloc(const char* what, void** p, size_t bytes) {
        log.push_back(std::string(what) + ":" + std::to_string(bytes));
        if (fail_at > 0 && --fail_at == 0) { *p = reinterpret_cast<void*>(0x10); return hipErrorOutOfMemory; }    // (a refused call may leave rubbish behind)
        *p = std::malloc(bytes ? bytes : 1);
        ++live; live_bytes += (long)bytes;
        return hipSuccess;
    }
    static void release(const char* what, void* p, size_t bytes) { log.push_back(what); std::free(p); --live; live_bytes -= (long)bytes; }
    static hipError_t device_alloc(void** p, size_t bytes) { return alloc("dev_alloc", p, bytes); }
    static void device_free(void* p, size_t bytes) { release("dev_free", p, bytes); }
    static hipError_t pinned_alloc(void** p, size_t bytes) { return alloc("pin_alloc", p, bytes); }
    static void pinned_free(void* p, size_t bytes) { release("pin_free", p, bytes); }
    static hipError_t sync_device() { log.push_back("sync_device"); return hipSuccess; }
    static hipError_t sync_stream(hipStream_t s) { log.push_back("sync_stream"); last_stream = s; return hipSuccess; }
    static hipError_t sync_event(hipEvent_t) { log.push_back("sync_event"); return hipSuccess; }
    static hipError_t event_create(hipEvent_t* e, bool timing) {
        log.push_back(timing ? "event_create:timing" : "event_create");
        *e = reinterpret_cast<hipEvent_t>(std::malloc(1)); ++live_events;
        return hipSuccess;
    }
    static hipError_t event_record(hipEvent_t, hipStream_t) { log.push_back("event_record"); return hipSuccess; }
    static void event_destroy(hipEvent_t e) { log.push_back("event_destroy"); std::free(e); --live_events; }
    static hipError_t stream_create(hipStream_t* s) { log.push_back("stream_create"); *s = reinterpret_cast<hipStream_t>(std::malloc(1)); ++live_streams; return hipSuccess; }
    static void stream_destroy(hipStream_t s) { log.push_back("stream_destroy"); std::free(s); --live_streams; }
};
using Dev = pfmem::Buf<Counting, false>;
using Pin = pfmem::Buf<Counting, true>;
using Ev = pfmem::EventT<Counting>;
using St = pfmem::StreamT<Counting>;
using Blk = pfmem::StagedBlockT<Counting>;
using pfmem::Wait;

using Log = std::vector<std::string>;
static Log take_log() { Log l; l.swap(Counting::log); return l; }
static int count(const Log& l, const std::string& w) { int n = 0; for (const auto& x : l) n += x == w; return n; }
// every scenario ends balanced: nothing live, nothing logged that was not looked at
static void balanced(const char* what) {
    if (Counting::live || Counting::live_bytes || Counting::live_events || Counting::live_streams) {
        std::printf("FAILED: %s leaves %ld allocations, %ld bytes, %ld events, %ld streams\n", what, Counting::live, Counting::live_bytes,
                    Counting::live_events, Counting::live_streams);
        ++failures;
    }
    Counting::log.clear();
}

// reserve at the boundaries, for one buffer kind and one wait
template <class B>
static void reserve_boundaries(const char* alloc, const char* free_, Wait w, const char* wait_word) {
    const size_t n = 96;
    hipStream_t stream = reinterpret_cast<hipStream_t>(0x40);
    if (w.kind == Wait::STREAM) w.stream = stream;
    {
        B b;
        bool gone = false;
        CHECK(b.reserve(0, 0, w, &gone) == hipSuccess);                     // need 0 on an empty buffer: nothing
        CHECK(take_log().empty() && !gone && !b && b.capacity() == 0);
        CHECK(b.reserve(n, n, w, &gone) == hipSuccess);                     // an empty buffer: no wait, no free
        CHECK(take_log() == Log{std::string(alloc) + ":96"});
        CHECK(gone && b && b.capacity() == n && b.template as<char>() == b.get());
        gone = false;
        CHECK(b.reserve(n, 4 * n, w, &gone) == hipSuccess);                 // need == n: no call at all
        CHECK(b.reserve(1, 1, w, &gone) == hipSuccess && b.reserve(0, 0, w, &gone) == hipSuccess);
        CHECK(take_log().empty() && !gone && b.capacity() == n);
        CHECK(b.reserve(n + 1, 2 * n + 8, w, &gone) == hipSuccess);         // need == n + 1: the wait, one free, one allocation of `want`
        Log expect;
        if (wait_word) expect.push_back(wait_word);
        expect.push_back(free_); expect.push_back(std::string(alloc) + ":200");
        CHECK(take_log() == expect);
        CHECK(gone && b.capacity() == 2 * n + 8 && Counting::live == 1 && Counting::live_bytes == (long)(2 * n + 8));
        if (w.kind == Wait::STREAM) CHECK(Counting::last_stream == stream);
        static_cast<char*>(b.get())[2 * n + 7] = 1;                          // (the whole of `want` is there)
        CHECK(b.reserve(n, n, w) == hipSuccess && take_log().empty());      // kept, never shrunk; no report asked for
    }
    CHECK(take_log() == Log{free_});                                        // the destructor frees
    balanced("reserve_boundaries");
}

static void failing_allocation() {
    for (int pinned = 0; pinned < 2; ++pinned) {
        Dev d; Pin p;
        bool gone = false;
        auto reserve = [&](size_t need, size_t want) { return pinned ? p.reserve(need, want, Wait::device(), &gone) : d.reserve(need, want, Wait::device(), &gone); };
        CHECK(reserve(64, 64) == hipSuccess);
        take_log(); gone = false;
        Counting::fail_at = 1;
        CHECK(reserve(65, 128) == hipErrorOutOfMemory);                     // the old memory went exactly once, nothing dangles
        const Log l = take_log();
        CHECK(count(l, pinned ? "pin_free" : "dev_free") == 1 && l.size() == 3 && l[0] == "sync_device");
        CHECK(!gone && Counting::live == 0);
        CHECK(pinned ? (!p && p.get() == nullptr && p.capacity() == 0) : (!d && d.get() == nullptr && d.capacity() == 0));
        CHECK(reserve(65, 128) == hipSuccess);                              // and the buffer is usable again: no wait, no free
        CHECK(take_log().size() == 1 && gone);
        Counting::fail_at = 2;                                              // the second allocation from here: this one passes ...
        Dev other;
        CHECK(other.reserve(8, 8, Wait::none()) == hipSuccess);
        CHECK(other.reserve(9, 16, Wait::none()) == hipErrorOutOfMemory);   // ... and the k-th fails, on a buffer that held something
        CHECK(!other && other.capacity() == 0);
        Counting::fail_at = 0;
    }
    balanced("failing_allocation");
}

static void moves() {
    {
        Dev a;
        CHECK(a.reserve(32, 32, Wait::none()) == hipSuccess);
        void* const p = a.get();
        Dev b(std::move(a));                                                // construction: the source is empty, nothing is freed
        CHECK(!a && a.capacity() == 0 && b.get() == p && b.capacity() == 32);
        Dev c;
        CHECK(c.reserve(16, 16, Wait::none()) == hipSuccess);
        take_log();
        c = std::move(b);                                                   // assignment: the target's own memory goes, the source's moves
        CHECK(take_log() == Log{"dev_free"} && !b && c.get() == p && c.capacity() == 32);
        Dev& self = c;
        c = std::move(self);                                                // self-assignment: harmless
        CHECK(take_log().empty() && c.get() == p && c.capacity() == 32);
        a.release(); b.release();                                           // empty buffers: nothing
        CHECK(take_log().empty());
    }
    CHECK(take_log() == Log{"dev_free"});                                   // one free in total for p, none from the moved-from sources
    {
        Pin p;
        CHECK(p.reserve(8, 8, Wait::none()) == hipSuccess);
        take_log();
        p.release(); p.release();                                           // twice: one free
        CHECK(take_log() == Log{"pin_free"} && !p && p.capacity() == 0);
    }
    CHECK(take_log().empty());
    balanced("moves");
}

static void events_and_streams() {
    hipStream_t s = reinterpret_cast<hipStream_t>(0x40);
    {
        Ev e; Ev timed(true); St st;
        CHECK(take_log().empty() && !e.recorded());                         // nothing is created before the first use
        CHECK(e.sync() == hipSuccess && take_log().empty());                // never recorded: nothing to wait for
        hipEvent_t h1 = nullptr, h2 = nullptr;
        CHECK(e.get(&h1) == hipSuccess && e.get(&h2) == hipSuccess && h1 && h1 == h2);
        CHECK(take_log() == Log{"event_create"} && !e.recorded());          // one create however often; still not recorded
        CHECK(e.record(s) == hipSuccess && e.recorded() && take_log() == Log{"event_record"});
        CHECK(e.sync() == hipSuccess && take_log() == Log{"sync_event"});
        e.forget();
        CHECK(!e.recorded() && e.sync() == hipSuccess && take_log().empty());
        CHECK(timed.record(s) == hipSuccess && (take_log() == Log{"event_create:timing", "event_record"}));
        Ev moved(std::move(timed));                                         // (a vector of events grows by moving them)
        CHECK(moved.recorded() && !timed.recorded() && take_log().empty());
        hipStream_t s1 = nullptr, s2 = nullptr;
        CHECK(st.get(&s1) == hipSuccess && st.get(&s2) == hipSuccess && s1 && s1 == s2 && take_log() == Log{"stream_create"});
    }
    const Log l = take_log();                                               // e, moved and the stream: one destroy each, none for the moved-from one
    CHECK(count(l, "event_destroy") == 2 && count(l, "stream_destroy") == 1 && l.size() == 3);
    { Ev never; St nor_this; }
    CHECK(take_log().empty());                                              // never used: never created, nothing to destroy
    balanced("events_and_streams");
}

static void staged_block() {
    hipStream_t s = reinterpret_cast<hipStream_t>(0x40);
    {
        Blk b;
        CHECK(b.reserve(100) == hipSuccess);                                // no event recorded: no wait; the pinned half is twice the bytes
        CHECK(take_log() == Log{"pin_alloc:200"} && b.stage.capacity() == 200 && !b.dev && !b.ev.recorded());
        CHECK(b.reserve(200) == hipSuccess && take_log().empty());          // fits: nothing (and still nothing recorded)
        CHECK(b.dev.reserve(100, 200, Wait::on(s)) == hipSuccess);          // the device half is the caller's to reserve
        take_log();
        CHECK(b.ev.record(s) == hipSuccess);                                // (what upload() ends with)
        take_log();
        CHECK(b.reserve(150) == hipSuccess && take_log() == Log{"sync_event"});                        // recorded: the wait, and nothing else while it fits
        CHECK(b.reserve(201) == hipSuccess && (take_log() == Log{"sync_event", "pin_free", "pin_alloc:402"}));
        CHECK(b.dev.capacity() == 200 && b.stage.capacity() == 402);        // reserve never touches the device half
    }
    const Log l = take_log();                                               // the destructor releases all three parts: buffers first, then the event
    CHECK((l == Log{"dev_free", "pin_free", "event_destroy"}));
    balanced("staged_block");
}

int main() {
    reserve_boundaries<Dev>("dev_alloc", "dev_free", Wait::device(), "sync_device");
    reserve_boundaries<Dev>("dev_alloc", "dev_free", Wait::on(nullptr), "sync_stream");
    reserve_boundaries<Dev>("dev_alloc", "dev_free", Wait::none(), nullptr);
    reserve_boundaries<Pin>("pin_alloc", "pin_free", Wait::none(), nullptr);
    reserve_boundaries<Pin>("pin_alloc", "pin_free", Wait::device(), "sync_device");
    failing_allocation();
    moves();
    events_and_streams();
    staged_block();
    // a typed array reads like the pointer it replaces
    {
        pfmem::Arr<int, Counting, false> a;
        CHECK(a.reserve(16, 16, Wait::none()) == hipSuccess);
        int* p = a;
        CHECK(p == a.as<int>() && a + 2 == p + 2 && a);
        p[3] = 7;
        CHECK(a[3] == 7);
    }
    balanced("typed array");
    if (failures) { std::printf("mem_check: %d checks FAILED\n", failures); return 1; }
    std::printf("mem_check: all checks passed\n");
    return 0;
}
