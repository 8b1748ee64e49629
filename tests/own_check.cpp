// Stand-alone check of the owner types in lili_om_amd/csrc/lili_own.h, built and run by tests/test_own_cpu.py under the address and undefined-behaviour
// sanitizers.  The runtime calls the header uses are counting stand-ins on malloc / free: every resource is tracked while it lives, a free of something that
// is not live is recorded as an error, and two switches make the next allocation / the device-pointer query fail.  Event records and stream waits (ForkJoin) are logged in order; a third switch fails them.  Exits non-zero at the first failed check.
#include "../lili_om_amd/csrc/lili_own.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

namespace {
struct Kind { std::set<void*> live; int made = 0, freed = 0; };
Kind g_dev, g_pin, g_event, g_stream;
std::map<void*, void*> g_dev_of_pin;      // what the device-pointer query answers for a live page-locked block (a fresh value per allocation)
uintptr_t g_next_dev = 0x1000;
int g_bad_frees = 0, g_last_error_reads = 0;
bool g_fail_alloc = false, g_fail_devptr = false, g_fail_enqueue = false;
struct Op { char what; void* event; void* stream; };
std::vector<Op> g_ops;
bool same(const Op& o, char what, void* event, void* stream) { return o.what == what && o.event == event && o.stream == stream; }

hipError_t make(Kind& k, void** out, size_t bytes) {
    if (g_fail_alloc) return hipErrorOutOfMemory;
    void* p = std::malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    k.live.insert(p); k.made++;
    *out = p;
    return hipSuccess;
}
hipError_t drop(Kind& k, void* p) {
    if (!k.live.erase(p)) { g_bad_frees++; return hipErrorInvalidValue; }
    k.freed++;
    std::free(p);
    return hipSuccess;
}
size_t live_total() { return g_dev.live.size() + g_pin.live.size() + g_event.live.size() + g_stream.live.size(); }

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "own_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return make(g_dev, p, bytes); }
hipError_t hipFree(void* p) { return drop(g_dev, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
    const hipError_t e = make(g_pin, p, bytes);
    if (e == hipSuccess) { g_dev_of_pin[*p] = reinterpret_cast<void*>(g_next_dev); g_next_dev += 0x1000; }
    return e;
}
hipError_t hipHostFree(void* p) { g_dev_of_pin.erase(p); return drop(g_pin, p); }
hipError_t hipHostGetDevicePointer(void** d, void* host, unsigned int) {
    const auto it = g_dev_of_pin.find(host);
    if (g_fail_devptr || it == g_dev_of_pin.end()) return hipErrorInvalidValue;
    *d = it->second;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { g_last_error_reads++; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(g_event, reinterpret_cast<void**>(e), 8); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(g_event, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return make(g_stream, reinterpret_cast<void**>(s), 8); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return make(g_stream, reinterpret_cast<void**>(s), 8); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(g_stream, s); }
// what ForkJoin enqueues: logged in order ('R'ecord / 'W'ait, the event, the stream); `g_fail_enqueue` makes every such call fail
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { g_ops.push_back({'R', e, s}); return g_fail_enqueue ? hipErrorInvalidValue : hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) { g_ops.push_back({'W', e, s}); return g_fail_enqueue ? hipErrorInvalidValue : hipSuccess; }
}

using namespace lili_detail;

static void check_devbuf() {
    DevBuf b;
    CHECK(b.ensure(1000) == hipSuccess && b.p && b.cap == 1000 + 125 + 256 && g_dev.made == 1);
    void* first = b.p;
    CHECK(b.ensure(0) == hipSuccess && b.ensure(b.cap - 256) == hipSuccess);      // within cap - 256: the same block
    CHECK(b.p == first && g_dev.made == 1 && g_dev.freed == 0);
    CHECK(b.ensure(b.cap - 255) == hipSuccess);                                    // one byte more: one free, one allocation
    CHECK(g_dev.made == 2 && g_dev.freed == 1 && g_dev.live.size() == 1 && b.cap == 1126 + 1126 / 8 + 256);
    DevBuf c;
    CHECK(c.ensure(10) == hipSuccess);
    void *bp = b.p, *cp = c.p; const size_t bc = b.cap, cc = c.cap;
    b.swap(c);
    CHECK(b.p == cp && b.cap == cc && c.p == bp && c.cap == bc);
    g_fail_alloc = true;
    CHECK(b.ensure(1 << 20) != hipSuccess && b.p == nullptr && b.cap == 0);       // the old block is gone, nothing replaced it
    DevBuf d;
    CHECK(d.ensure(16) != hipSuccess && d.p == nullptr && d.cap == 0);
    g_fail_alloc = false;
    CHECK(g_dev.live.size() == 1);
    c.release(); c.release(); d.release();
    CHECK(c.p == nullptr && c.cap == 0 && g_dev.live.empty() && g_bad_frees == 0);
    CHECK(d.as<int>() == nullptr);
}

static void check_pinbuf() {
    PinBuf b;
    CHECK(b.dev() == nullptr && g_pin.made == 0);      // nothing allocated, nothing asked
    CHECK(b.ensure(64) == hipSuccess && b.p && b.cap == 64 && g_pin.made == 1);
    void* first = b.p;
    CHECK(b.ensure(64) == hipSuccess && b.ensure(1) == hipSuccess && b.ensure(0) == hipSuccess);
    CHECK(b.p == first && b.cap == 64 && g_pin.made == 1 && g_pin.freed == 0);
    void* d0 = b.dev();
    CHECK(d0 && d0 == g_dev_of_pin[b.p] && b.dev_as<char>() == d0);
    CHECK(b.ensure(65) == hipSuccess && b.cap == 65 && g_pin.made == 2 && g_pin.freed == 1 && g_pin.live.size() == 1);
    CHECK(b.dev() == g_dev_of_pin[b.p] && b.dev() != d0);      // the regrown block's address, not the freed one's
    b.release(); b.release();
    CHECK(b.p == nullptr && b.cap == 0 && b.dev() == nullptr && g_pin.live.empty());
    g_fail_devptr = true;
    const int reads = g_last_error_reads;
    CHECK(b.ensure(32) == hipSuccess && b.dev() == nullptr && b.as<int>() != nullptr);
    CHECK(g_last_error_reads == reads + 1);                      // the failed query's error does not stay with the runtime
    g_fail_devptr = false;
    g_fail_alloc = true;
    CHECK(b.ensure(1024) != hipSuccess && b.p == nullptr && b.cap == 0 && b.dev() == nullptr);
    g_fail_alloc = false;
    CHECK(g_pin.live.empty() && g_bad_frees == 0);
}

static void check_event_and_stream() {
    {
        Event never;
        Stream idle;
        CHECK(!never && !idle);
    }
    CHECK(g_event.made == 0 && g_stream.made == 0);
    {
        Event e;
        for (int i = 0; i < 5; i++) CHECK(e.get() == hipSuccess);
        CHECK(e.get(hipEventDefault) == hipSuccess && g_event.made == 1 && static_cast<hipEvent_t>(e) == e.e && e.e);
        Stream s, lo;
        for (int i = 0; i < 3; i++) CHECK(s.get() == hipSuccess && lo.get(1) == hipSuccess);
        CHECK(g_stream.made == 2 && static_cast<hipStream_t>(s) == s.s);
        lo.release(); lo.release();
        CHECK(g_stream.live.size() == 1);
        g_fail_alloc = true;
        Event f;
        CHECK(f.get() != hipSuccess && !f);
        g_fail_alloc = false;
    }
    CHECK(g_event.made == 1 && g_event.freed == 1 && g_stream.freed == 2 && g_event.live.empty() && g_stream.live.empty() && g_bad_frees == 0);
    Event e;
    CHECK(e.get() == hipSuccess);
    e.release(); e.release();
    CHECK(g_event.live.empty() && g_bad_frees == 0);
}

// a context-like holder of module states: deleting it must free everything below it, with no release list anywhere
struct Child { DevBuf pts; };
struct StateA : ExtState { DevBuf d; PinBuf h; Event ev; std::vector<std::unique_ptr<Child>> kids; };
struct StateB : ExtState { DevBuf d[3]; PinBuf h; Event ev; Stream side; std::vector<std::unique_ptr<Child>> kids; std::unique_ptr<ExtState> inner; };
struct StateC : ExtState {
    DevBuf d; PinBuf h; Event ev; std::vector<std::unique_ptr<Child>> kids;
    bool* waited;
    explicit StateC(bool* w) : waited(w) {}
    ~StateC() override { *waited = !kids.empty() && kids[0]->pts.p != nullptr; }      // a destructor body runs while the members still hold what they own
};
struct Holder { DevBuf own; PinBuf pin; Event ev[2]; Stream side[2]; std::unique_ptr<ExtState> ext[3]; };

template <class S> static void fill(S* s, int n_kids) {
    CHECK(s->h.ensure(128) == hipSuccess && s->h.dev() && s->ev.get() == hipSuccess);
    for (int i = 0; i < n_kids; i++) { s->kids.emplace_back(new Child()); CHECK(s->kids.back()->pts.ensure(100 * (i + 1)) == hipSuccess); }
}

static void check_ext_states() {
    const int made[4] = {g_dev.made, g_pin.made, g_event.made, g_stream.made};
    bool waited = false;
    {
        Holder* H = new Holder();
        CHECK(H->own.ensure(512) == hipSuccess && H->pin.ensure(64) == hipSuccess && H->ev[1].get() == hipSuccess && H->side[0].get() == hipSuccess);
        StateA* a = new StateA(); H->ext[0].reset(a);
        CHECK(a->d.ensure(10) == hipSuccess); fill(a, 3);
        StateB* b = new StateB(); H->ext[1].reset(b);
        CHECK(b->d[0].ensure(10) == hipSuccess && b->d[2].ensure(30) == hipSuccess && b->side.get() == hipSuccess); fill(b, 2);
        StateA* in = new StateA(); b->inner.reset(in);      // a state one level down (the loop's and the global map's private filters)
        CHECK(in->d.ensure(77) == hipSuccess); fill(in, 1);
        StateC* c = new StateC(&waited); H->ext[2].reset(c);
        CHECK(c->d.ensure(1) == hipSuccess); fill(c, 4);
        c->kids.erase(c->kids.begin() + 1);                  // a keyframe that leaves the ring frees itself
        CHECK(live_total() == (1 + 1 + 1 + 1) + (1 + 1 + 1 + 3) + (2 + 1 + 1 + 1 + 2) + (1 + 1 + 1 + 1) + (1 + 1 + 1 + 3));
        delete H;
    }
    CHECK(waited);
    CHECK(live_total() == 0 && g_bad_frees == 0);
    CHECK(g_dev.made - made[0] == 1 + 4 + 4 + 2 + 5 && g_pin.made - made[1] == 5 && g_event.made - made[2] == 5 && g_stream.made - made[3] == 2);
    CHECK(g_dev.made == g_dev.freed && g_pin.made == g_pin.freed && g_event.made == g_event.freed && g_stream.made == g_stream.freed);
    Holder half;      // a half-built holder (a failed create): nothing to free, nothing freed
    (void)half;
}

// a context-like owner of the streams and events ForkJoin works on; `work` stands for a launch helper: it enqueues on `stream`, whatever that is at the time
struct Forker {
    hipStream_t stream;
    Stream side[4];
    Event fork_ev, join_ev[4];
    void work() { g_ops.push_back({'K', nullptr, stream}); }
    // three branches, leaving early — between fork and join — in branch `leave_in` (-1: never)
    hipError_t run(int leave_in) {
        ForkJoin fj(stream, fork_ev, side, join_ev);
        hipError_t e = fj.begin();
        for (int i = 0; i < 3 && e == hipSuccess; i++) {
            if ((e = fj.fork(i)) != hipSuccess) return e;
            work();
            if (i == leave_in) return hipErrorUnknown;
            e = fj.join(i);
        }
        return e;
    }
};

static void check_fork_join() {
    int main_tag = 0;
    hipStream_t const main_stream = reinterpret_cast<hipStream_t>(&main_tag);
    const int events0 = g_event.made, streams0 = g_stream.made;
    {
        Forker f;
        f.stream = main_stream;
        {   // branch 0 alone: no event, no stream, nothing enqueued but the work — on the main stream
            ForkJoin fj(f.stream, f.fork_ev, f.side, f.join_ev);
            g_ops.clear();
            CHECK(fj.fork(0) == hipSuccess && f.stream == main_stream);
            f.work();
            CHECK(fj.join(0) == hipSuccess && f.stream == main_stream);
            CHECK(g_ops.size() == 1 && same(g_ops[0], 'K', nullptr, main_stream));
            CHECK(g_event.made == events0 && g_stream.made == streams0 && !f.fork_ev && !f.side[0] && !f.join_ev[0]);
        }
        // a whole call: fork -> work -> join per branch, in this order on these streams; the main stream is current again at the end
        g_ops.clear();
        CHECK(f.run(-1) == hipSuccess && f.stream == main_stream);
        CHECK(g_event.made == events0 + 3 && g_stream.made == streams0 + 2 && !f.side[0] && !f.join_ev[0]);      // fork_ev, join_ev[1..2]; side[1..2]
        hipStream_t s1 = f.side[1], s2 = f.side[2];
        hipEvent_t fe = f.fork_ev, j1 = f.join_ev[1], j2 = f.join_ev[2];
        const Op want[] = {{'R', fe, main_stream}, {'K', nullptr, main_stream},
                           {'W', fe, s1}, {'K', nullptr, s1}, {'R', j1, s1}, {'W', j1, main_stream},
                           {'W', fe, s2}, {'K', nullptr, s2}, {'R', j2, s2}, {'W', j2, main_stream}};
        CHECK(g_ops.size() == sizeof(want) / sizeof(want[0]));
        for (size_t i = 0; i < g_ops.size(); i++) CHECK(same(g_ops[i], want[i].what, want[i].event, want[i].stream));
        // a second call creates nothing more
        CHECK(f.run(-1) == hipSuccess && g_event.made == events0 + 3 && g_stream.made == streams0 + 2);
        // an early return with a branch still open: the work went to the side stream, the main stream is current afterwards, nothing was joined
        g_ops.clear();
        CHECK(f.run(2) == hipErrorUnknown && f.stream == main_stream);
        CHECK(g_ops.size() == 8 && same(g_ops[7], 'K', nullptr, s2));
        CHECK(f.run(0) == hipErrorUnknown && f.stream == main_stream);
        // a failing enqueue: fork leaves the main stream current; join puts it back before it reports
        {
            ForkJoin fj(f.stream, f.fork_ev, f.side, f.join_ev);
            g_fail_enqueue = true;
            CHECK(fj.begin() != hipSuccess && fj.fork(1) != hipSuccess && f.stream == main_stream);
            g_fail_enqueue = false;
            CHECK(fj.fork(1) == hipSuccess && f.stream == s1);
            g_fail_enqueue = true;
            CHECK(fj.join(1) != hipSuccess && f.stream == main_stream);
            g_fail_enqueue = false;
        }
        // a stream or an event that cannot be created: the same
        Forker g;
        g.stream = main_stream;
        g_fail_alloc = true;
        CHECK(g.run(-1) != hipSuccess && g.stream == main_stream && !g.fork_ev);
        g_fail_alloc = false;
    }
    CHECK(g_event.live.empty() && g_stream.live.empty() && g_bad_frees == 0);
}

int main() {
    check_devbuf();
    check_pinbuf();
    check_event_and_stream();
    check_ext_states();
    check_fork_join();
    CHECK(live_total() == 0 && g_bad_frees == 0);
    std::puts("own_check: ok");
    return 0;
}
