// Stand-alone check of the owner types in lili_om_amd/csrc/lili_own.h, built and run by tests/test_own_cpu.py under the address and undefined-behaviour
// sanitizers.  The runtime calls the header uses are counting stand-ins on malloc / free: every resource is tracked while it lives, a free of something that
// is not live is recorded as an error, and two switches make the next allocation / the device-pointer query fail.  Exits non-zero at the first failed check.
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
bool g_fail_alloc = false, g_fail_devptr = false;

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

int main() {
    check_devbuf();
    check_pinbuf();
    check_event_and_stream();
    check_ext_states();
    CHECK(live_total() == 0 && g_bad_frees == 0);
    std::puts("own_check: ok");
    return 0;
}
