// The contract of a caller's cloud (lili_om_amd/csrc/lili_cloud_source.h) on the CPU: what cloud_fault refuses, condition by condition at its boundary, and where
// plan_sources has the rows of n clouds read from — the named cases, then a seeded random sweep against the two-pass code the readers used to repeat.
// Built and run by tests/test_cloud_source_cpu.py under the address and undefined-behaviour sanitizers.
#include "../lili_om_amd/csrc/lili_cloud_source.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

using lili_detail::CloudSource;
using lili_detail::SourcePolicy;
using lili_detail::cloud_fault;
using lili_detail::kReadPinnedInPlace;
using lili_detail::kStageHostAlways;
using lili_detail::plan_sources;

static int g_failed = 0;
static const char* g_case = "";
#define CHECK(cond) do { if (!(cond)) { std::printf("%s: FAILED line %d: %s\n", g_case, __LINE__, #cond); g_failed++; } } while (0)

// addresses that are never read: host rows, and the device-side address the table gives a page-locked one
static const void* host_at(size_t i) { return reinterpret_cast<const void*>(0x10000 + 0x1000 * i); }
static void* dev_of(const void* host) { return reinterpret_cast<void*>(reinterpret_cast<size_t>(host) + 0x70000000); }

// the "page-locked?" query as a table that counts how often each address is asked
struct PinTable {
    std::map<const void*, bool> locked;
    std::map<const void*, int> asked;
    int calls = 0;
    void* operator()(const void* p) {
        calls++; asked[p]++;
        auto it = locked.find(p);
        return it != locked.end() && it->second ? dev_of(p) : nullptr;
    }
};

static lili_cloud cloud(const void* data, size_t n, size_t stride, int aux, int mem) { lili_cloud c; c.data = data; c.n = n; c.stride = stride; c.aux_offset = aux; c.mem = mem; return c; }
static bool says(const lili_cloud& c, const char* want) {
    const char* f = cloud_fault(c);
    return want ? f && std::strcmp(f, want) == 0 : f == nullptr;
}

static const char* const kNull = "null data";
static const char* const kStride = "stride must be a multiple of 4 and >= 12";
static const char* const kAux = "aux_offset outside the point";
static const char* const kMem = "bad mem";
static const char* const kMany = "too many points";

static void fault_cases() {
    g_case = "cloud_fault";
    const void* p = host_at(0);
    CHECK(says(cloud(p, 10, 16, 12, LILI_MEM_HOST), nullptr));
    // null data: refused with points, accepted without
    CHECK(says(cloud(nullptr, 1, 16, 12, LILI_MEM_HOST), kNull));
    CHECK(says(cloud(nullptr, 0, 16, 12, LILI_MEM_HOST), nullptr));
    CHECK(says(cloud(nullptr, 0, 16, -1, LILI_MEM_DEVICE), nullptr));
    // stride 8, 12, 14, 16
    CHECK(says(cloud(p, 10, 8, -1, LILI_MEM_HOST), kStride));
    CHECK(says(cloud(p, 10, 12, -1, LILI_MEM_HOST), nullptr));
    CHECK(says(cloud(p, 10, 14, -1, LILI_MEM_HOST), kStride));
    CHECK(says(cloud(p, 10, 16, -1, LILI_MEM_HOST), nullptr));
    CHECK(says(cloud(nullptr, 0, 0, -1, LILI_MEM_HOST), kStride));      // (every reader that looked at an empty cloud at all refused this)
    // aux_offset at stride - 4, at stride - 3, negative
    CHECK(says(cloud(p, 10, 20, 16, LILI_MEM_HOST), nullptr));
    CHECK(says(cloud(p, 10, 20, 17, LILI_MEM_HOST), kAux));
    CHECK(says(cloud(p, 10, 20, -1, LILI_MEM_HOST), nullptr));
    CHECK(says(cloud(p, 10, 20, -2147483647 - 1, LILI_MEM_HOST), nullptr));
    CHECK(says(cloud(p, 10, 20, 2147483647, LILI_MEM_HOST), kAux));
    // mem 0, 1, 2 — also of an empty cloud
    CHECK(says(cloud(p, 10, 16, 12, 0), nullptr));
    CHECK(says(cloud(p, 10, 16, 12, 1), nullptr));
    CHECK(says(cloud(p, 10, 16, 12, 2), kMem));
    CHECK(says(cloud(p, 10, 16, 12, -1), kMem));
    CHECK(says(cloud(nullptr, 0, 16, 12, 2), kMem));
    // n = 2^31 - 1 and 2^31
    CHECK(says(cloud(p, ((size_t)1 << 31) - 1, 16, 12, LILI_MEM_DEVICE), nullptr));
    CHECK(says(cloud(p, (size_t)1 << 31, 16, 12, LILI_MEM_DEVICE), kMany));
    // two faults: the earlier one in the order null data, stride, aux_offset, mem, count
    CHECK(says(cloud(nullptr, 1, 8, 12, 2), kNull));
    CHECK(says(cloud(nullptr, (size_t)1 << 31, 16, 12, LILI_MEM_HOST), kNull));
    CHECK(says(cloud(p, 10, 8, 8, LILI_MEM_HOST), kStride));
    CHECK(says(cloud(p, 10, 14, 0, 2), kStride));
    CHECK(says(cloud(p, 10, 16, 13, 2), kAux));
    CHECK(says(cloud(p, (size_t)1 << 31, 16, 13, LILI_MEM_HOST), kAux));
    CHECK(says(cloud(p, (size_t)1 << 31, 16, 12, 2), kMem));
}

static bool is(const CloudSource& s, CloudSource::Kind kind, const void* pinned, size_t offset) { return s.kind == kind && s.pinned == pinned && s.offset == offset; }

static void plan_cases() {
    const void *a = host_at(1), *b = host_at(2), *c = host_at(3), *d = host_at(4);
    CloudSource out[5];
    {
        g_case = "one device cloud";
        PinTable pin;
        const lili_cloud cl = cloud(a, 100, 16, 12, LILI_MEM_DEVICE);
        CHECK(plan_sources(&cl, 1, kReadPinnedInPlace, pin, out) == 0);
        CHECK(is(out[0], CloudSource::kInPlace, nullptr, 0) && pin.calls == 0);
    }
    {
        g_case = "one pinned cloud";
        PinTable pin;
        pin.locked[a] = true;
        const lili_cloud cl = cloud(a, 100, 16, 12, LILI_MEM_HOST);
        CHECK(plan_sources(&cl, 1, kReadPinnedInPlace, pin, out) == 0);
        CHECK(is(out[0], CloudSource::kPinned, dev_of(a), 0) && pin.calls == 1);
    }
    {
        g_case = "one pageable cloud";
        PinTable pin;
        const lili_cloud cl = cloud(a, 100, 20, 16, LILI_MEM_HOST);
        CHECK(plan_sources(&cl, 1, kReadPinnedInPlace, pin, out) == 2048);      // 2000 bytes
        CHECK(is(out[0], CloudSource::kStaged, nullptr, 0) && pin.calls == 1);
    }
    {
        g_case = "kStageHostAlways on a pinned cloud";
        PinTable pin;
        pin.locked[a] = true;
        const lili_cloud cl = cloud(a, 16, 16, 12, LILI_MEM_HOST);
        CHECK(plan_sources(&cl, 1, kStageHostAlways, pin, out) == 256);
        CHECK(is(out[0], CloudSource::kStaged, nullptr, 0) && pin.calls == 0);
        const lili_cloud dv = cloud(a, 16, 16, 12, LILI_MEM_DEVICE);
        CHECK(plan_sources(&dv, 1, kStageHostAlways, pin, out) == 0);
        CHECK(is(out[0], CloudSource::kInPlace, nullptr, 0) && pin.calls == 0);
    }
    {
        g_case = "three pageable clouds of 100, 0 and 1400 bytes";
        PinTable pin;
        const lili_cloud cl[3] = {cloud(a, 5, 20, 16, LILI_MEM_HOST), cloud(b, 0, 20, 16, LILI_MEM_HOST), cloud(c, 70, 20, 16, LILI_MEM_HOST)};
        CHECK(plan_sources(cl, 3, kReadPinnedInPlace, pin, out) == 256 + 1536);
        CHECK(is(out[0], CloudSource::kStaged, nullptr, 0));
        CHECK(is(out[1], CloudSource::kInPlace, nullptr, 0));
        CHECK(is(out[2], CloudSource::kStaged, nullptr, 256));
        CHECK(pin.calls == 2 && pin.asked.count(b) == 0);
    }
    {
        g_case = "device, pinned, pageable and empty clouds mixed";
        PinTable pin;
        pin.locked[b] = true; pin.locked[d] = true;
        const lili_cloud cl[5] = {cloud(a, 7, 16, 12, LILI_MEM_DEVICE), cloud(b, 300, 12, -1, LILI_MEM_HOST), cloud(c, 257, 20, 16, LILI_MEM_HOST),
                                  cloud(d, 0, 16, 12, LILI_MEM_HOST), cloud(a, 1, 16, 12, LILI_MEM_HOST)};
        CHECK(plan_sources(cl, 5, kReadPinnedInPlace, pin, out) == 5376 + 256);      // 257 * 20 = 5140 -> 5376; 16 -> 256
        CHECK(is(out[0], CloudSource::kInPlace, nullptr, 0));
        CHECK(is(out[1], CloudSource::kPinned, dev_of(b), 0));
        CHECK(is(out[2], CloudSource::kStaged, nullptr, 0));
        CHECK(is(out[3], CloudSource::kInPlace, nullptr, 0));      // empty: not asked, though its address is page-locked
        CHECK(is(out[4], CloudSource::kStaged, nullptr, 5376));
        CHECK(pin.calls == 3 && pin.asked.count(d) == 0);
        g_case = "no clouds";
        CHECK(plan_sources(cl, 0, kReadPinnedInPlace, pin, out) == 0 && pin.calls == 3);
    }
}

// the readers' code before there was a plan, restated: a sizing pass, then a placing pass that repeats the rounding (kStageHostAlways: lili_map_set's "stage if host")
struct Placed { int kind; const void* pinned; size_t offset; };
static size_t two_pass(const std::vector<lili_cloud>& cl, SourcePolicy policy, const std::map<const void*, bool>& locked, std::vector<Placed>& out) {
    auto pinned = [&](const void* p) -> void* { auto it = locked.find(p); return it != locked.end() && it->second ? dev_of(p) : nullptr; };
    size_t bytes = 0;
    for (const lili_cloud& c : cl)
        if (c.mem == LILI_MEM_HOST && c.n && (policy == kStageHostAlways || !pinned(c.data))) bytes += (c.n * c.stride + 255) / 256 * 256;
    size_t off = 0;
    out.clear();
    for (const lili_cloud& c : cl) {
        Placed p{0, nullptr, 0};
        if (c.mem == LILI_MEM_HOST && c.n) {
            void* d = policy == kStageHostAlways ? nullptr : pinned(c.data);
            if (d) { p.kind = 1; p.pinned = d; }
            else { p.kind = 2; p.offset = off; off += (c.n * c.stride + 255) / 256 * 256; }
        }
        out.push_back(p);
    }
    if (off != bytes) { std::printf("two_pass: the passes disagree\n"); g_failed++; }
    return bytes;
}

static void sweep() {
    g_case = "sweep";
    std::mt19937 rng(20240607);
    const size_t strides[4] = {12, 16, 20, 48};
    const size_t counts[8] = {0, 0, 1, 5, 16, 64, 257, 70000};
    for (int it = 0; it < 20000; it++) {
        const int n = (int)(rng() % 9);
        const SourcePolicy policy = rng() % 4 == 0 ? kStageHostAlways : kReadPinnedInPlace;
        std::vector<lili_cloud> cl;
        PinTable pin;
        for (int i = 0; i < n; i++) {
            const void* p = host_at(10 + (size_t)i);      // distinct addresses: the per-address counts below are per cloud
            cl.push_back(cloud(p, counts[rng() % 8], strides[rng() % 4], -1, rng() % 3 == 0 ? LILI_MEM_DEVICE : LILI_MEM_HOST));
            pin.locked[p] = rng() % 2 == 0;
        }
        std::vector<CloudSource> out((size_t)n + 1);
        const size_t total = plan_sources(cl.data(), n, policy, pin, out.data());
        size_t end = 0;      // the end of the last staged range so far
        int want_calls = 0;
        for (int i = 0; i < n; i++) {
            const bool host_rows = cl[i].mem == LILI_MEM_HOST && cl[i].n > 0;
            const int want = host_rows && policy == kReadPinnedInPlace ? 1 : 0;
            want_calls += want;
            CHECK((pin.asked.count(cl[i].data) ? pin.asked[cl[i].data] : 0) == want);
            if (!host_rows) CHECK(out[i].kind == CloudSource::kInPlace);
            if (out[i].kind != CloudSource::kStaged) continue;
            CHECK(host_rows);
            CHECK(out[i].offset % 256 == 0);
            CHECK(out[i].offset == end);      // in cloud order, disjoint, no gap beyond the rounding
            end = out[i].offset + (cl[i].n * cl[i].stride + 255) / 256 * 256;
            CHECK(end >= out[i].offset + cl[i].n * cl[i].stride);
        }
        CHECK(total == end);
        CHECK(pin.calls == want_calls);
        std::vector<Placed> ref;
        CHECK(two_pass(cl, policy, pin.locked, ref) == total);
        for (int i = 0; i < n; i++) CHECK((int)out[i].kind == ref[i].kind && out[i].pinned == ref[i].pinned && out[i].offset == ref[i].offset);
    }
}

int main() {
    static_assert(CloudSource::kInPlace == 0 && CloudSource::kPinned == 1 && CloudSource::kStaged == 2, "two_pass numbers the kinds this way");
    fault_cases();
    plan_cases();
    sweep();
    if (g_failed) { std::printf("cloud_source_check: %d check(s) FAILED\n", g_failed); return 1; }
    std::printf("cloud_source_check: ok\n");
    return 0;
}
