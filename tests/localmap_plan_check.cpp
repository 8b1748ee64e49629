// The plan of lili_localmap_commit (lili_om_amd/csrc/lili_localmap_plan.h) on the CPU: the named cases of the sorted ring's life, then a seeded random sweep.
// Built and run by tests/test_localmap_plan_cpu.py under the address and undefined-behaviour sanitizers.
#include "../lili_om_amd/csrc/lili_localmap_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using lili_detail::LocalmapPlan;
using lili_detail::SeqCount;
using lili_detail::localmap_plan;
typedef std::vector<SeqCount> Ring;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s: FAILED line %d: %s\n", g_case, __LINE__, #cond); g_failed++; } } while (0)
static const char* g_case = "";

// the properties every "merge" answer has, whatever the input
static void check_merge_properties(const Ring& members, const Ring& ring, const LocalmapPlan& P) {
    CHECK(P.keep_lo <= P.keep_hi);
    CHECK(P.first_add <= ring.size());
    long long kept = 0, dropped = 0, incoming = 0, total = 0;
    size_t n_kept = 0;
    for (const auto& m : members) {
        bool in_ring = false;      // a member stays if the ring's kept part still holds it under its number
        for (size_t i = 0; i < P.first_add; i++) in_ring = in_ring || ring[i].first == m.first;
        const bool in_range = m.first >= P.keep_lo && m.first <= P.keep_hi;
        CHECK(in_ring == in_range);
        if (in_range) { kept += m.second; n_kept++; } else dropped += m.second;
    }
    CHECK(n_kept == P.first_add);
    for (size_t i = 0; i < ring.size(); i++) { total += ring[i].second; if (i >= P.first_add) incoming += ring[i].second; }
    CHECK(P.n_drop == dropped);
    CHECK(kept + incoming == total);
    const size_t n_add = ring.size() - P.first_add;
    if (P.after_repose) CHECK(n_add >= 1 && n_add <= lili_detail::kResuffixMaxAdd);
    else CHECK(n_add <= lili_detail::kPlanMaxPending);
}

static LocalmapPlan expect_merge(const char* name, const Ring& members, const Ring& ring, bool after_repose, unsigned lo, unsigned hi, long long n_drop, size_t first_add) {
    g_case = name;
    const LocalmapPlan P = localmap_plan(members, ring);
    CHECK(P.merge);
    if (P.merge) {
        CHECK(P.after_repose == after_repose); CHECK(P.keep_lo == lo); CHECK(P.keep_hi == hi); CHECK(P.n_drop == n_drop); CHECK(P.first_add == first_add);
        check_merge_properties(members, ring, P);
    }
    return P;
}
static void expect_rebuild(const char* name, const Ring& members, const Ring& ring) {
    g_case = name;
    CHECK(!localmap_plan(members, ring).merge);
}

// members 1 .. n with 10 * seq points each
static Ring run(unsigned first, unsigned last) { Ring r; for (unsigned s = first; s <= last; s++) r.push_back({s, (int)(10 * s)}); return r; }
static Ring cat(Ring a, const Ring& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

static void named_cases() {
    expect_merge("ring still filling: nothing popped, one pushed", run(1, 3), run(1, 4), false, 1, 3, 0, 3);
    expect_merge("pop 1 / push 1", run(1, 5), run(2, 6), false, 2, 5, 10, 4);
    expect_merge("pop 2 / push 1", run(1, 5), run(3, 6), false, 3, 5, 30, 3);
    expect_merge("pop 4", run(1, 8), run(5, 9), false, 5, 8, 100, 4);
    expect_rebuild("pop 5", run(1, 8), run(6, 9));
    expect_merge("2 pending", run(1, 5), run(2, 7), false, 2, 5, 10, 4);
    expect_rebuild("3 pending", run(1, 5), run(2, 8));
    expect_merge("only pops", run(1, 5), run(3, 5), false, 3, 5, 30, 3);
    expect_merge("nothing changed", run(1, 5), run(1, 5), false, 1, 5, 0, 5);
    {   // an empty keyframe at either end of the kept run: the range is of sequence numbers, not of points
        const Ring members = {{1, 7}, {2, 0}, {3, 5}, {4, 0}}, ring = {{2, 0}, {3, 5}, {4, 0}, {5, 9}};
        expect_merge("empty keyframes at both ends of the kept run", members, ring, false, 2, 4, 7, 3);
        expect_merge("an empty keyframe pushed", members, Ring{{2, 0}, {3, 5}, {4, 0}, {5, 0}}, false, 2, 4, 7, 3);
        expect_merge("an empty keyframe popped", Ring{{1, 0}, {2, 3}}, Ring{{2, 3}, {3, 4}}, false, 2, 2, 0, 1);
    }
    expect_rebuild("first member not found: everything popped", run(1, 5), run(6, 8));
    expect_rebuild("first member not found: the ring's front was never a member", run(2, 5), run(1, 5));
    expect_rebuild("empty ring", run(1, 5), Ring{});
    expect_rebuild("no members", Ring{}, run(1, 2));
    expect_rebuild("ring not 'old members, then new keyframes': an old number behind the run", run(1, 3), Ring{{2, 20}, {1, 10}});
    expect_rebuild("ring not 'old members, then new keyframes': a member missing in the middle, nothing behind", run(1, 4), Ring{{1, 10}, {2, 20}});
    expect_rebuild("ring not 'old members, then new keyframes': a member missing in the middle", run(1, 4), Ring{{1, 10}, {2, 20}, {4, 40}});
    // repose: the suffix comes back under fresh numbers (above every member's), same points
    expect_merge("repose of the last", run(1, 5), cat(run(1, 4), Ring{{6, 50}}), true, 1, 4, 50, 4);
    expect_merge("repose of a suffix of 3", run(1, 5), cat(run(1, 2), Ring{{6, 30}, {7, 40}, {8, 50}}), true, 1, 2, 120, 2);
    expect_rebuild("repose of everything", run(1, 3), Ring{{4, 10}, {5, 20}, {6, 30}});
    expect_merge("repose then push with a pop", run(1, 5), cat(run(2, 3), Ring{{6, 40}, {7, 50}, {8, 33}}), true, 2, 3, 100, 2);
    {
        Ring suffix8, suffix9;
        for (unsigned s = 0; s < 8; s++) suffix8.push_back({20 + s, (int)(10 * (3 + s))});
        for (unsigned s = 0; s < 9; s++) suffix9.push_back({20 + s, (int)(10 * (2 + s))});
        expect_merge("repose suffix of 8", run(1, 10), cat(run(1, 2), suffix8), true, 1, 2, 10 * (3 + 4 + 5 + 6 + 7 + 8 + 9 + 10), 2);
        expect_rebuild("repose suffix of 9", run(1, 10), cat(run(1, 1), suffix9));
        expect_rebuild("repose suffix of 7 and 2 pushes", run(1, 10), cat(cat(run(1, 3), Ring(suffix8.begin() + 1, suffix8.end())), Ring{{40, 1}, {41, 1}}));
    }
    expect_rebuild("the point-count mismatch that cancels the repose route", run(1, 5), Ring{{1, 10}, {2, 21}, {3, 30}, {6, 40}, {7, 50}});      // (a kept keyframe's points differ)
    expect_rebuild("a point-count mismatch on the plain route", run(1, 3), Ring{{1, 10}, {2, 21}, {3, 30}, {4, 40}});
    expect_rebuild("numbers that do not rise: a dropped member inside the range", Ring{{5, 1}, {2, 1}, {3, 1}, {6, 1}}, Ring{{2, 1}, {3, 1}, {6, 1}, {7, 1}});
}

// rings as the library makes them: members with rising numbers; p popped, the last r of the rest renumbered (repose), a pushed — the decision is known
static void sweep() {
    g_case = "sweep";
    std::mt19937 rng(20240611u);
    auto below = [&](unsigned n) { return (unsigned)(rng() % n); };
    int merges = 0, rebuilds = 0, reposes = 0;
    for (int trial = 0; trial < 20000; trial++) {
        const size_t k = 1 + below(12);
        Ring members;
        unsigned seq = 1 + below(5);
        for (size_t i = 0; i < k; i++) { members.push_back({seq, below(4) == 0 ? 0 : (int)below(1000)}); seq += 1 + below(3); }
        const size_t p = below((unsigned)k + 1), r = below((unsigned)(k - p) + 1);
        size_t a = below(5);
        const size_t kept = k - p - r;
        if (kept + r + a > 12) a = 12 - kept - r;
        Ring ring(members.begin() + (long)p, members.begin() + (long)(k - r));
        for (size_t i = 0; i < r; i++) { ring.push_back({seq, members[k - r + i].second}); seq += 1; }
        for (size_t i = 0; i < a; i++) { ring.push_back({seq, below(4) == 0 ? 0 : (int)below(1000)}); seq += 1 + below(2); }
        const int corrupt = below(5) == 0 ? 1 + (int)below(3) : 0;      // a fifth of the rings are not what the library makes: only the properties are asserted
        if (corrupt == 1 && ring.size() >= 2) std::swap(ring[below((unsigned)ring.size())], ring[below((unsigned)ring.size())]);
        if (corrupt == 2 && !ring.empty()) ring[below((unsigned)ring.size())].second += 1;
        if (corrupt == 3 && members.size() >= 2) std::swap(members[below((unsigned)k)].first, members[below((unsigned)k)].first);
        const LocalmapPlan P = localmap_plan(members, ring);
        if (P.merge) { check_merge_properties(members, ring, P); merges++; reposes += P.after_repose ? 1 : 0; } else rebuilds++;
        if (corrupt) continue;
        bool want = kept > 0;
        if (want) want = r > 0 ? r + a <= lili_detail::kResuffixMaxAdd : (p <= lili_detail::kPlanMaxPopped && a <= lili_detail::kPlanMaxPending);
        CHECK(P.merge == want);
        if (P.merge && want) {
            long long n_drop = 0;
            for (size_t i = 0; i < k; i++) if (i < p || i >= k - r) n_drop += members[i].second;
            CHECK(P.after_repose == (r > 0)); CHECK(P.keep_lo == members[p].first); CHECK(P.keep_hi == members[k - r - 1].first); CHECK(P.first_add == kept); CHECK(P.n_drop == n_drop);
        }
        if (g_failed > 20) return;
    }
    CHECK(merges > 2000 && rebuilds > 2000 && reposes > 500);      // (the sweep visits every answer)
    std::printf("sweep: %d merges (%d after a repose), %d rebuilds\n", merges, reposes, rebuilds);
}

int main() {
    named_cases();
    sweep();
    if (g_failed) { std::printf("localmap_plan_check: %d check(s) failed\n", g_failed); return 1; }
    std::printf("localmap_plan_check: ok\n");
    return 0;
}
