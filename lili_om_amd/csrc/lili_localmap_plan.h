// Internal: what lili_localmap_commit does with the sorted ring, decided from sequence numbers and point counts alone (plain C++17, no HIP: tests/localmap_plan_check.cpp
// runs it on the CPU).  The sorted ring holds the keyframes `members` (oldest first); the ring now holds `ring`.  Ring sequence numbers rise in ring order — pushes take
// next_seq++, lili_localmap_repose renumbers its suffix upwards —, a commit drops a prefix of the members and, after a repose, a suffix as well: the entries that stay
// are those of ONE range [keep_lo, keep_hi] of sequence numbers, and the keyframes ring[first_add ..] come in.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace lili_detail {

constexpr size_t kPlanMaxPopped = 4;       // popped keyframes of one plain commit; more take the full rebuild (the length of the drop list the keep rule used to be: lifting it is a separate change)
constexpr size_t kPlanMaxPending = 2;      // pending keyframes of one plain commit, one merge step each: beyond, the rebuild is cheaper than as many merge passes
constexpr size_t kResuffixMaxAdd = 8;      // keyframes merged in at once after a repose; more (a long re-posed suffix, a loop closure) take the full rebuild

using SeqCount = std::pair<unsigned, int>;      // (sequence number, points) of one keyframe

struct LocalmapPlan {
    bool merge = false;                    // false: full rebuild, nothing below means anything
    bool after_repose = false;             // ONE merge step of all incoming keyframes (a re-posed suffix under fresh numbers, then the pending pushes); else one step per keyframe
    unsigned keep_lo = 0, keep_hi = 0;     // the members that stay
    long long n_drop = 0;                  // points of the members that go
    size_t first_add = 0;                  // ring[first_add ..] come in (may be none: only pops)
};

inline LocalmapPlan localmap_plan(const std::vector<SeqCount>& members, const std::vector<SeqCount>& ring) {
    LocalmapPlan P;
    if (members.empty() || ring.empty()) return P;
    // keyframes popped at the front (f), then the run of members the ring still holds under their numbers (m)
    size_t f = 0, m = 0;
    while (f < members.size() && members[f].first != ring.front().first) f++;
    if (f == members.size()) return P;
    while (f + m < members.size() && m < ring.size() && members[f + m].first == ring[m].first) m++;
    if (f + m < members.size()) {
        // members behind the kept ones that the ring no longer holds under their numbers: a re-posed suffix (its fresh numbers are above every member's)
        if (!(m < ring.size() && ring[m].first > members.back().first && ring.size() - m <= kResuffixMaxAdd)) return P;      // (else the ring is not "old members, then new keyframes")
        P.after_repose = true;
    } else if (f > kPlanMaxPopped || ring.size() - m > kPlanMaxPending) return P;
    P.keep_lo = members[f].first; P.keep_hi = members[f + m - 1].first; P.first_add = m;
    // the keep rule is a RANGE: it must say of every member what the run says (it does while the numbers rise in ring order)
    long long kept = 0, incoming = 0, total = 0;
    for (size_t i = 0; i < members.size(); i++) {
        const bool in_run = i >= f && i < f + m, in_range = members[i].first >= P.keep_lo && members[i].first <= P.keep_hi;
        if (in_run != in_range) return P;
        (in_run ? kept : P.n_drop) += members[i].second;
    }
    for (size_t i = 0; i < ring.size(); i++) { total += ring[i].second; if (i >= m) incoming += ring[i].second; }
    if (kept + incoming != total) return P;      // (the merge writes exactly the ring's points; anything else is not this case)
    P.merge = true;
    return P;
}

}  // namespace lili_detail
