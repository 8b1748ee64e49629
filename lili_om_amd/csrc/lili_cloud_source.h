// Internal: the contract of a caller's lili_cloud, decided from the description alone (plain C++17, no HIP: tests/cloud_source_check.cpp runs it on the CPU).
// cloud_fault says what is wrong with a description; plan_sources says where a kernel reads the rows of n clouds from: a device cloud (or an empty one) where it
// lies, a page-locked host cloud through its device-side address, a pageable one from a staging buffer, at offsets of 256 bytes in cloud order.  "Page-locked" is
// asked through `pinned` on every call and never cached (lili_pinned_dev_ptr in lili_api.hip says why); lili_cloud_check / lili_cloud_sources apply both.
#pragma once
#include "../../include/lili_hip.h"

#include <cstddef>

namespace lili_detail {

// nullptr, or the first thing wrong with the description
inline const char* cloud_fault(const lili_cloud& c) {
    if (c.n != 0 && !c.data) return "null data";
    if (c.stride < 12 || c.stride % 4 != 0) return "stride must be a multiple of 4 and >= 12";
    if (c.aux_offset >= 0 && (size_t)c.aux_offset + 4 > c.stride) return "aux_offset outside the point";
    if (c.mem != LILI_MEM_HOST && c.mem != LILI_MEM_DEVICE) return "bad mem";
    if (c.n >= (size_t)1 << 31) return "too many points";
    return nullptr;
}

enum SourcePolicy { kReadPinnedInPlace,      // a page-locked host cloud is read where it lies, across PCIe
                    kStageHostAlways };      // every host cloud is staged (lili_map_set: three passes read it); `pinned` is not asked
struct CloudSource {
    enum Kind { kInPlace, kPinned, kStaged } kind = kInPlace;
    const void* pinned = nullptr;      // kPinned: the device-side address
    size_t offset = 0;                 // kStaged: byte offset into the staging buffer
};

// out[i] for the valid clouds[0 .. n); returns the staging bytes.  `pinned(data)` -> the device-side address or nullptr: at most once per non-empty host cloud.
template <class Pinned> size_t plan_sources(const lili_cloud* clouds, int n, SourcePolicy policy, Pinned&& pinned, CloudSource* out) {
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        const lili_cloud& c = clouds[i];
        out[i] = CloudSource{};
        if (c.mem != LILI_MEM_HOST || c.n == 0) continue;
        if (policy == kReadPinnedInPlace) out[i].pinned = pinned(c.data);
        if (out[i].pinned) { out[i].kind = CloudSource::kPinned; continue; }
        out[i].kind = CloudSource::kStaged; out[i].offset = total;
        total += (c.n * c.stride + 255) / 256 * 256;
    }
    return total;
}

}  // namespace lili_detail
