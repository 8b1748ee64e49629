// Device-side helpers of the point-cloud kernels (map index, voxel filter, keyframe ring, loop submaps, archive and global map) whose exact arithmetic or ordering
// is the contract between files: the ordered-uint form of a float, the absolute voxel key, the segment lookup of a concatenation, the read of a caller's row, and the
// staged sequential f32 fold of a crowded voxel's members.  ONE definition each: a map built through one path is bit-identical to the map built through another because both
// run the same body, not two bodies kept alike by hand.  No floating-point atomics anywhere: the order of the additions is the contract.
#pragma once
#include <hip/hip_runtime.h>

namespace lili {

// order-preserving float -> uint (bounding boxes are reduced with integer atomics) and its inverse, which the host uses on the words it reads back
__device__ __forceinline__ unsigned f2ord(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ float ord2f(unsigned u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// between two steps in which a wave reads from LDS what only ITS OWN lanes wrote: the LDS serves a wave's accesses in order; the compiler must keep them in order too
__device__ __forceinline__ void wave_lds_order() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// Absolute voxel key of a point: (k, j, i) = floor(p * inverse_leaf) packed lexicographically — the order pcl::VoxelGrid's box-relative index induces whatever the
// bounding box is.  The sorted keyframe ring and the global map's table both hold it.  Two sentinels above every voxel: ~0 = a non-finite point (sorts last, never a
// voxel: voxel_grid.hpp skips !isFinite), ~0 - 1 = beyond +-2^20 voxels from the origin (the caller raises a flag: the ring rebuilds, the global map refuses).
__device__ __forceinline__ unsigned long long abs_voxel_key(float4 p, float inv_leaf) {
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return ~0ull;
    const long long i = (long long)floorf(p.x * inv_leaf) + (1ll << 20), j = (long long)floorf(p.y * inv_leaf) + (1ll << 20), k = (long long)floorf(p.z * inv_leaf) + (1ll << 20);
    if ((i | j | k) < 0 || i >= (1ll << 21) || j >= (1ll << 21) || k >= (1ll << 21)) return ~0ull - 1ull;
    return ((unsigned long long)k << 42) | ((unsigned long long)j << 21) | (unsigned long long)i;
}

// the segment of a concatenation that holds position i: the last one whose `first` is <= i, by bisection over the (ascending) first positions
template <typename Seg, typename Index>
__device__ __forceinline__ int seg_of(const Seg* segs, int n_seg, Index i) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (segs[mid].first <= (long long)i) lo = mid; else hi = mid - 1; }
    return lo;
}

// a row of a caller's cloud (floats x, y, z at its start, the auxiliary float at byte `aux_off` or absent: < 0) as float4 (x, y, z, aux; absent: 0), read where it lies
__device__ __forceinline__ float4 load_row_f4(const unsigned char* row, int aux_off) {
    const float* p = reinterpret_cast<const float*>(row);
    return make_float4(p[0], p[1], p[2], aux_off >= 0 ? *reinterpret_cast<const float*>(row + aux_off) : 0.f);
}

// CentroidPoint's sequential f32 sums over the members [m, end) of a crowded voxel, by ONE WAVE: the wave requests kStage members at once, parks them in `stage` (its own kStage rows of LDS) and lane c of every
// four carries component c of the sum — ONE dependent addition per member instead of four, the operands read from a wave-uniform LDS address sixteen ahead of the
// additions.  `acc`: the lane's component of the sum so far; returns it with the members [m, end) added in order (lanes 0..3 hold x, y, z, w).
template <int kStage>
__device__ __forceinline__ float fold_staged(const float4* spts, int m, int end, float4* stage, int lane, float acc) {
    const float* st = reinterpret_cast<const float*>(stage) + (lane & 3);
    while (m < end) {
        const int cnt = min(end - m, kStage);
        float4 reg[kStage / 64];
#pragma unroll
        for (int r = 0; r < kStage / 64; r++) reg[r] = spts[min(m + 64 * r + lane, end - 1)];      // (no branch: every request leaves before the first answer is awaited; rows behind the end re-read its last point)
#pragma unroll
        for (int r = 0; r < kStage / 64; r++) stage[64 * r + lane] = reg[r];
        wave_lds_order();
        float p[16];
#pragma unroll
        for (int t = 0; t < 16; t++) p[t] = st[4 * t];
        for (int u = 0; u < cnt; u += 16) {
            float nx[16];
#pragma unroll
            for (int t = 0; t < 16; t++) nx[t] = st[4 * min(u + 16 + t, kStage - 1)];
#pragma unroll
            for (int t = 0; t < 16; t++) if (u + t < cnt) acc += p[t];
#pragma unroll
            for (int t = 0; t < 16; t++) p[t] = nx[t];
        }
        m += cnt;
        wave_lds_order();      // the next members overwrite the stage
    }
    return acc;
}

}  // namespace lili
