// Keyframe archive and global map on gfx950:
//   saveKeyFramesAndFactors — L/src/BackendFusion.cpp:1494-1514 (the clouds of every keyframe are kept), correctPoses — L:2177-2311 (they take new poses),
//   detectLoopClosure — L:2423-2550 (submaps of archived keyframes), publishCompleteMap — L:2644-2685 / the PCD save L:2697-2723 (every interval-th keyframe's cloud at
//   its current pose, VoxelGrid over all of them).
// Pieces:
//   * the archive: float4 rows (x, y, z, aux) in the LiDAR frame, as pushed, in a pool of large slabs that never move (a hipMalloc / hipFree is a device-wide
//     synchronisation: none per keyframe); body pose and time on the host, the map pose (q_po q_bl, q_po t_bl + t_po) in f64 in Eigen's operation order;
//   * loop-closure submaps from the archive: device views handed to lili_loop_cloud — the same gather, the same filter, the same buffers;
//   * the global map as an ACCUMULATING voxel table: per occupied voxel the absolute 64-bit key (k, j, i) = floor(p * inverse_leaf) packed lexicographically — the
//     order pcl::VoxelGrid's box-relative index induces whatever the box is —, the running f32 sum and the count, sorted by key.  A batch of placed points is sorted
//     stably by its own box-relative voxel index (lili_voxel.hip's radix sort: the same order, 32-bit keys), and every voxel of the batch CONTINUES the left fold
//     from the table's sum (or from 0.0f): a voxel's members of a later batch all come after those of the earlier ones in concatenation order, so the sequence of f32
//     additions per voxel is the one-shot filter's for any split into batches.  New keys are merged in by prefix sum and binary search (as k_merge does for the ring);
//   * the table's way out and back in, and the crop: export / import of (key, sum, count) — an imported table serves its readers but is not extended —,
//     and the voxels inside a box at the cost of the box: one run of the sorted keys per (k, j) row, found by bisection, scanned and gathered.
// No floating-point atomics anywhere: the order of the additions is the contract.
#include "lili_launch.h"
#include "lili_device_math.h"
#include "lili_device_cloud.h"

#include <climits>
#include <memory>

namespace lili {

// a pushed cloud's rows -> float4 (x, y, z, aux; aux absent: 0), read where they lie
__global__ void k_arc_rows(const unsigned char* __restrict__ src, int n, int stride, int aux_off, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = load_row_f4(src + (size_t)i * stride, aux_off);
}

// one batch of the global map: runs of archived rows placed at their keyframes' map poses, concatenated (thread i finds its run by bisection)
struct GmSeg { const float4* src; long long first; double t[3], q[4]; };
__global__ void k_gm_gather(const GmSeg* __restrict__ segs, int n_seg, int total, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const GmSeg& s = segs[seg_of(segs, n_seg, i)];
    out[i] = transform_point(s.src[(long long)i - s.first], dq{s.q[0], s.q[1], s.q[2], s.q[3]}, d3{s.t[0], s.t[1], s.t[2]});
}

// head flags of the batch's sorted keys; the points are copied into sorted order on the way (a voxel's members become one contiguous run)
__global__ void k_gm_heads(const unsigned* __restrict__ keys, const int* __restrict__ order, const float4* __restrict__ raw, int n, unsigned sentinel, int* __restrict__ flags,
                           float4* __restrict__ spts) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    spts[r] = raw[order[r]];
    flags[r] = (keys[r] != sentinel && (r == 0 || keys[r] != keys[r - 1])) ? 1 : 0;
}

// per voxel of the batch (its head's thread): where its members start, its absolute key and its place in the table — pos = lower_bound(table keys, key), is_new = the
// table does not hold the key.  head_pos[number of voxels] = where the voxels end (the non-finite rows sort behind them).  res[0] is raised by either sentinel of
// abs_voxel_key (a head is a finite point, so only "beyond +-2^20 voxels" can occur).
__global__ void k_gm_voxels(const unsigned* __restrict__ keys, const int* __restrict__ flags, const int* __restrict__ slot /*[n+1]*/, const float4* __restrict__ spts, int n,
                            unsigned sentinel, float inv_leaf, const unsigned long long* __restrict__ tkey, int n_tab, int* __restrict__ head_pos,
                            unsigned long long* __restrict__ bkey, int* __restrict__ pos, int* __restrict__ is_new, int* __restrict__ res) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const bool live = keys[r] != sentinel;
    if (live && (r == n - 1 || keys[r + 1] == sentinel)) head_pos[slot[n]] = r + 1;
    if (!flags[r]) return;
    const int v = slot[r];
    const unsigned long long key = abs_voxel_key(spts[r], inv_leaf);
    if (key >= ~0ull - 1ull) res[0] = 1;
    int lo = 0, hi = n_tab;
    while (lo < hi) { const int mid = (int)(((long long)lo + hi) >> 1); if (tkey[mid] < key) lo = mid + 1; else hi = mid; }
    head_pos[v] = r; bkey[v] = key; pos[v] = lo;
    is_new[v] = (lo < n_tab && tkey[lo] == key) ? 0 : 1;
}

// The fold, ONE THREAD PER VOXEL of the batch: the running sum starts at the table's (a voxel the table holds) or at 0.0f and takes the batch's members in order — the
// member count is known from the head positions before the first load, so the loads of a trip of eight leave together and only the additions are serial.  A voxel of
// more than kGmShort members in this batch (next to a stationary sensor: thousands) is left to k_gm_fold_long through `long_list` (its order does not matter: every
// entry is a voxel of its own).  bcnt = the voxel's count after the fold.
constexpr int kGmShort = 48;
__global__ void k_gm_fold(int n_vox, const int* __restrict__ head_pos, const float4* __restrict__ spts, const int* __restrict__ pos, const int* __restrict__ is_new,
                          const float4* __restrict__ tsum, const int* __restrict__ tcnt, float4* __restrict__ bsum, int* __restrict__ bcnt, int* __restrict__ long_list,
                          int* __restrict__ res) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vox) return;
    const int i = head_pos[v], end = head_pos[v + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f, sa = 0.f;
    int c0 = 0;
    if (!is_new[v]) { const float4 s = tsum[pos[v]]; sx = s.x; sy = s.y; sz = s.z; sa = s.w; c0 = tcnt[pos[v]]; }
    bcnt[v] = c0 + (end - i);
    if (end - i > kGmShort) {
        long_list[atomicAdd(&res[1], 1)] = v;
        bsum[v] = make_float4(sx, sy, sz, sa);
        return;
    }
    for (int m = i; m < end; m += 8) {
        float4 pp[8];
#pragma unroll
        for (int u = 0; u < 8; u++) pp[u] = spts[m + u < end ? m + u : end - 1];
#pragma unroll
        for (int u = 0; u < 8; u++) if (m + u < end) { sx += pp[u].x; sy += pp[u].y; sz += pp[u].z; sa += pp[u].w; }
    }
    bsum[v] = make_float4(sx, sy, sz, sa);
}
// the crowded voxels, one WAVE each (fold_staged, kGmStage members at a time), continued from what k_gm_fold left in bsum
constexpr int kGmStage = 512;
__global__ __launch_bounds__(256) void k_gm_fold_long(const int* __restrict__ long_list, const int* __restrict__ res, const int* __restrict__ head_pos,
                                                      const float4* __restrict__ spts, float4* __restrict__ bsum) {
    __shared__ float4 stage[4][kGmStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_long = res[1];
    for (int j = blockIdx.x * 4 + wave; j < n_long; j += gridDim.x * 4) {      // (wave-uniform)
        const int v = long_list[j];
        const int m = head_pos[v], end = head_pos[v + 1];
        const int comp = lane & 3;
        const float4 s0 = bsum[v];
        float acc = comp == 0 ? s0.x : comp == 1 ? s0.y : comp == 2 ? s0.z : s0.w;
        acc = fold_staged<kGmStage>(spts, m, end, stage[wave], lane, acc);
        const float ax = __shfl(acc, 0), ay = __shfl(acc, 1), az = __shfl(acc, 2), aw = __shfl(acc, 3);
        if (lane == 0) bsum[v] = make_float4(ax, ay, az, aw);
    }
}

// The merge, one streaming pass: threads [0, n_tab) move the table's entries — entry i goes to i + (new voxels of the batch with a smaller key), and takes the batch's sum
// and count if the batch holds its key —, threads [n_tab, n_tab + n_vox) place the batch's NEW voxels at (table keys below theirs) + (new voxels before them).
__global__ void k_gm_merge(const unsigned long long* __restrict__ tkey, const float4* __restrict__ tsum, const int* __restrict__ tcnt, long long n_tab,
                           const unsigned long long* __restrict__ bkey, const float4* __restrict__ bsum, const int* __restrict__ bcnt, const int* __restrict__ pos,
                           const int* __restrict__ is_new, const int* __restrict__ new_rank /*exclusive scan of is_new, [n_vox+1]*/, int n_vox,
                           unsigned long long* __restrict__ okey, float4* __restrict__ osum, int* __restrict__ ocnt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tab) {
        const unsigned long long k = tkey[i];
        int lo = 0, hi = n_vox;                       // lower_bound(bkey, k)
        while (lo < hi) { const int mid = (int)(((long long)lo + hi) >> 1); if (bkey[mid] < k) lo = mid + 1; else hi = mid; }
        const long long dst = i + new_rank[lo];
        const bool hit = lo < n_vox && bkey[lo] == k;
        okey[dst] = k; osum[dst] = hit ? bsum[lo] : tsum[i]; ocnt[dst] = hit ? bcnt[lo] : tcnt[i];
    } else if (i < n_tab + n_vox) {
        const int v = (int)(i - n_tab);
        if (!is_new[v]) return;
        const long long dst = (long long)pos[v] + new_rank[v];
        okey[dst] = bkey[v]; osum[dst] = bsum[v]; ocnt[dst] = bcnt[v];
    }
}

// CentroidPoint::get: sum / (float)count
__global__ void k_gm_centroid(const float4* __restrict__ tsum, const int* __restrict__ tcnt, long long n, float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = tsum[i];
    const float fn = (float)tcnt[i];
    out[i] = make_float4(s.x / fn, s.y / fn, s.z / fn, s.w / fn);
}

// The crop of the table by a box of voxel indices.  The key is k << 42 | j << 21 | i and the table is sorted, so the voxels of one (k, j) pair with i in
// [i0, i1] are ONE contiguous run of the table: thread r of k_gm_crop_runs takes row (k0 + r / nj, j0 + r % nj) and finds its run by two bisections over the keys —
// begin = lower_bound(key(k, j, i0)), len = upper_bound(key(k, j, i1)) - begin.  Integer work only.
struct CropBox { int i0, i1, j0, nj, k0; };
__global__ void k_gm_crop_runs(const unsigned long long* __restrict__ tkey, int n_tab, CropBox b, int n_rows, int* __restrict__ begin, int* __restrict__ len) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const unsigned long long kj = ((unsigned long long)(b.k0 + r / b.nj) << 42) | ((unsigned long long)(b.j0 + r % b.nj) << 21);
    const unsigned long long first = kj | (unsigned long long)b.i0, last = kj | (unsigned long long)b.i1;
    int lo = 0, hi = n_tab;
    while (lo < hi) { const int mid = (int)(((long long)lo + hi) >> 1); if (tkey[mid] < first) lo = mid + 1; else hi = mid; }
    const int at = lo;
    hi = n_tab;
    while (lo < hi) { const int mid = (int)(((long long)lo + hi) >> 1); if (tkey[mid] <= last) lo = mid + 1; else hi = mid; }
    begin[r] = at; len[r] = lo - at;
}
// The gather, ONE WAVE PER ROW: the wave of row r copies the run [begin[r], begin[r] + len) to the outputs [first[r], first[r] + len), first = the exclusive scan of the
// lengths — lane t reads the 16-byte row begin + t and writes output first + t, so both sides are runs of neighbouring rows; outputs at or beyond `cap` (the caller's
// capacity) are not written.  No bisection per output: measured against one thread per output finding its run with seg_of, this form was 10 % faster on both §7n tables.
__global__ __launch_bounds__(256) void k_gm_crop_gather(const int* __restrict__ first, const int* __restrict__ begin, int n_rows, long long cap, const float4* __restrict__ cen,
                                                        const int* __restrict__ tcnt, float4* __restrict__ out, int* __restrict__ out_cnt) {
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < n_rows; r += gridDim.x * 4) {      // (wave-uniform)
        const int f = first[r], len = first[r + 1] - f, b = begin[r];
        for (int t = lane; t < len && (long long)f + t < cap; t += 64) { out[f + t] = cen[b + t]; out_cnt[f + t] = tcnt[b + t]; }
    }
}

// an imported table is a table: keys strictly ascending, every index below 2^21 (bit 63 clear: three fields of 21 bits), every count >= 1; *bad is raised otherwise
__global__ void k_gm_validate(const unsigned long long* __restrict__ key, const int* __restrict__ cnt, long long n, int* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if ((key[i] >> 63) || cnt[i] < 1 || (i > 0 && key[i - 1] >= key[i])) *bad = 1;
}

}  // namespace lili

// `count` float4 rows of device memory into a caller's lili_feature_out (declared in lili_launch.h): out->count = count, the first min(count, capacity) rows are
// copied at out->stride (0: 16 bytes) on ctx->stream.  copy_rows_enqueue only enqueues and reports the rows the copy covers (0: nothing was enqueued);
// copy_rows_out synchronises the stream behind it, whether or not a row was copied.
int copy_rows_enqueue(lili_ctx* ctx, const void* d_rows, size_t count, lili_feature_out* out, const char* what, size_t* copied) {
    out->count = count;
    const size_t k = std::min(out->count, out->capacity);
    *copied = 0;
    if (out->data && k) {
        const size_t stride = out->stride ? out->stride : 16;
        if (stride < 16) return ctx->fail(LILI_E_ARG, std::string(what) + ": stride must be >= 16");
        const hipMemcpyKind kind = out->mem == LILI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (stride == 16) HIPCHK(hipMemcpyAsync(out->data, d_rows, k * 16, kind, ctx->stream));
        else HIPCHK(hipMemcpy2DAsync(out->data, stride, d_rows, 16, 16, k, kind, ctx->stream));
        *copied = k;
    }
    return LILI_OK;
}
int copy_rows_out(lili_ctx* ctx, const void* d_rows, size_t count, lili_feature_out* out, const char* what) {
    size_t copied = 0;
    const int rc = copy_rows_enqueue(ctx, d_rows, count, out, what, &copied);
    if (rc != LILI_OK) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

namespace {

constexpr int kKinds = 3;

struct Slab { void* p = nullptr; size_t cap = 0, used = 0; };
struct ArcCloud { float4* p = nullptr; int n = 0; bool present = false; };
struct ArcKeyframe { ArcCloud c[kKinds]; double time = 0, t_po[3] = {0, 0, 0}, q_po[4] = {1, 0, 0, 0}, t_map[3] = {0, 0, 0}, q_map[4] = {1, 0, 0, 0}; };

struct Folded { int id; double t[3], q[4]; };      // a keyframe the table holds and the map pose it was folded at
struct GlobalMap {
    std::unique_ptr<ExtState> sort;                  // the batch sort's own buffers (lili_voxel.hip)
    DevBuf key[2], sum[2], cnt[2];
    int cur = 0;
    long long n_tab = 0;
    bool valid = false;                              // the table is the fold of `folded`
    int kind = -1, interval = 0;
    float leaf = 0.f;
    double t_bl[3] = {0, 0, 0}, q_bl[4] = {1, 0, 0, 0};
    std::vector<Folded> folded;
    bool box_any = false;
    float box[6] = {0, 0, 0, 0, 0, 0};               // of every finite point folded
    int64_t n_raw = 0, folded_last = 0;
    int incremental = 0, rebuilds = 0;
    DevBuf raw, spts, flags, slot, head_pos, bkey, pos, is_new, new_rank, bsum, bcnt, long_list, sums, segs, res, out;
    DevBuf crop_begin, crop_len, crop_first, crop_rows, crop_cnt;      // lili_global_map_crop: the runs, their scan, and the gathered rows and counts
    unsigned long long key_first = 0, key_last = 0;  // of the table `out` was made from (n_tab >= 1): the crop clips its k range to theirs
    std::vector<lili::GmSeg> seg_host;
    bool has_map = false;                            // `out` holds the centroids of a successful build or import (imported: has_map && !valid — the next build starts empty)
    void clear_table() { n_tab = 0; folded.clear(); box_any = false; n_raw = 0; valid = false; has_map = false; }
    size_t table_bytes() const { size_t b = out.cap; for (int k = 0; k < 2; k++) b += key[k].cap + sum[k].cap + cnt[k].cap; return b; }
    size_t work_bytes() const {
        size_t b = lili_vox_sort_bytes(sort.get());
        for (const DevBuf* d : {&raw, &spts, &flags, &slot, &head_pos, &bkey, &pos, &is_new, &new_rank, &bsum, &bcnt, &long_list, &sums, &segs, &res, &crop_begin, &crop_len, &crop_first,
                                &crop_rows, &crop_cnt}) b += d->cap;
        return b;
    }
};

struct ArchiveState : ExtState {
    std::vector<Slab> slabs;
    std::vector<ArcKeyframe> kf;
    double t_bl[3] = {0, 0, 0}, q_bl[4] = {1, 0, 0, 0};
    int64_t n_points[kKinds] = {0, 0, 0};
    size_t bytes = 0;
    std::vector<lili_cloud> view_tmp;
    std::vector<double> pose_tmp;
    GlobalMap gm;
    unsigned long long resets = 0;      // lili_archive_reset calls so far (lili_place.hip: descriptors of an earlier archive are dropped)
    void free_slabs() { for (auto& s : slabs) if (s.p) (void)hipFree(s.p); slabs.clear(); bytes = 0; }
    ~ArchiveState() override { free_slabs(); }
};

ArchiveState* archive_of(lili_ctx* ctx) { return ext_of<ArchiveState>(ctx, lili_ctx::kExtArchive); }

// keyframe_map_pose: (q_po * q_bl, q_po * t_bl + t_po) in f64, Eigen's operation order (L:2659-2660, 2489-2490; lili_om_amd/api.py keyframe_map_pose)
void map_pose(const double t_po[3], const double a[4], const double t_bl[3], const double b[4], double t[3], double q[4]) {
    q[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    q[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    q[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    q[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
    const double u[3] = {a[1], a[2], a[3]};
    double uv[3] = {u[1] * t_bl[2] - u[2] * t_bl[1], u[2] * t_bl[0] - u[0] * t_bl[2], u[0] * t_bl[1] - u[1] * t_bl[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c[3] = {u[1] * uv[2] - u[2] * uv[1], u[2] * uv[0] - u[0] * uv[2], u[0] * uv[1] - u[1] * uv[0]};
    for (int k = 0; k < 3; k++) t[k] = ((t_bl[k] + uv[k] * a[0]) + c[k]) + t_po[k];
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

// room for `need` bytes in one piece: the last slab, or a new one (the keyframe's three clouds share one piece, so a push opens at most one slab).  The archive is
// changed only by commit_room, once nothing of the push can fail any more.
struct Room { int slab = -1; size_t off = 0; void* fresh = nullptr; size_t fresh_cap = 0; };
int find_room(lili_ctx* ctx, ArchiveState* A, size_t need, Room& r) {
    r = Room{};
    if (need == 0) return LILI_OK;
    if (!A->slabs.empty() && A->slabs.back().used + need <= A->slabs.back().cap) { r.slab = (int)A->slabs.size() - 1; r.off = A->slabs.back().used; return LILI_OK; }
    const size_t cap = std::max(need, (size_t)ctx->archive_slab_mb << 20);
    if (ctx->archive_max_mb > 0 && A->bytes + cap > ((size_t)ctx->archive_max_mb << 20))
        return ctx->fail(LILI_E_NOMEM, "archive_push: the slab pool would exceed archive_max_mb (nothing is evicted; the archive is unchanged)");
    if (hipMalloc(&r.fresh, cap + 256) != hipSuccess) { (void)hipGetLastError(); r.fresh = nullptr; return ctx->fail(LILI_E_NOMEM, "archive_push: out of device memory (the archive is unchanged)"); }
    r.fresh_cap = cap;
    return LILI_OK;
}
unsigned char* room_ptr(ArchiveState* A, const Room& r) { return r.fresh ? static_cast<unsigned char*>(r.fresh) : static_cast<unsigned char*>(A->slabs[r.slab].p) + r.off; }
void commit_room(ArchiveState* A, const Room& r, size_t need) {
    if (need == 0) return;
    if (r.fresh) { Slab s; s.p = r.fresh; s.cap = r.fresh_cap; s.used = need; A->slabs.push_back(s); A->bytes += r.fresh_cap; }
    else A->slabs[r.slab].used += need;
}

// the rows of a described cloud into `dst` (float4 rows), enqueued on the context's stream
int ingest_rows(lili_ctx* ctx, const lili_cloud* c, float4* dst) {
    if (c->n == 0) return LILI_OK;
    const unsigned char* src = nullptr;
    TRY(lili_cloud_sources(ctx, ctx->staging, c, 1, kReadPinnedInPlace, &src));
    hipLaunchKernelGGL(lili::k_arc_rows, dim3(nblocks((int64_t)c->n, 256)), dim3(256), 0, ctx->stream, src, (int)c->n, (int)c->stride, c->aux_offset, dst);
    HIPCHK(hipGetLastError());
    return LILI_OK;
}

// `dev[k]` (push_slot): float4 rows already on the device instead of a described cloud
int push_keyframe(lili_ctx* ctx, const lili_cloud* const clouds[kKinds], const float4* const dev[kKinds], const int dev_n[kKinds], double time, const double t_po[3],
                  const double q_po[4], int* id) {
    ARGCHK(t_po && q_po, "archive_push: null pose");
    for (int k = 0; k < kKinds; k++) if (clouds[k]) TRY(lili_cloud_check(ctx, *clouds[k], "archive_push"));
    HIPCHK(hipSetDevice(ctx->device));
    ArchiveState* A = archive_of(ctx);
    ARGCHK(A->kf.size() < (size_t)INT_MAX, "archive_push: too many keyframes");
    size_t need = 0, off[kKinds] = {0, 0, 0};
    int n[kKinds] = {0, 0, 0};
    bool present[kKinds] = {false, false, false};
    for (int k = 0; k < kKinds; k++) {
        present[k] = clouds[k] || dev[k];
        n[k] = clouds[k] ? (int)clouds[k]->n : dev[k] ? dev_n[k] : 0;
        off[k] = need;
        need += round256((size_t)n[k] * sizeof(float4));
    }
    Room room;
    int rc = find_room(ctx, A, need, room);
    if (rc != LILI_OK) return rc;
    unsigned char* base = need ? room_ptr(A, room) : nullptr;
    bool sync = false;
    for (int k = 0; k < kKinds && rc == LILI_OK; k++) {
        if (!n[k]) continue;
        float4* dst = reinterpret_cast<float4*>(base + off[k]);
        if (clouds[k]) { rc = ingest_rows(ctx, clouds[k], dst); sync = true; }      // (a page-locked cloud is read across PCIe by the kernel: the call returns when it has been)
        else if (hipMemcpyAsync(dst, dev[k], (size_t)n[k] * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) rc = ctx->fail(LILI_E_HIP, "archive_push: device copy failed");
    }
    if (rc == LILI_OK && sync && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = ctx->fail(LILI_E_HIP, "archive_push: synchronisation failed");
    if (rc != LILI_OK) { (void)hipStreamSynchronize(ctx->stream); if (room.fresh) (void)hipFree(room.fresh); return rc; }
    commit_room(A, room, need);
    ArcKeyframe kf;
    for (int k = 0; k < kKinds; k++) {
        kf.c[k].present = present[k]; kf.c[k].n = n[k]; kf.c[k].p = n[k] ? reinterpret_cast<float4*>(base + off[k]) : nullptr;
        A->n_points[k] += n[k];
    }
    kf.time = time;
    for (int k = 0; k < 3; k++) kf.t_po[k] = t_po[k];
    for (int k = 0; k < 4; k++) kf.q_po[k] = q_po[k];
    map_pose(kf.t_po, kf.q_po, A->t_bl, A->q_bl, kf.t_map, kf.q_map);
    if (id) *id = (int)A->kf.size();
    A->kf.push_back(kf);
    return LILI_OK;
}

// a buffer of the table that is about to be WRITTEN from scratch grows by half at least (its old content is not needed: the merge fills it)
hipError_t grow(DevBuf& b, size_t bytes) { return bytes + 256 <= b.cap ? hipSuccess : b.ensure(std::max(bytes, b.cap + b.cap / 2)); }

// folds the batch described by G.seg_host (`total` >= 1 points) into the table.  Blocking.
int fold_batch(lili_ctx* ctx, GlobalMap& G, int total) {
    const int n = total, n_seg = (int)G.seg_host.size();
    HIPCHK(G.segs.ensure((size_t)n_seg * sizeof(lili::GmSeg)));
    HIPCHK(hipMemcpyAsync(G.segs.p, G.seg_host.data(), (size_t)n_seg * sizeof(lili::GmSeg), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(G.raw.ensure((size_t)n * 16));
    hipLaunchKernelGGL(lili::k_gm_gather, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, G.segs.as<lili::GmSeg>(), n_seg, n, G.raw.as<float4>());
    HIPCHK(hipGetLastError());
    int status = 0;
    float box[6];
    unsigned sentinel = 0;
    const unsigned* d_keys = nullptr;
    const int* d_order = nullptr;
    int rc = lili_voxel_sort_dev(ctx, G.sort, G.raw.as<float4>(), n, G.leaf, &status, box, &sentinel, &d_keys, &d_order);
    if (rc != LILI_OK) return rc;
    if (status == 2) return LILI_OK;      // no finite point: nothing to fold
    if (status == 3) return ctx->fail(LILI_E_ARG, kVoxelOverflowMsg);
    // PCL's guard over EVERYTHING folded so far plus this batch: the box a one-shot filter of the concatenation would find
    float nb6[6];
    for (int k = 0; k < 3; k++) { nb6[k] = G.box_any ? std::min(G.box[k], box[k]) : box[k]; nb6[3 + k] = G.box_any ? std::max(G.box[3 + k], box[3 + k]) : box[3 + k]; }
    {
        const float inv_leaf = 1.0f / G.leaf;
        double tot = 1.0;
        for (int k = 0; k < 3; k++) { const int mn = (int)std::floor(nb6[k] * inv_leaf); tot *= (double)((int)std::floor(nb6[3 + k] * inv_leaf) - mn + 1); }
        if (tot > 2147483647.0) return ctx->fail(LILI_E_ARG, kVoxelOverflowMsg);
    }
    const size_t w = (size_t)n + 1;
    HIPCHK(G.spts.ensure((size_t)n * 16)); HIPCHK(G.flags.ensure(w * 4)); HIPCHK(G.slot.ensure(w * 4)); HIPCHK(G.head_pos.ensure(w * 4)); HIPCHK(G.bkey.ensure(w * 8));
    HIPCHK(G.pos.ensure(w * 4)); HIPCHK(G.is_new.ensure(w * 4)); HIPCHK(G.new_rank.ensure(w * 4)); HIPCHK(G.bsum.ensure(w * 16)); HIPCHK(G.bcnt.ensure(w * 4));
    HIPCHK(G.long_list.ensure(((size_t)n / lili::kGmShort + 1) * 4)); HIPCHK(G.res.ensure(16));
    HIPCHK(hipMemsetAsync(G.res.p, 0, 16, ctx->stream));
    hipLaunchKernelGGL(lili::k_gm_heads, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, d_keys, d_order, (const float4*)G.raw.as<float4>(), n, sentinel, G.flags.as<int>(), G.spts.as<float4>());
    rc = lili_scan_exclusive3(ctx, G.flags.as<int>(), n, G.sums, G.slot.as<int>());
    if (rc != LILI_OK) return rc;
    const int n_tab = (int)G.n_tab;
    hipLaunchKernelGGL(lili::k_gm_voxels, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, d_keys, (const int*)G.flags.as<int>(), (const int*)G.slot.as<int>(), (const float4*)G.spts.as<float4>(), n,
                       sentinel, 1.0f / G.leaf, (const unsigned long long*)G.key[G.cur].as<unsigned long long>(), n_tab, G.head_pos.as<int>(), G.bkey.as<unsigned long long>(), G.pos.as<int>(),
                       G.is_new.as<int>(), G.res.as<int>());
    HIPCHK(hipGetLastError());
    int n_vox = 0, bad = 0;
    rc = lili_readback_add(ctx, &n_vox, G.slot.as<int>() + n, sizeof(int));
    if (rc == LILI_OK) rc = lili_readback_add(ctx, &bad, G.res.p, sizeof(int));
    if (rc == LILI_OK) rc = lili_readback_finish(ctx);
    if (rc != LILI_OK) return rc;
    if (bad) return ctx->fail(LILI_E_ARG, "global_map: a point lies farther than 2^20 voxels from the origin");
    if (n_vox <= 0 || n_vox > n) return ctx->fail(LILI_E_STATE, "global_map: internal: voxel count of a batch out of range");
    if ((long long)n_tab + n_vox > 2147483647ll) return ctx->fail(LILI_E_ARG, kVoxelOverflowMsg);
    rc = lili_scan_exclusive3(ctx, G.is_new.as<int>(), n_vox, G.sums, G.new_rank.as<int>());
    if (rc != LILI_OK) return rc;
    hipLaunchKernelGGL(lili::k_gm_fold, dim3(nblocks(n_vox, 256)), dim3(256), 0, ctx->stream, n_vox, (const int*)G.head_pos.as<int>(), (const float4*)G.spts.as<float4>(), (const int*)G.pos.as<int>(),
                       (const int*)G.is_new.as<int>(), (const float4*)G.sum[G.cur].as<float4>(), (const int*)G.cnt[G.cur].as<int>(), G.bsum.as<float4>(), G.bcnt.as<int>(), G.long_list.as<int>(),
                       G.res.as<int>());
    hipLaunchKernelGGL(lili::k_gm_fold_long, dim3(std::min(nblocks(n / lili::kGmShort + 1, 4), 2048)), dim3(256), 0, ctx->stream, (const int*)G.long_list.as<int>(), (const int*)G.res.as<int>(),
                       (const int*)G.head_pos.as<int>(), (const float4*)G.spts.as<float4>(), G.bsum.as<float4>());
    HIPCHK(hipGetLastError());
    const int nxt = G.cur ^ 1;
    const size_t cap = (size_t)n_tab + (size_t)n_vox;      // (upper bound: the number of new voxels comes back with the merge)
    HIPCHK(grow(G.key[nxt], cap * 8)); HIPCHK(grow(G.sum[nxt], cap * 16)); HIPCHK(grow(G.cnt[nxt], cap * 4));
    hipLaunchKernelGGL(lili::k_gm_merge, dim3(nblocks((int64_t)cap, 256)), dim3(256), 0, ctx->stream, (const unsigned long long*)G.key[G.cur].as<unsigned long long>(),
                       (const float4*)G.sum[G.cur].as<float4>(), (const int*)G.cnt[G.cur].as<int>(), (long long)n_tab, (const unsigned long long*)G.bkey.as<unsigned long long>(),
                       (const float4*)G.bsum.as<float4>(), (const int*)G.bcnt.as<int>(), (const int*)G.pos.as<int>(), (const int*)G.is_new.as<int>(), (const int*)G.new_rank.as<int>(), n_vox,
                       G.key[nxt].as<unsigned long long>(), G.sum[nxt].as<float4>(), G.cnt[nxt].as<int>());
    HIPCHK(hipGetLastError());
    int n_new = 0;
    TRY(lili_readback_now(ctx, &n_new, G.new_rank.as<int>() + n_vox, sizeof(int)));
    if (n_new < 0 || n_new > n_vox) return ctx->fail(LILI_E_STATE, "global_map: internal: new-voxel count of a batch out of range");
    G.cur = nxt;
    G.n_tab = (long long)n_tab + n_new;
    for (int k = 0; k < 6; k++) G.box[k] = nb6[k];
    G.box_any = true;
    return LILI_OK;
}

// what a built or imported table (G.cur, G.n_tab) owes its readers: the centroids in G.out, and its first and last key on the host.  Blocking.
int finish_table(lili_ctx* ctx, GlobalMap& G) {
    if (!G.n_tab) { HIPCHK(hipStreamSynchronize(ctx->stream)); return LILI_OK; }
    HIPCHK(grow(G.out, (size_t)G.n_tab * 16));
    hipLaunchKernelGGL(lili::k_gm_centroid, dim3(nblocks(G.n_tab, 256)), dim3(256), 0, ctx->stream, (const float4*)G.sum[G.cur].as<float4>(), (const int*)G.cnt[G.cur].as<int>(), G.n_tab,
                       G.out.as<float4>());
    HIPCHK(hipGetLastError());
    const unsigned long long* d_key = G.key[G.cur].as<unsigned long long>();
    TRY(lili_readback_add(ctx, &G.key_first, d_key, 8));
    TRY(lili_readback_add(ctx, &G.key_last, d_key + (G.n_tab - 1), 8));
    return lili_readback_finish(ctx);
}

// a face of the crop's box as a voxel index: floorf(x * inv_leaf) in f32, offset by 2^20 and clipped to [0, 2^21 - 1] (abs_voxel_key's index; +-inf clips)
int crop_index(float x, float inv_leaf) {
    const float f = std::floor(x * inv_leaf);
    return f < -1048576.f ? 0 : f >= 1048576.f ? (1 << 21) - 1 : (int)f + (1 << 20);
}

}  // namespace

int lili_archive_size(lili_ctx* ctx) { return (int)archive_of(ctx)->kf.size(); }
unsigned long long lili_archive_resets(lili_ctx* ctx) { return archive_of(ctx)->resets; }
lili_archive_rows lili_archive_rows_of(lili_ctx* ctx, int id, int kind) {
    const ArcKeyframe& kf = archive_of(ctx)->kf[id];
    lili_archive_rows r;
    r.p = kf.c[kind].p; r.n = kf.c[kind].n; r.time = kf.time;
    return r;
}
void lili_archive_map_pose_of(lili_ctx* ctx, int id, double pose[7]) {
    const ArcKeyframe& kf = archive_of(ctx)->kf[id];
    for (int k = 0; k < 3; k++) pose[k] = kf.t_map[k];
    for (int k = 0; k < 4; k++) pose[3 + k] = kf.q_map[k];
}

extern "C" {

int lili_archive_reset(lili_ctx* ctx) {
    if (!ctx) return LILI_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ArchiveState* A = archive_of(ctx);
    A->free_slabs();
    A->kf.clear();
    for (auto& n : A->n_points) n = 0;
    A->gm.clear_table();      // (the extrinsic, the options and the statistics stay)
    A->resets++;
    return LILI_OK;
}

int lili_archive_set_extrinsic(lili_ctx* ctx, const double t_bl[3], const double q_bl[4]) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(t_bl && q_bl, "archive_set_extrinsic: null argument");
    ArchiveState* A = archive_of(ctx);
    for (int k = 0; k < 3; k++) A->t_bl[k] = t_bl[k];
    for (int k = 0; k < 4; k++) A->q_bl[k] = q_bl[k];
    for (auto& kf : A->kf) map_pose(kf.t_po, kf.q_po, A->t_bl, A->q_bl, kf.t_map, kf.q_map);
    return LILI_OK;
}

int lili_archive_push(lili_ctx* ctx, const lili_cloud* edge, const lili_cloud* surf, const lili_cloud* full, double time, const double t_po[3], const double q_po[4], int* id) {
    if (!ctx) return LILI_E_ARG;
    const lili_cloud* clouds[kKinds] = {edge, surf, full};
    const float4* dev[kKinds] = {nullptr, nullptr, nullptr};
    const int dev_n[kKinds] = {0, 0, 0};
    return push_keyframe(ctx, clouds, dev, dev_n, time, t_po, q_po, id);
}

int lili_archive_push_slot(lili_ctx* ctx, int slot, const lili_cloud* full, double time, const double t_po[3], const double q_po[4], int* id) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(slot >= 0 && slot < LILI_MAX_SLOTS, "archive_push_slot: bad slot");
    const KindSlot& e = ctx->slots[slot].k[LILI_KIND_EDGE];
    const KindSlot& s = ctx->slots[slot].k[LILI_KIND_SURF];
    static const float4 kNone{};      // a kind with queries but none of them: present, empty
    const lili_cloud* clouds[kKinds] = {nullptr, nullptr, full};
    const float4* dev[kKinds] = {e.has_queries ? (e.n_q ? e.q.as<float4>() : &kNone) : nullptr, s.has_queries ? (s.n_q ? s.q.as<float4>() : &kNone) : nullptr, nullptr};
    const int dev_n[kKinds] = {e.has_queries ? (int)e.n_q : 0, s.has_queries ? (int)s.n_q : 0, 0};
    return push_keyframe(ctx, clouds, dev, dev_n, time, t_po, q_po, id);
}

int lili_archive_set_poses(lili_ctx* ctx, int first, int n, const double* t_po, const double* q_po) {
    if (!ctx) return LILI_E_ARG;
    ArchiveState* A = archive_of(ctx);
    ARGCHK(t_po && q_po, "archive_set_poses: null pose");
    ARGCHK(first >= 0 && n >= 0 && (long long)first + n <= (long long)A->kf.size(), "archive_set_poses: first + n beyond the archive");
    for (int i = 0; i < n; i++) {
        ArcKeyframe& kf = A->kf[(size_t)first + i];
        for (int k = 0; k < 3; k++) kf.t_po[k] = t_po[3 * i + k];
        for (int k = 0; k < 4; k++) kf.q_po[k] = q_po[4 * i + k];
        map_pose(kf.t_po, kf.q_po, A->t_bl, A->q_bl, kf.t_map, kf.q_map);
    }
    return LILI_OK;
}

int lili_archive_info(lili_ctx* ctx, int* n_keyframes, int64_t n_points[3], int64_t* bytes_used) {
    if (!ctx) return LILI_E_ARG;
    ArchiveState* A = archive_of(ctx);
    if (n_keyframes) *n_keyframes = (int)A->kf.size();
    if (n_points) for (int k = 0; k < kKinds; k++) n_points[k] = A->n_points[k];
    if (bytes_used) *bytes_used = (int64_t)A->bytes;
    return LILI_OK;
}

int lili_archive_pose(lili_ctx* ctx, int id, double t_po[3], double q_po[4], double* time) {
    if (!ctx) return LILI_E_ARG;
    ArchiveState* A = archive_of(ctx);
    ARGCHK(id >= 0 && (size_t)id < A->kf.size(), "archive_pose: id out of range");
    const ArcKeyframe& kf = A->kf[id];
    if (t_po) for (int k = 0; k < 3; k++) t_po[k] = kf.t_po[k];
    if (q_po) for (int k = 0; k < 4; k++) q_po[k] = kf.q_po[k];
    if (time) *time = kf.time;
    return LILI_OK;
}

int lili_archive_get(lili_ctx* ctx, int id, int kind, lili_feature_out* out) {
    if (!ctx) return LILI_E_ARG;
    ArchiveState* A = archive_of(ctx);
    ARGCHK(out, "archive_get: null out");
    ARGCHK(id >= 0 && (size_t)id < A->kf.size(), "archive_get: id out of range");
    ARGCHK(kind >= 0 && kind < kKinds, "archive_get: unknown kind");
    HIPCHK(hipSetDevice(ctx->device));
    const ArcCloud& c = A->kf[id].c[kind];
    return copy_rows_out(ctx, c.p, (size_t)c.n, out, "archive_get");
}

int lili_archive_view(lili_ctx* ctx, int id, int kind, lili_cloud* view) {
    if (!ctx) return LILI_E_ARG;
    ArchiveState* A = archive_of(ctx);
    ARGCHK(view, "archive_view: null view");
    ARGCHK(id >= 0 && (size_t)id < A->kf.size(), "archive_view: id out of range");
    ARGCHK(kind >= 0 && kind < kKinds, "archive_view: unknown kind");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // (a push_slot copy may still be on the stream)
    const ArcCloud& c = A->kf[id].c[kind];
    view->data = c.p; view->n = (size_t)c.n; view->stride = 16; view->aux_offset = 12; view->mem = LILI_MEM_DEVICE;
    return LILI_OK;
}

int lili_loop_cloud_archive(lili_ctx* ctx, int which, const int* ids, int n_ids, float leaf, int64_t* n_raw, int64_t* n_ds) {
    if (!ctx) return LILI_E_ARG;
    ArchiveState* A = archive_of(ctx);
    ARGCHK(ids && n_ids >= 1, "loop_cloud_archive: bad argument");
    for (int i = 0; i < n_ids; i++) ARGCHK(ids[i] >= 0 && (size_t)ids[i] < A->kf.size(), "loop_cloud_archive: id out of range");
    A->view_tmp.clear(); A->pose_tmp.clear();
    std::vector<double> q;
    for (int i = 0; i < n_ids; i++) {
        const ArcKeyframe& kf = A->kf[ids[i]];
        for (int kind : {LILI_ARCHIVE_EDGE, LILI_ARCHIVE_SURF}) {
            lili_cloud c{};
            c.data = kf.c[kind].p; c.n = (size_t)kf.c[kind].n; c.stride = 16; c.aux_offset = 12; c.mem = LILI_MEM_DEVICE;
            A->view_tmp.push_back(c);
            for (int k = 0; k < 3; k++) A->pose_tmp.push_back(kf.t_map[k]);
            for (int k = 0; k < 4; k++) q.push_back(kf.q_map[k]);
        }
    }
    return lili_loop_cloud(ctx, which, A->view_tmp.data(), (int)A->view_tmp.size(), A->pose_tmp.data(), q.data(), leaf, n_raw, n_ds);
}

int lili_loop_detect(const float* positions, const double* times, int n, const float select_pose[3], double t_now, int variant, double radius, double local_thres,
                     double global_thres, double time_last_loop, int slide_window_width, int* latest, int* his) {
    if (n < 0 || (n > 0 && (!positions || !times)) || !select_pose || !latest || !his || (variant != 0 && variant != 1)) return LILI_E_ARG;
    if (n == 0) return 0;
    const float r2 = (float)(radius * radius);
    std::vector<std::pair<float, int>> in;      // kd_tree_his_key_poses->radiusSearch in f32: d2 < radius^2, ascending d2 (ties: smaller index)
    for (int i = 0; i < n; i++) {
        const float dx = positions[3 * i] - select_pose[0], dy = positions[3 * i + 1] - select_pose[1], dz = positions[3 * i + 2] - select_pose[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < r2) in.emplace_back(d2, i);
    }
    std::stable_sort(in.begin(), in.end(), [](const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first < b.first; });
    int h = -1;
    for (const auto& c : in)
        if (std::fabs(times[c.second] - t_now) > global_thres) { h = c.second; break; }
    if (variant == 0) {
        if (h == -1) {
            double max_time = 0.0;
            int max_id = -1;
            for (const auto& c : in) {
                const double dt = std::fabs(times[c.second] - t_now);
                if (local_thres < dt && dt < global_thres && dt > max_time) { max_time = dt; max_id = c.second; }
            }
            if (max_id == -1) return 0;
            h = max_id;
        }
    } else if (h == -1 || std::fabs(time_last_loop - t_now) < 0.2) return 0;
    *latest = n - slide_window_width;
    *his = h;
    return 1;
}

int lili_global_map(lili_ctx* ctx, int kind, int interval, float leaf, int64_t* n_raw, int64_t* n_map) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(kind >= 0 && kind < kKinds, "global_map: unknown kind");
    ARGCHK(interval >= 1, "global_map: interval must be >= 1");
    ARGCHK(leaf > 0 && std::isfinite(leaf), "global_map: leaf must be positive");
    HIPCHK(hipSetDevice(ctx->device));
    ArchiveState* A = archive_of(ctx);
    GlobalMap& G = A->gm;
    std::vector<int> sel;
    for (size_t i = 0; i < A->kf.size(); i += (size_t)interval) sel.push_back((int)i);
    // incremental: the table rests on the same settings, holds a prefix of the selection, and every keyframe it holds still has the map pose it was folded at, bit for bit
    bool inc = G.valid && G.kind == kind && G.interval == interval && std::memcmp(&G.leaf, &leaf, sizeof(float)) == 0 && std::memcmp(G.t_bl, A->t_bl, sizeof(G.t_bl)) == 0 &&
               std::memcmp(G.q_bl, A->q_bl, sizeof(G.q_bl)) == 0 && G.folded.size() <= sel.size();
    for (size_t i = 0; inc && i < G.folded.size(); i++) {
        const ArcKeyframe& kf = A->kf[sel[i]];
        inc = G.folded[i].id == sel[i] && std::memcmp(G.folded[i].t, kf.t_map, sizeof(kf.t_map)) == 0 && std::memcmp(G.folded[i].q, kf.q_map, sizeof(kf.q_map)) == 0;
    }
    if (inc) G.incremental++;
    else {
        G.clear_table(); G.rebuilds++;
        G.kind = kind; G.interval = interval; G.leaf = leaf;
        std::memcpy(G.t_bl, A->t_bl, sizeof(G.t_bl)); std::memcpy(G.q_bl, A->q_bl, sizeof(G.q_bl));
    }
    G.valid = false; G.has_map = false;      // until the call is through: a failure leaves no half-built table behind
    G.folded_last = 0;
    const long long batch = ctx->global_map_batch_points;
    const size_t first_new = G.folded.size();
    // batches: runs of rows in keyframe order, cut wherever `batch` points are full (a keyframe may straddle batches: its rows stay in point order)
    long long in_batch = 0;
    G.seg_host.clear();
    int rc = LILI_OK;
    for (size_t s = first_new; s < sel.size() && rc == LILI_OK; s++) {
        const ArcKeyframe& kf = A->kf[sel[s]];
        long long done = 0;
        const long long n = kf.c[kind].n;
        while (done < n && rc == LILI_OK) {
            const long long take = std::min(n - done, batch - in_batch);
            lili::GmSeg g{};
            g.src = kf.c[kind].p + done; g.first = in_batch;
            for (int k = 0; k < 3; k++) g.t[k] = kf.t_map[k];
            for (int k = 0; k < 4; k++) g.q[k] = kf.q_map[k];
            G.seg_host.push_back(g);
            in_batch += take; done += take;
            if (in_batch == batch) { rc = fold_batch(ctx, G, (int)in_batch); G.folded_last += in_batch; in_batch = 0; G.seg_host.clear(); }
        }
    }
    if (rc == LILI_OK && in_batch > 0) { rc = fold_batch(ctx, G, (int)in_batch); G.folded_last += in_batch; G.seg_host.clear(); }
    if (rc != LILI_OK) { (void)hipStreamSynchronize(ctx->stream); G.clear_table(); return rc; }
    for (size_t s = first_new; s < sel.size(); s++) {
        const ArcKeyframe& kf = A->kf[sel[s]];
        Folded f{};
        f.id = sel[s];
        std::memcpy(f.t, kf.t_map, sizeof(f.t)); std::memcpy(f.q, kf.q_map, sizeof(f.q));
        G.folded.push_back(f);
    }
    G.n_raw += G.folded_last;
    TRY(finish_table(ctx, G));
    G.valid = true; G.has_map = true;
    if (n_raw) *n_raw = G.n_raw;
    if (n_map) *n_map = G.n_tab;
    return LILI_OK;
}

int lili_global_map_get(lili_ctx* ctx, lili_feature_out* out, int32_t* counts) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(out, "global_map_get: null out");
    GlobalMap& G = archive_of(ctx)->gm;
    if (!G.has_map) return ctx->fail(LILI_E_STATE, "global_map_get: no map yet (lili_global_map first)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t k = std::min((size_t)G.n_tab, out->capacity);
    if (counts && k) HIPCHK(hipMemcpyAsync(counts, G.cnt[G.cur].p, k * 4, hipMemcpyDefault, ctx->stream));
    return copy_rows_out(ctx, G.out.p, (size_t)G.n_tab, out, "global_map_get");
}

int lili_global_map_crop(lili_ctx* ctx, const float lo[3], const float hi[3], lili_feature_out* out, int32_t* counts, int64_t* n) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(lo && hi && out, "global_map_crop: null argument");
    for (int a = 0; a < 3; a++) ARGCHK(lo[a] <= hi[a], "global_map_crop: lo > hi on an axis, or a NaN");      // (a comparison with a NaN is false)
    GlobalMap& G = archive_of(ctx)->gm;
    if (!G.has_map) return ctx->fail(LILI_E_STATE, "global_map_crop: no map yet (lili_global_map or lili_global_map_import first)");
    HIPCHK(hipSetDevice(ctx->device));
    out->count = 0;
    if (n) *n = 0;
    if (!G.n_tab) return LILI_OK;
    const float inv_leaf = 1.0f / G.leaf;
    int a0[3], a1[3];
    for (int a = 0; a < 3; a++) { a0[a] = crop_index(lo[a], inv_leaf); a1[a] = crop_index(hi[a], inv_leaf); }
    // no table row lies outside the k of its first and last key: an unbounded z face costs the table's own height
    const int k0 = std::max(a0[2], (int)(G.key_first >> 42)), k1 = std::min(a1[2], (int)(G.key_last >> 42));
    if (k0 > k1) return LILI_OK;
    const long long n_rows = (long long)(k1 - k0 + 1) * (a1[1] - a0[1] + 1);
    if (n_rows > (1ll << 24)) return ctx->fail(LILI_E_ARG, "global_map_crop: the box spans " + std::to_string(n_rows) + " (k, j) rows of voxels, more than 2^24");
    const int rows = (int)n_rows, n_tab = (int)G.n_tab;
    const size_t w = (size_t)rows + 1;
    const long long cap = out->data ? (long long)std::min(out->capacity, (size_t)n_tab) : 0;
    HIPCHK(grow(G.crop_begin, w * 4)); HIPCHK(grow(G.crop_len, w * 4)); HIPCHK(grow(G.crop_first, w * 4));
    const lili::CropBox box{a0[0], a1[0], a0[1], a1[1] - a0[1] + 1, k0};
    hipLaunchKernelGGL(lili::k_gm_crop_runs, dim3(nblocks(rows, 256)), dim3(256), 0, ctx->stream, (const unsigned long long*)G.key[G.cur].as<unsigned long long>(), n_tab, box, rows,
                       G.crop_begin.as<int>(), G.crop_len.as<int>());
    TRY(lili_scan_exclusive3(ctx, G.crop_len.as<int>(), rows, G.sums, G.crop_first.as<int>()));
    if (cap) {
        HIPCHK(grow(G.crop_rows, (size_t)cap * 16)); HIPCHK(grow(G.crop_cnt, (size_t)cap * 4));
        hipLaunchKernelGGL(lili::k_gm_crop_gather, dim3(std::min(nblocks(rows, 4), 8192)), dim3(256), 0, ctx->stream, (const int*)G.crop_first.as<int>(), (const int*)G.crop_begin.as<int>(), rows,
                           cap, (const float4*)G.out.as<float4>(), (const int*)G.cnt[G.cur].as<int>(), G.crop_rows.as<float4>(), G.crop_cnt.as<int>());
    }
    HIPCHK(hipGetLastError());
    int total = 0;
    TRY(lili_readback_now(ctx, &total, G.crop_first.as<int>() + rows, sizeof(int)));
    if (total < 0 || total > n_tab) return ctx->fail(LILI_E_STATE, "global_map_crop: internal: voxel count out of range");
    if (n) *n = total;
    const size_t k = (size_t)std::min((long long)total, cap);
    if (counts && k) HIPCHK(hipMemcpyAsync(counts, G.crop_cnt.p, k * 4, hipMemcpyDefault, ctx->stream));
    return copy_rows_out(ctx, G.crop_rows.p, (size_t)total, out, "global_map_crop");
}

int lili_global_map_export(lili_ctx* ctx, int64_t capacity, uint64_t* keys, float* sums, int32_t* counts, int64_t* n, float* leaf, int* kind) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(capacity >= 0, "global_map_export: negative capacity");
    GlobalMap& G = archive_of(ctx)->gm;
    if (!G.has_map) return ctx->fail(LILI_E_STATE, "global_map_export: no map yet (lili_global_map or lili_global_map_import first)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t k = (size_t)std::min((long long)capacity, G.n_tab);
    if (keys && k) HIPCHK(hipMemcpyAsync(keys, G.key[G.cur].p, k * 8, hipMemcpyDefault, ctx->stream));
    if (sums && k) HIPCHK(hipMemcpyAsync(sums, G.sum[G.cur].p, k * 16, hipMemcpyDefault, ctx->stream));
    if (counts && k) HIPCHK(hipMemcpyAsync(counts, G.cnt[G.cur].p, k * 4, hipMemcpyDefault, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n) *n = G.n_tab;
    if (leaf) *leaf = G.leaf;
    if (kind) *kind = G.kind;
    return LILI_OK;
}

int lili_global_map_import(lili_ctx* ctx, float leaf, int kind, int64_t n, const uint64_t* keys, const float* sums, const int32_t* counts) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(kind >= 0 && kind < kKinds, "global_map_import: unknown kind");
    ARGCHK(leaf > 0 && std::isfinite(leaf), "global_map_import: leaf must be positive");
    ARGCHK(n >= 0 && n <= 2147483647ll, "global_map_import: n out of range");
    ARGCHK(n == 0 || (keys && sums && counts), "global_map_import: null table");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    GlobalMap& G = archive_of(ctx)->gm;
    G.clear_table();      // (valid stays false: the list of folded keyframes does not travel, the next lili_global_map starts from an empty table)
    G.kind = kind; G.interval = 0; G.leaf = leaf;
    if (n) {
        const int c = G.cur;
        HIPCHK(grow(G.key[c], (size_t)n * 8)); HIPCHK(grow(G.sum[c], (size_t)n * 16)); HIPCHK(grow(G.cnt[c], (size_t)n * 4)); HIPCHK(G.res.ensure(16));
        HIPCHK(hipMemcpyAsync(G.key[c].p, keys, (size_t)n * 8, hipMemcpyDefault, ctx->stream));
        HIPCHK(hipMemcpyAsync(G.sum[c].p, sums, (size_t)n * 16, hipMemcpyDefault, ctx->stream));
        HIPCHK(hipMemcpyAsync(G.cnt[c].p, counts, (size_t)n * 4, hipMemcpyDefault, ctx->stream));
        HIPCHK(hipMemsetAsync(G.res.p, 0, 16, ctx->stream));
        hipLaunchKernelGGL(lili::k_gm_validate, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, (const unsigned long long*)G.key[c].as<unsigned long long>(), (const int*)G.cnt[c].as<int>(),
                           (long long)n, G.res.as<int>());
        HIPCHK(hipGetLastError());
        int bad = 0;
        TRY(lili_readback_now(ctx, &bad, G.res.p, sizeof(int)));
        if (bad) return ctx->fail(LILI_E_ARG, "global_map_import: not a table (keys strictly ascending, every index below 2^21, counts >= 1)");
    }
    G.n_tab = n;
    const int rc = finish_table(ctx, G);
    if (rc != LILI_OK) { (void)hipStreamSynchronize(ctx->stream); G.clear_table(); return rc; }
    G.has_map = true;
    return LILI_OK;
}

int lili_global_map_stats(lili_ctx* ctx, int32_t* incremental, int32_t* rebuilds, int64_t* points_folded_last) {
    if (!ctx) return LILI_E_ARG;
    const GlobalMap& G = archive_of(ctx)->gm;
    if (incremental) *incremental = G.incremental;
    if (rebuilds) *rebuilds = G.rebuilds;
    if (points_folded_last) *points_folded_last = G.folded_last;
    return LILI_OK;
}

int lili_global_map_info(lili_ctx* ctx, int64_t* table_bytes, int64_t* work_bytes) {
    if (!ctx) return LILI_E_ARG;
    const GlobalMap& G = archive_of(ctx)->gm;
    if (table_bytes) *table_bytes = (int64_t)G.table_bytes();
    if (work_bytes) *work_bytes = (int64_t)G.work_bytes();
    return LILI_OK;
}

}  // extern "C"
