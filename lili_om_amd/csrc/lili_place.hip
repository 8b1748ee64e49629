// Place recognition on gfx950: a polar descriptor per archived keyframe in the manner of Scan Context (Kim & Kim, IROS 2018) — n_sector x n_ring
// maximum heights, stored sector-major — and the exact search of a batch of queries against every described keyframe at every circular shift.
// Pieces:
//   * the descriptor: ring and sector of a point by comparisons against tables the host computes once (no arctangent, no square root: lili_place_layout), the cell's
//     maximum by integer atomics on the ordered-uint form of the height.  A maximum does not depend on order: the descriptor is the same bytes on every run and for
//     every split of the work.  One launch over a segment table describes any number of keyframes (k_place_cells), one more turns the words into floats;
//   * levelled submap descriptors (lili_place_set_submap): a keyframe described by the rows of a window of keyframes placed in its levelled frame — one workgroup bins
//     a tile of rows into an image in LDS and merges it once (k_place_cells_sub); a descriptor is rebuilt when its build key (members and relative placements) changes;
//   * the search: a wave holds one candidate, a lane one sector's column as a unit vector in f64; the query's unit columns lie ring-major in LDS, so that at shift s lane l
//     reads column l - s without a bank conflict.  The per-lane cosines of sixteen shifts are parked in LDS and summed per shift in a fixed order (four lanes a shift,
//     sixteen terms each, then the four parts): a pair's distance and shift depend on the two descriptors alone, never on where the candidate lies or what else is in
//     the batch.  The valid count of a shift is a rotate and a popcount of the two occupancy ballots;
//   * the k best of a query: k rounds of a block-wide minimum over (distance, id).
// No floating-point atomics anywhere.
#include "lili_launch.h"
#include "lili_device_cloud.h"
#include "lili_device_math.h"

#include <climits>

namespace lili {

constexpr int kPlMaxRing = 32, kPlMaxSector = 64, kPlMaxQuery = 64, kPlMaxK = 16;
constexpr int kPlShiftGroup = 16;                            // shifts whose per-lane cosines are parked in LDS before they are summed
constexpr int kPlRowPad = kPlMaxSector + 1;                  // a parked shift's row: 65 doubles, so that the four parts of a sum start in different banks

// what lili_place_layout computes: ring k's inner boundary squared, cos / sin of sector boundary m inside a quadrant (all f32)
struct PlaceLayout {
    float ring_r2[kPlMaxRing], sec_cos[kPlMaxSector / 4], sec_sin[kPlMaxSector / 4];
    float max_r2, lidar_height;
    int n_ring, n_sector;
};

// the cell (sector * n_ring + ring) of a point and the value it offers the cell, or -1: skipped
__device__ __forceinline__ int place_cell(const PlaceLayout& L, float x, float y, float z, float* val) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return -1;
    const float r2 = x * x + y * y;
    if (r2 > L.max_r2) return -1;
    int ring = 0;
    for (int k = 1; k < L.n_ring; k++) ring += r2 > L.ring_r2[k] ? 1 : 0;
    const int q = y >= 0.f ? (x >= 0.f ? 0 : 1) : (x < 0.f ? 2 : 3);
    const float u = q == 0 ? x : q == 1 ? y : q == 2 ? -x : -y;
    const float v = q == 0 ? y : q == 1 ? -x : q == 2 ? -y : x;
    const int per_quadrant = L.n_sector / 4;
    int j = 0;
    for (int m = 1; m < per_quadrant; m++) j += v * L.sec_cos[m] >= u * L.sec_sin[m] ? 1 : 0;
    *val = z + L.lidar_height;
    return (q * per_quadrant + j) * L.n_ring + ring;
}

// a run of rows (any stride; x, y, z at a row's start) whose points go into image `slot`; `first`: the run's position in the concatenation
struct PlSeg { const unsigned char* src; long long first; int stride, slot; };
// the same with the placement k_place_cells_sub applies first: transform_point by (q, t), or none where `ident` is set (the row is read as it is).  A type of its
// own: k_place_cells keeps PlSeg's 24-byte stride and with it its address arithmetic, instruction for instruction.
struct PlSubSeg : PlSeg { dq q; d3 t; int ident, pad_; };

// every point of the concatenation offers its height to its cell: atomicMax on the ordered-uint form (0 = no point yet: below every float's word).  The plain read in
// front of the atomic may be stale, but a cell's word only grows: a stale word costs an atomic, never a maximum.
__global__ void k_place_cells(const PlSeg* __restrict__ segs, int n_seg, long long total, PlaceLayout L, unsigned* img, int cells) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const PlSeg s = segs[seg_of(segs, n_seg, i)];
    const float* p = reinterpret_cast<const float*>(s.src + (size_t)(i - s.first) * (size_t)s.stride);
    float val;
    const int cell = place_cell(L, p[0], p[1], p[2], &val);
    if (cell < 0) return;
    const unsigned w = f2ord(val);
    unsigned* a = img + (size_t)s.slot * cells + cell;
    if (*reinterpret_cast<volatile unsigned*>(a) < w) atomicMax(a, w);
}

// Submap descriptors: a descriptor's concatenation holds the rows of a whole window of keyframes, about twenty times a keyframe's, and k_place_cells' global atomics
// slow down as the rows per image grow.  Here ONE WORKGROUP bins one TILE — at most kPlTileRows rows of ONE descriptor's concatenation — into an image
// in LDS and offers the global image only the tile's non-zero cells, once.  The tile table comes from the host with the tile's first segment in it: a thread's rows
// ascend, so it walks the segment table forward from there and never bisects.  A row is placed by transform_point (lili_device_math.h) unless its segment carries the
// identity flag; place_cell and the ordered-uint maximum are k_place_cells'.  The maximum is order-free: tiles, batches and runs cannot change a byte.
constexpr int kPlTileRows = LILI_PLACE_TILE_ROWS;
struct PlTile { long long first; int n, seg, slot, pad_; };      // rows [first, first + n) of the concatenation, the segment that holds `first`, the image

__global__ __launch_bounds__(256) void k_place_cells_sub(const PlSubSeg* __restrict__ segs, int n_seg, const PlTile* __restrict__ tiles, PlaceLayout L, unsigned* img, int cells) {
    __shared__ unsigned s_img[kPlMaxSector * kPlMaxRing];
    const int tid = threadIdx.x;
    for (int c = tid; c < cells; c += 256) s_img[c] = 0u;
    const PlTile tile = tiles[blockIdx.x];
    __syncthreads();
    int si = tile.seg;
    PlSubSeg s = segs[si];
    for (int k = tid; k < tile.n; k += 256) {
        const long long i = tile.first + k;
        if (si + 1 < n_seg && segs[si + 1].first <= i) {      // (the tile ends inside its descriptor: the walk stays among that descriptor's segments)
            do si++; while (si + 1 < n_seg && segs[si + 1].first <= i);
            s = segs[si];
        }
        const float* p = reinterpret_cast<const float*>(s.src + (size_t)(i - s.first) * (size_t)s.stride);
        float x = p[0], y = p[1], z = p[2];
        if (!s.ident) {
            const float4 r = transform_point(make_float4(x, y, z, 0.f), s.q, s.t);
            x = r.x; y = r.y; z = r.z;
        }
        float val;
        const int cell = place_cell(L, x, y, z, &val);
        if (cell < 0) continue;
        const unsigned w = f2ord(val);
        if (*reinterpret_cast<volatile unsigned*>(&s_img[cell]) < w) atomicMax(&s_img[cell], w);
    }
    __syncthreads();
    unsigned* out = img + (size_t)tile.slot * cells;
    for (int c = tid; c < cells; c += 256) {
        const unsigned w = s_img[c];
        if (w && *reinterpret_cast<volatile unsigned*>(out + c) < w) atomicMax(out + c, w);
    }
}

#ifdef LILI_PLACE_PROBE_GLOBAL
// tools/place_time.py's probe build only (never the shipped library): the same segment table in k_place_cells' form — a thread a row, the segment by bisection, the
// maximum straight into the global image — to time the LDS form against.  The same bytes: the maximum is order-free.
__global__ void k_place_cells_sub_global(const PlSubSeg* __restrict__ segs, int n_seg, long long total, PlaceLayout L, unsigned* img, int cells) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const PlSubSeg s = segs[seg_of(segs, n_seg, i)];
    const float* p = reinterpret_cast<const float*>(s.src + (size_t)(i - s.first) * (size_t)s.stride);
    float x = p[0], y = p[1], z = p[2];
    if (!s.ident) {
        const float4 r = transform_point(make_float4(x, y, z, 0.f), s.q, s.t);
        x = r.x; y = r.y; z = r.z;
    }
    float val;
    const int cell = place_cell(L, x, y, z, &val);
    if (cell < 0) return;
    const unsigned w = f2ord(val);
    unsigned* a = img + (size_t)s.slot * cells + cell;
    if (*reinterpret_cast<volatile unsigned*>(a) < w) atomicMax(a, w);
}
#endif

// ordered-uint words -> the descriptor's floats, in place (no point: 0)
__global__ void k_place_finish(unsigned* img, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned w = img[i];
    reinterpret_cast<float*>(img)[i] = w ? ord2f(w) : 0.f;
}

// Sector `lane`'s column of a descriptor as a unit vector in f64 (rows >= n_ring and lanes >= n_sector: zeros): products of two f32 values are exact in f64, the
// sum of squares runs ring 0 upward.  Returns whether the column is non-zero; an all-zero column stays zero.
template <int NR>
__device__ __forceinline__ bool unit_column(const float* __restrict__ desc, int lane, int ns, int nr, double (&b)[NR]) {
    const float* col = desc + (size_t)(lane < ns ? lane : 0) * nr;
    double n2 = 0.0;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        b[r] = (lane < ns && r < nr) ? (double)col[r] : 0.0;
        n2 += b[r] * b[r];
    }
    const double nrm = sqrt(n2);
    const bool nz = nrm > 0.0;
#pragma unroll
    for (int r = 0; r < NR; r++) b[r] = nz ? b[r] / nrm : 0.0;
    return nz;
}

struct PlQuery { int id, max_id; double time, min_time_gap; };      // id < 0: the descriptor lies in the batch's upload

// one wave per query: its unit columns ring-major ([ring][64 sectors], kPlMaxRing rows) and its occupancy ballot
__global__ __launch_bounds__(64) void k_place_prep(const PlQuery* __restrict__ qs, const float* __restrict__ store, const float* __restrict__ ext, int ns, int nr,
                                                   double* __restrict__ qcols, unsigned long long* __restrict__ qmask) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const size_t cells = (size_t)ns * nr;
    const float* desc = qs[q].id >= 0 ? store + (size_t)qs[q].id * cells : ext + (size_t)q * cells;
    double b[kPlMaxRing];
    const bool nz = unit_column<kPlMaxRing>(desc, lane, ns, nr, b);
    const unsigned long long m = __ballot(nz);
#pragma unroll
    for (int r = 0; r < kPlMaxRing; r++) qcols[((size_t)q * kPlMaxRing + r) * kPlMaxSector + lane] = b[r];
    if (lane == 0) qmask[q] = m;
}

struct PlScan {
    const float* desc;                  // [n][n_sector * n_ring]
    const double* times;                // [n]
    const double* qcols;                // [n_q][kPlMaxRing][64]
    const unsigned long long* qmask;    // [n_q]
    const PlQuery* qs;
    double* dist;                       // [n_q][n]: min over the shifts, +inf: not eligible or no shift with a common sector
    int* shift;                         // [n_q][n]
    int n, ns, nr, chunk;               // chunk: candidates per workgroup
};

// blockIdx.y = the query, blockIdx.x = a chunk of candidates, one wave per candidate at a time.  NR = n_ring rounded up to a multiple of 4 (zero rows add +0.0).
template <int NR>
__global__ __launch_bounds__(256) void k_place_scan(PlScan a) {
    __shared__ double sA[NR * kPlMaxSector];
    __shared__ double sC[4][kPlShiftGroup * kPlRowPad];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < NR * kPlMaxSector; i += 256) sA[i] = a.qcols[(size_t)q * kPlMaxRing * kPlMaxSector + i];
    const unsigned long long mask_a = a.qmask[q];
    const PlQuery me = a.qs[q];
    __syncthreads();
    double* C = sC[wave];
    const int ns = a.ns;
    const unsigned long long full = ns == 64 ? ~0ull : (1ull << ns) - 1ull;
    const int c_end = min(a.n, (blockIdx.x + 1) * a.chunk);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    for (int c = blockIdx.x * a.chunk + wave; c < c_end; c += 4) {      // (wave-uniform)
        const size_t at = (size_t)q * a.n + c;
        const bool eligible = c <= me.max_id && c != me.id && fabs(a.times[c] - me.time) > me.min_time_gap;
        double b[NR];
        unsigned long long mask_b = 0;
        if (eligible) mask_b = __ballot(unit_column<NR>(a.desc + (size_t)c * ns * a.nr, lane, ns, a.nr, b));
        if (!eligible || !mask_b || !mask_a) {
            if (lane == 0) { a.dist[at] = inf; a.shift[at] = 0; }
            continue;
        }
        const int t = lane & (kPlShiftGroup - 1), part = lane >> 4;
        double best = inf;
        int best_s = 0;
        for (int s0 = 0; s0 < ns; s0 += kPlShiftGroup) {
            for (int u = 0; u < kPlShiftGroup && s0 + u < ns; u++) {
                int col = lane - (s0 + u);                // column j of the query meets column j + s of the candidate
                col = col < 0 ? col + ns : col;
                col = lane < ns ? col : 0;                // (lanes past the last sector hold a zero column)
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < NR; r++) acc += sA[r * kPlMaxSector + col] * b[r];
                C[u * kPlRowPad + lane] = acc;
            }
            wave_lds_order();
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < 16; i++) sum += C[t * kPlRowPad + part * 16 + i];
            const double p0 = __shfl(sum, t), p1 = __shfl(sum, t + 16), p2 = __shfl(sum, t + 32), p3 = __shfl(sum, t + 48);
            const int s = s0 + t;
            if (s < ns) {
                const unsigned long long rot = s ? ((mask_a << s) | (mask_a >> (ns - s))) & full : mask_a;
                const int cnt = __popcll(rot & mask_b);
                const double d = cnt ? 1.0 - (((p0 + p1) + p2) + p3) / (double)cnt : inf;
                if (d < best) { best = d; best_s = s; }      // (a lane's shifts ascend: the smallest shift of a minimum stays)
            }
            wave_lds_order();      // the next group overwrites the rows
        }
#pragma unroll
        for (int m = kPlShiftGroup / 2; m >= 1; m >>= 1) {
            const double od = __shfl_xor(best, m);
            const int os = __shfl_xor(best_s, m);
            if (od < best || (od == best && os < best_s)) { best = od; best_s = os; }
        }
        if (lane == 0) { a.dist[at] = best; a.shift[at] = best < inf ? best_s : 0; }
    }
}

// one workgroup per query: its k smallest finite distances, ascending by (distance, id) — round j takes the smallest pair above round j - 1's
__global__ __launch_bounds__(256) void k_place_topk(const double* __restrict__ dist, const int* __restrict__ shift, int n, int k, lili_place_match* __restrict__ out,
                                                    int* __restrict__ n_found) {
    __shared__ double sd[256];
    __shared__ int si[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const double* d = dist + (size_t)q * n;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double last_d = -inf;
    int last_i = -1, found = 0;
    for (int j = 0; j < k; j++) {
        double bd = inf;
        int bi = INT_MAX;
        for (int c = tid; c < n; c += 256) {
            const double v = d[c];
            if (!(v < inf)) continue;
            if (!(v > last_d || (v == last_d && c > last_i))) continue;
            if (v < bd || (v == bd && c < bi)) { bd = v; bi = c; }
        }
        sd[tid] = bd; si[tid] = bi;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if (tid < w) {
                const double od = sd[tid + w];
                const int oi = si[tid + w];
                if (od < sd[tid] || (od == sd[tid] && oi < si[tid])) { sd[tid] = od; si[tid] = oi; }
            }
            __syncthreads();
        }
        bd = sd[0]; bi = si[0];
        __syncthreads();
        if (bi == INT_MAX) break;      // (uniform: every thread read the same words)
        if (tid == 0) { lili_place_match m; m.id = bi; m.shift = shift[(size_t)q * n + bi]; m.distance = bd; out[(size_t)q * kPlMaxK + j] = m; }
        last_d = bd; last_i = bi; found++;
    }
    if (tid == 0) n_found[q] = found;
}

}  // namespace lili

namespace {

using lili::PlaceLayout;
using lili::PlQuery;
using lili::PlSeg;
using lili::PlSubSeg;
using lili::PlTile;
using lili::kPlTileRows;
using lili::kPlMaxK;
using lili::kPlMaxQuery;
using lili::kPlMaxRing;
using lili::kPlMaxSector;

bool params_ok(const lili_place_params* p) {
    return p && p->n_ring >= 1 && p->n_ring <= kPlMaxRing && p->n_sector >= 4 && p->n_sector <= kPlMaxSector && p->n_sector % 4 == 0 && std::isfinite(p->max_radius) &&
           p->max_radius > 0.f && std::isfinite(p->max_radius * p->max_radius) && std::isfinite(p->lidar_height) && p->kind >= LILI_ARCHIVE_EDGE && p->kind <= LILI_ARCHIVE_FULL;
}
bool same_params(const lili_place_params& a, const lili_place_params& b) {
    return a.n_ring == b.n_ring && a.n_sector == b.n_sector && a.kind == b.kind && std::memcmp(&a.max_radius, &b.max_radius, 4) == 0 &&
           std::memcmp(&a.lidar_height, &b.lidar_height, 4) == 0;
}

PlaceLayout layout_of(const lili_place_params& p) {
    PlaceLayout L{};
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < p.n_ring; k++) { const float b = (p.max_radius * (float)k) / (float)p.n_ring; L.ring_r2[k] = b * b; }
    for (int m = 0; m < p.n_sector / 4; m++) {
        const double a = two_pi * (double)m / (double)p.n_sector;
        L.sec_cos[m] = (float)std::cos(a); L.sec_sin[m] = (float)std::sin(a);
    }
    L.max_r2 = p.max_radius * p.max_radius;
    L.lidar_height = p.lidar_height;
    L.n_ring = p.n_ring; L.n_sector = p.n_sector;
    return L;
}

constexpr int kPlMaxBack = 64, kPlMaxFwd = 16, kPlMaxMembers = kPlMaxBack + kPlMaxFwd + 1;
constexpr long long kPlBatchRows = 1ll << 26;      // rows of one launch of a submap update (a batch holds whole descriptors, one at least)

// one member of a descriptor's build key: 64 bytes without padding, compared bytewise
struct PlKey { int id, ident; double q[4], t[3]; };
static_assert(sizeof(PlKey) == 64, "PlKey is compared bytewise: no padding");

bool submap_ok(const lili_place_submap& s) { return s.back >= 0 && s.back <= kPlMaxBack && s.fwd >= 0 && s.fwd <= kPlMaxFwd && (s.level == 0 || s.level == 1); }
bool submap_plain(const lili_place_submap& s) { return s.back == 0 && s.fwd == 0 && s.level == 0; }

double quat_norm(const double q[4]) { return std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }

// the frame of a LiDAR map pose (include/lili_hip.h "levelled submap descriptors"), statement by statement as the header words it
void frame_of(const double pose[7], int level, double frame[7]) {
    for (int k = 0; k < 7; k++) frame[k] = pose[k];
    if (!level) return;
    const double n = quat_norm(pose + 3);
    const double w = pose[3] / n, x = pose[4] / n, y = pose[5] / n, z = pose[6] / n;
    const double r00 = 1.0 - 2.0 * (y * y + z * z), r10 = 2.0 * (x * y + w * z);
    const double h = std::sqrt(r00 * r00 + r10 * r10);
    double c = 1.0, s = 0.0;
    if (!(h < 1e-9)) { c = r00 / h; s = r10 / h; }
    c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
    const double qz = std::sqrt((1.0 - c) / 2.0);
    frame[3] = std::sqrt((1.0 + c) / 2.0); frame[4] = 0.0; frame[5] = 0.0; frame[6] = s < 0.0 ? -qz : qz;
}

// (q_rel, t_rel) of a member at `pose` in `frame`: f' (x) p and f' . (t_k - t_i), f' the unit frame quaternion's conjugate
void relative_of(const double frame[7], const double pose[7], double q_rel[4], double t_rel[3]) {
    const double nf = quat_norm(frame + 3), np = quat_norm(pose + 3);
    const double a[4] = {frame[3] / nf, -(frame[4] / nf), -(frame[5] / nf), -(frame[6] / nf)};
    const double b[4] = {pose[3] / np, pose[4] / np, pose[5] / np, pose[6] / np};
    q_rel[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
    q_rel[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
    q_rel[2] = ((a[0] * b[2] + a[2] * b[0]) + a[3] * b[1]) - a[1] * b[3];
    q_rel[3] = ((a[0] * b[3] + a[3] * b[0]) + a[1] * b[2]) - a[2] * b[1];
    const double v[3] = {pose[0] - frame[0], pose[1] - frame[1], pose[2] - frame[2]}, u[3] = {a[1], a[2], a[3]};
    double uv[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double cr[3] = {u[1] * uv[2] - u[2] * uv[1], u[2] * uv[0] - u[0] * uv[2], u[0] * uv[1] - u[1] * uv[0]};
    for (int k = 0; k < 3; k++) t_rel[k] = (v[k] + a[0] * uv[k]) + cr[k];
}

bool pose_ok(const double pose[7]) { return pose && finite_n(pose, 7) && quat_norm(pose + 3) > 0.0 && std::isfinite(quat_norm(pose + 3)); }

struct PlaceState : ExtState {
    bool has_params = false;
    lili_place_params params{};
    lili_place_submap sub{};            // all zeros: a keyframe's own rows (the plain path)
    std::vector<std::vector<PlKey>> keys;      // submap setting: the build key of every described keyframe
    DevBuf tiles;
    unsigned long long resets = 0;      // the archive's reset count the descriptors belong to
    int n_desc = 0, cap = 0;            // keyframes 0 .. n_desc - 1 are described; room for `cap`
    DevBuf desc, times;                 // [cap][n_sector * n_ring] f32, [cap] f64
    DevBuf one;                         // lili_place_describe: the image of a caller's cloud (staged rows of a pageable one: the context's staging)
    DevBuf segs, qs, ext, qcols, qmask, dist, shift, out;
    PinBuf h_in, h_out, h_tab;          // h_tab: the segment and tile tables of a k_place_cells_sub launch
    size_t cells() const { return (size_t)params.n_sector * params.n_ring; }
    size_t bytes() const { return desc.cap + times.cap; }
    void drop() { n_desc = 0; keys.clear(); }
};

PlaceState* place_of(lili_ctx* ctx) {
    PlaceState* P = ext_of<PlaceState>(ctx, lili_ctx::kExtPlace);
    const unsigned long long r = lili_archive_resets(ctx);
    if (P->resets != r) { P->resets = r; P->drop(); }      // lili_archive_reset drops every descriptor
    return P;
}

// room for n keyframes: the store grows by half at least and keeps what it holds
int reserve(lili_ctx* ctx, PlaceState* P, int n) {
    if (n <= P->cap) return LILI_OK;
    const int cap = std::max(n, P->cap + P->cap / 2);
    DevBuf d, t;
    HIPCHK(d.ensure((size_t)cap * P->cells() * 4));
    HIPCHK(t.ensure((size_t)cap * 8));
    if (P->n_desc) {
        HIPCHK(hipMemcpyAsync(d.p, P->desc.p, (size_t)P->n_desc * P->cells() * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(t.p, P->times.p, (size_t)P->n_desc * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    P->desc.swap(d); P->times.swap(t);
    P->cap = cap;
    return LILI_OK;
}

// the images `img` (zeroed here, n_img of them) of the concatenation described by `segs` (host; uploaded through P->h_in at byte `h_off`), as floats.  Enqueued only.
int build_images(lili_ctx* ctx, PlaceState* P, const lili_place_params& prm, const std::vector<PlSeg>& segs, long long total, unsigned* img, int n_img, size_t h_off) {
    const size_t cells = (size_t)prm.n_sector * prm.n_ring;
    HIPCHK(hipMemsetAsync(img, 0, (size_t)n_img * cells * 4, ctx->stream));
    if (total > 0) {
        const size_t sb = segs.size() * sizeof(PlSeg);
        HIPCHK(P->segs.ensure(sb));
        std::memcpy(P->h_in.as<unsigned char>() + h_off, segs.data(), sb);
        HIPCHK(hipMemcpyAsync(P->segs.p, P->h_in.as<unsigned char>() + h_off, sb, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(lili::k_place_cells, dim3(nblocks(total, 256)), dim3(256), 0, ctx->stream, (const PlSeg*)P->segs.as<PlSeg>(), (int)segs.size(), total, layout_of(prm), img,
                           (int)cells);
    }
    const long long words = (long long)n_img * (long long)cells;
    hipLaunchKernelGGL(lili::k_place_finish, dim3(nblocks(words, 256)), dim3(256), 0, ctx->stream, img, words);
    HIPCHK(hipGetLastError());
    return LILI_OK;
}

// the tile table of a segment table (segments of one image adjacent, no empty segment): every image's rows cut into runs of at most kPlTileRows, none across two images
void tiles_of(const std::vector<PlSubSeg>& segs, long long total, std::vector<PlTile>& tiles) {
    tiles.clear();
    for (size_t i = 0; i < segs.size();) {
        size_t j = i;
        while (j + 1 < segs.size() && segs[j + 1].slot == segs[i].slot) j++;
        const long long end = j + 1 < segs.size() ? segs[j + 1].first : total;
        size_t si = i;
        for (long long at = segs[i].first; at < end; at += kPlTileRows) {
            while (si < j && segs[si + 1].first <= at) si++;
            PlTile t{};
            t.first = at; t.n = (int)std::min<long long>(kPlTileRows, end - at); t.seg = (int)si; t.slot = segs[i].slot;
            tiles.push_back(t);
        }
        i = j + 1;
    }
}

// build_images through k_place_cells_sub: the segment and tile tables go up together through P->h_tab (nothing of an earlier call may still be in flight from it).  Enqueued only.
int build_images_sub(lili_ctx* ctx, PlaceState* P, const lili_place_params& prm, const std::vector<PlSubSeg>& segs, long long total, unsigned* img, int n_img) {
    const size_t cells = (size_t)prm.n_sector * prm.n_ring;
    HIPCHK(hipMemsetAsync(img, 0, (size_t)n_img * cells * 4, ctx->stream));
    if (total > 0) {
        std::vector<PlTile> tiles;
        tiles_of(segs, total, tiles);
        const size_t sb = segs.size() * sizeof(PlSubSeg), tb = tiles.size() * sizeof(PlTile);
        HIPCHK(P->segs.ensure(sb)); HIPCHK(P->tiles.ensure(tb)); HIPCHK(P->h_tab.ensure(sb + tb));
        std::memcpy(P->h_tab.as<unsigned char>(), segs.data(), sb);
        std::memcpy(P->h_tab.as<unsigned char>() + sb, tiles.data(), tb);
        HIPCHK(hipMemcpyAsync(P->segs.p, P->h_tab.as<unsigned char>(), sb, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(P->tiles.p, P->h_tab.as<unsigned char>() + sb, tb, hipMemcpyHostToDevice, ctx->stream));
#ifdef LILI_PLACE_PROBE_GLOBAL
        hipLaunchKernelGGL(lili::k_place_cells_sub_global, dim3(nblocks(total, 256)), dim3(256), 0, ctx->stream, (const PlSubSeg*)P->segs.as<PlSubSeg>(), (int)segs.size(), total,
                           layout_of(prm), img, (int)cells);
#else
        hipLaunchKernelGGL(lili::k_place_cells_sub, dim3((unsigned)tiles.size()), dim3(256), 0, ctx->stream, (const PlSubSeg*)P->segs.as<PlSubSeg>(), (int)segs.size(),
                           (const PlTile*)P->tiles.as<PlTile>(), layout_of(prm), img, (int)cells);
#endif
    }
    const long long words = (long long)n_img * (long long)cells;
    hipLaunchKernelGGL(lili::k_place_finish, dim3(nblocks(words, 256)), dim3(256), 0, ctx->stream, img, words);
    HIPCHK(hipGetLastError());
    return LILI_OK;
}

// keyframe i's build key from the archive as it is now
void key_of(lili_ctx* ctx, const lili_place_submap& sub, int i, int n, std::vector<PlKey>& key) {
    const int first = std::max(0, i - sub.back), last = std::min(n - 1, i + sub.fwd);
    double pose_i[7], frame[7], pose_k[7];
    lili_archive_map_pose_of(ctx, i, pose_i);
    frame_of(pose_i, sub.level, frame);
    key.clear();
    for (int k = first; k <= last; k++) {
        PlKey e{};
        e.id = k;
        if (k == i && !sub.level) e.ident = 1;      // the centre's own rows in its own frame: read as they are
        else { lili_archive_map_pose_of(ctx, k, pose_k); relative_of(frame, pose_k, e.q, e.t); }
        key.push_back(e);
    }
}

// the submap setting's lili_place_update: every descriptor whose key is missing or no longer the archive's is built, run by run of adjacent keyframes, in batches of
// whole descriptors of about kPlBatchRows rows
int update_submap(lili_ctx* ctx, PlaceState* P, int* n_built) {
    const int n = lili_archive_size(ctx);
    if (n_built) *n_built = 0;
    if (n <= 0) return LILI_OK;
    for (int i = 0; i < n; i++) {
        double pose[7];
        lili_archive_map_pose_of(ctx, i, pose);
        ARGCHK(pose_ok(pose), "place_update: a keyframe's map pose is not finite or its quaternion is zero");
    }
    TRY(reserve(ctx, P, n));
    P->keys.resize((size_t)n);
    std::vector<std::vector<PlKey>> fresh((size_t)n);
    std::vector<int> todo;
    for (int i = 0; i < n; i++) {
        key_of(ctx, P->sub, i, n, fresh[i]);
        const std::vector<PlKey>& old = P->keys[i];
        if (old.size() != fresh[i].size() || std::memcmp(old.data(), fresh[i].data(), old.size() * sizeof(PlKey)) != 0) todo.push_back(i);
    }
    std::vector<PlSubSeg> segs;
    size_t at = 0;
    while (at < todo.size()) {
        const int first = todo[at];
        long long total = 0;
        size_t end = at;
        segs.clear();
        while (end < todo.size() && todo[end] == first + (int)(end - at) && (end == at || total < kPlBatchRows)) {
            const int i = todo[end];
            for (const PlKey& e : fresh[i]) {
                const lili_archive_rows r = lili_archive_rows_of(ctx, e.id, P->params.kind);
                if (r.n <= 0) continue;      // absent or empty: offers nothing
                PlSubSeg s{};
                s.src = reinterpret_cast<const unsigned char*>(r.p); s.first = total; s.stride = 16; s.slot = i - first; s.ident = e.ident;
                s.q = lili::dq{e.q[0], e.q[1], e.q[2], e.q[3]}; s.t = lili::d3{e.t[0], e.t[1], e.t[2]};
                segs.push_back(s);
                total += r.n;
            }
            end++;
        }
        const int n_img = (int)(end - at);
        HIPCHK(P->h_in.ensure((size_t)n_img * 8));
        double* h_times = P->h_in.as<double>();
        for (int j = 0; j < n_img; j++) h_times[j] = lili_archive_rows_of(ctx, first + j, P->params.kind).time;
        HIPCHK(hipMemcpyAsync(P->times.as<double>() + first, h_times, (size_t)n_img * 8, hipMemcpyHostToDevice, ctx->stream));
        TRY(build_images_sub(ctx, P, P->params, segs, total, P->desc.as<unsigned>() + (size_t)first * P->cells(), n_img));
        HIPCHK(hipStreamSynchronize(ctx->stream));      // (the next batch reuses the pinned tables)
        for (size_t j = at; j < end; j++) P->keys[todo[j]].swap(fresh[todo[j]]);
        at = end;
    }
    P->n_desc = n;
    if (n_built) *n_built = (int)todo.size();
    return LILI_OK;
}

template <int NR> void launch_scan(hipStream_t stream, dim3 grid, const lili::PlScan& a) { hipLaunchKernelGGL(lili::k_place_scan<NR>, grid, dim3(256), 0, stream, a); }

void quat_matrix(const double pose[7], double M[16]) {
    const double n = quat_norm(pose + 3);
    const double w = pose[3] / n, x = pose[4] / n, y = pose[5] / n, z = pose[6] / n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) M[4 * i + j] = R[3 * i + j]; M[4 * i + 3] = pose[i]; }
    M[12] = M[13] = M[14] = 0.0; M[15] = 1.0;
}
void mat_mul4(const double A[16], const double B[16], double C[16]) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) { double s = 0.0; for (int k = 0; k < 4; k++) s += A[4 * i + k] * B[4 * k + j]; C[4 * i + j] = s; }
}

// lili_place_describe / _describe_submap (`who`): the checks, where the n clouds are read from (page-locked rows where they lie, pageable ones staged as they are),
// `build(P, src)` — which enqueues the clouds' image into P->one —, and the image copied out.  Blocking.
template <class Build> int describe_clouds(lili_ctx* ctx, const char* who, const lili_cloud* clouds, int n, const lili_place_params* params, float* desc, Build build) {
    ARGCHK(clouds && desc, std::string(who) + ": null argument");
    ARGCHK(params_ok(params), std::string(who) + ": bad parameters (n_ring 1..32, n_sector a multiple of 4 in 4..64, max_radius > 0, kind an archive kind)");
    for (int i = 0; i < n; i++) {
        TRY(lili_cloud_check(ctx, clouds[i], who));
        ARGCHK(clouds[i].stride <= (size_t)INT_MAX, std::string(who) + ": stride too large");
    }
    HIPCHK(hipSetDevice(ctx->device));
    PlaceState* P = place_of(ctx);
    const size_t cells = (size_t)params->n_sector * params->n_ring;
    HIPCHK(P->one.ensure(cells * 4));
    HIPCHK(P->h_out.ensure((size_t)kPlMaxSector * kPlMaxRing * 4));
    std::vector<const unsigned char*> src((size_t)n);
    TRY(lili_cloud_sources(ctx, ctx->staging, clouds, n, kReadPinnedInPlace, src.data()));
    TRY(build(P, src.data()));
    HIPCHK(hipMemcpyAsync(P->h_out.p, P->one.p, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memcpy(desc, P->h_out.p, cells * 4);
    return LILI_OK;
}

}  // namespace

extern "C" {

void lili_place_default_params(lili_place_params* p) {
    if (!p) return;
    p->n_ring = 20; p->n_sector = 60; p->max_radius = 80.f; p->lidar_height = 2.f; p->kind = LILI_ARCHIVE_FULL; p->reserved_ = 0;
}

int lili_place_layout(const lili_place_params* params, float ring_r2[32], float sec_cos[16], float sec_sin[16]) {
    if (!params_ok(params) || !ring_r2 || !sec_cos || !sec_sin) return LILI_E_ARG;
    const PlaceLayout L = layout_of(*params);
    std::memcpy(ring_r2, L.ring_r2, sizeof(L.ring_r2)); std::memcpy(sec_cos, L.sec_cos, sizeof(L.sec_cos)); std::memcpy(sec_sin, L.sec_sin, sizeof(L.sec_sin));
    return LILI_OK;
}

int lili_place_guess(const double pose_src[7], const double pose_dst[7], int shift, int n_sector, double T[16]) {
    if (!pose_src || !pose_dst || !T || n_sector < 1 || !finite_n(pose_src, 7) || !finite_n(pose_dst, 7)) return LILI_E_ARG;
    if (pose_src[3] * pose_src[3] + pose_src[4] * pose_src[4] + pose_src[5] * pose_src[5] + pose_src[6] * pose_src[6] == 0.0) return LILI_E_ARG;
    if (pose_dst[3] * pose_dst[3] + pose_dst[4] * pose_dst[4] + pose_dst[5] * pose_dst[5] + pose_dst[6] * pose_dst[6] == 0.0) return LILI_E_ARG;
    double Ms[16], Md[16], Mi[16], Rz[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, A[16];
    quat_matrix(pose_src, Ms); quat_matrix(pose_dst, Md);
    for (int i = 0; i < 3; i++) {      // M_src^-1 = [R^T, -R^T t]
        for (int j = 0; j < 3; j++) Mi[4 * i + j] = Ms[4 * j + i];
        Mi[4 * i + 3] = -(Ms[i] * Ms[3] + Ms[4 + i] * Ms[7] + Ms[8 + i] * Ms[11]);
    }
    Mi[12] = Mi[13] = Mi[14] = 0.0; Mi[15] = 1.0;
    const double a = 6.283185307179586476925286766559 * (double)shift / (double)n_sector;
    Rz[0] = std::cos(a); Rz[1] = -std::sin(a); Rz[4] = std::sin(a); Rz[5] = std::cos(a);
    mat_mul4(Md, Rz, A);
    mat_mul4(A, Mi, T);
    return LILI_OK;
}

int lili_place_update(lili_ctx* ctx, const lili_place_params* params, int* n_built) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(params_ok(params), "place_update: bad parameters (n_ring 1..32, n_sector a multiple of 4 in 4..64, max_radius > 0, kind an archive kind)");
    HIPCHK(hipSetDevice(ctx->device));
    PlaceState* P = place_of(ctx);
    if (!P->has_params || !same_params(P->params, *params)) {      // other parameters: every descriptor is rebuilt (the store is sized for the new cells)
        HIPCHK(hipStreamSynchronize(ctx->stream));
        P->desc.release(); P->times.release();
        P->cap = 0; P->drop();
        P->params = *params; P->params.reserved_ = 0; P->has_params = true;
    }
    if (!submap_plain(P->sub)) return update_submap(ctx, P, n_built);
    const int n = lili_archive_size(ctx), first = P->n_desc, n_new = n - first;
    if (n_built) *n_built = 0;
    if (n_new <= 0) return LILI_OK;
    TRY(reserve(ctx, P, n));
    std::vector<PlSeg> segs;
    long long total = 0;
    const size_t t_bytes = (size_t)n_new * 8;
    HIPCHK(P->h_in.ensure(t_bytes + (size_t)n_new * sizeof(PlSeg) + 64));
    double* h_times = P->h_in.as<double>();
    for (int i = 0; i < n_new; i++) {
        const lili_archive_rows r = lili_archive_rows_of(ctx, first + i, P->params.kind);
        h_times[i] = r.time;
        if (r.n <= 0) continue;      // absent or empty: all zeros
        PlSeg s{};
        s.src = reinterpret_cast<const unsigned char*>(r.p); s.first = total; s.stride = 16; s.slot = i;
        segs.push_back(s);
        total += r.n;
    }
    HIPCHK(hipMemcpyAsync(P->times.as<double>() + first, h_times, t_bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(build_images(ctx, P, P->params, segs, total, P->desc.as<unsigned>() + (size_t)first * P->cells(), n_new, t_bytes));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    P->n_desc = n;
    if (n_built) *n_built = n_new;
    return LILI_OK;
}

int lili_place_describe(lili_ctx* ctx, const lili_cloud* cloud, const lili_place_params* params, float* desc) {
    if (!ctx) return LILI_E_ARG;
    return describe_clouds(ctx, "place_describe", cloud, 1, params, desc, [&](PlaceState* P, const unsigned char* const* src) {
        HIPCHK(P->h_in.ensure(sizeof(PlSeg) + 64));
        std::vector<PlSeg> segs;
        if (cloud->n) {
            PlSeg s{};
            s.src = src[0]; s.first = 0; s.stride = (int)cloud->stride; s.slot = 0;
            segs.push_back(s);
        }
        return build_images(ctx, P, *params, segs, (long long)cloud->n, P->one.as<unsigned>(), 1, 0);
    });
}

int lili_place_frame(const double pose[7], int level, double frame[7]) {
    if (!pose_ok(pose) || !frame || (level != 0 && level != 1)) return LILI_E_ARG;
    frame_of(pose, level, frame);
    return LILI_OK;
}

int lili_place_relative(const double frame[7], const double pose[7], double q_rel[4], double t_rel[3]) {
    if (!pose_ok(frame) || !pose_ok(pose) || !q_rel || !t_rel) return LILI_E_ARG;
    relative_of(frame, pose, q_rel, t_rel);
    return LILI_OK;
}

int lili_place_set_submap(lili_ctx* ctx, const lili_place_submap* s) {
    if (!ctx) return LILI_E_ARG;
    lili_place_submap v{};
    if (s) v = *s;
    v.reserved_ = 0;
    ARGCHK(submap_ok(v), "place_set_submap: back must be in 0..64, fwd in 0..16, level 0 or 1");
    PlaceState* P = place_of(ctx);
    if (v.back != P->sub.back || v.fwd != P->sub.fwd || v.level != P->sub.level) { P->drop(); P->sub = v; }
    return LILI_OK;
}

int lili_place_get_submap(lili_ctx* ctx, lili_place_submap* s) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(s, "place_get_submap: null argument");
    *s = place_of(ctx)->sub;
    return LILI_OK;
}

int lili_place_window(lili_ctx* ctx, int id, int* first, int* last) {
    if (!ctx) return LILI_E_ARG;
    PlaceState* P = place_of(ctx);
    ARGCHK(first && last, "place_window: null argument");
    ARGCHK(id >= 0 && id < P->n_desc, "place_window: the keyframe has no descriptor (lili_place_update first)");
    if (submap_plain(P->sub)) { *first = *last = id; return LILI_OK; }
    *first = P->keys[(size_t)id].front().id; *last = P->keys[(size_t)id].back().id;
    return LILI_OK;
}

int lili_place_describe_submap(lili_ctx* ctx, const lili_cloud* clouds, int n, const double* q_rel, const double* t_rel, const lili_place_params* params, float* desc) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(n >= 1 && n <= kPlMaxMembers, "place_describe_submap: 1..81 clouds");
    ARGCHK((q_rel == nullptr) == (t_rel == nullptr), "place_describe_submap: q_rel and t_rel are both given or both NULL");
    if (q_rel) ARGCHK(finite_n(q_rel, (size_t)4 * n) && finite_n(t_rel, (size_t)3 * n), "place_describe_submap: a transform is not finite");
    return describe_clouds(ctx, "place_describe_submap", clouds, n, params, desc, [&](PlaceState* P, const unsigned char* const* src) {
        std::vector<PlSubSeg> segs;
        long long total = 0;
        for (int i = 0; i < n; i++) {
            const lili_cloud& c = clouds[i];
            if (!c.n) continue;
            PlSubSeg s{};
            s.src = src[i]; s.first = total; s.stride = (int)c.stride; s.slot = 0;
            const double* q = q_rel ? q_rel + 4 * i : nullptr;
            if (!q || (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0)) s.ident = 1;
            else { s.q = lili::dq{q[0], q[1], q[2], q[3]}; s.t = lili::d3{t_rel[3 * i], t_rel[3 * i + 1], t_rel[3 * i + 2]}; }
            segs.push_back(s);
            total += (long long)c.n;
        }
        return build_images_sub(ctx, P, *params, segs, total, P->one.as<unsigned>(), 1);
    });
}

int lili_place_get(lili_ctx* ctx, int id, float* desc) {
    if (!ctx) return LILI_E_ARG;
    PlaceState* P = place_of(ctx);
    ARGCHK(desc, "place_get: null desc");
    ARGCHK(id >= 0 && id < P->n_desc, "place_get: the keyframe has no descriptor (lili_place_update first)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(desc, P->desc.as<float>() + (size_t)id * P->cells(), P->cells() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

int lili_place_info(lili_ctx* ctx, int* n_described, lili_place_params* params, int64_t* bytes) {
    if (!ctx) return LILI_E_ARG;
    PlaceState* P = place_of(ctx);
    if (n_described) *n_described = P->n_desc;
    if (params) { if (P->has_params) *params = P->params; else lili_place_default_params(params); }
    if (bytes) *bytes = (int64_t)P->bytes();
    return LILI_OK;
}

int lili_place_search(lili_ctx* ctx, const lili_place_query* queries, int n_q, int k, lili_place_match* matches, int* n_found) {
    if (!ctx) return LILI_E_ARG;
    PlaceState* P = place_of(ctx);
    ARGCHK(queries && matches && n_found, "place_search: null argument");
    ARGCHK(n_q >= 1 && n_q <= kPlMaxQuery, "place_search: 1..64 queries");
    ARGCHK(k >= 1 && k <= kPlMaxK, "place_search: k must be in 1..16");
    for (int q = 0; q < n_q; q++) {
        ARGCHK(queries[q].id >= -1, "place_search: a query's id is a keyframe or -1");
        ARGCHK(queries[q].id >= 0 || queries[q].desc, "place_search: a query without a keyframe needs a descriptor");
        ARGCHK(queries[q].id < 0 || queries[q].id < lili_archive_size(ctx), "place_search: a query's keyframe is not in the archive");
        ARGCHK(std::isfinite(queries[q].time) && !std::isnan(queries[q].min_time_gap), "place_search: a query's time must be finite");
    }
    for (int q = 0; q < n_q; q++) n_found[q] = 0;
    const int n = P->n_desc;
    if (n == 0) return LILI_OK;      // nothing is described (a fresh or a reset archive): no candidate
    for (int q = 0; q < n_q; q++) ARGCHK(queries[q].id < n, "place_search: a query's keyframe has no descriptor (lili_place_update first)");
    HIPCHK(hipSetDevice(ctx->device));
    const int ns = P->params.n_sector, nr = P->params.n_ring;
    const size_t cells = P->cells();
    // one upload: the queries, then the descriptors the batch brings along (slot q: query q's, unused for an archived one)
    const size_t q_bytes = (size_t)n_q * sizeof(PlQuery), e_bytes = (size_t)n_q * cells * 4;
    HIPCHK(P->h_in.ensure(q_bytes + e_bytes));
    PlQuery* hq = P->h_in.as<PlQuery>();
    float* he = reinterpret_cast<float*>(P->h_in.as<unsigned char>() + q_bytes);
    bool any_ext = false;
    for (int q = 0; q < n_q; q++) {
        hq[q].id = queries[q].id; hq[q].max_id = queries[q].max_id; hq[q].time = queries[q].time; hq[q].min_time_gap = queries[q].min_time_gap;
        if (queries[q].id < 0) { std::memcpy(he + (size_t)q * cells, queries[q].desc, cells * 4); any_ext = true; }
    }
    HIPCHK(P->qs.ensure(q_bytes)); HIPCHK(P->ext.ensure(e_bytes));
    HIPCHK(P->qcols.ensure((size_t)n_q * kPlMaxRing * kPlMaxSector * 8)); HIPCHK(P->qmask.ensure((size_t)n_q * 8));
    HIPCHK(P->dist.ensure((size_t)n_q * n * 8)); HIPCHK(P->shift.ensure((size_t)n_q * n * 4));
    const size_t m_bytes = (size_t)n_q * kPlMaxK * sizeof(lili_place_match), out_bytes = m_bytes + (size_t)n_q * 4;
    HIPCHK(P->out.ensure(out_bytes)); HIPCHK(P->h_out.ensure(std::max(out_bytes, (size_t)kPlMaxSector * kPlMaxRing * 4)));
    HIPCHK(hipMemcpyAsync(P->qs.p, hq, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (any_ext) HIPCHK(hipMemcpyAsync(P->ext.p, he, e_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(lili::k_place_prep, dim3(n_q), dim3(64), 0, ctx->stream, (const PlQuery*)P->qs.as<PlQuery>(), (const float*)P->desc.as<float>(), (const float*)P->ext.as<float>(), ns, nr,
                       P->qcols.as<double>(), P->qmask.as<unsigned long long>());
    lili::PlScan a{};
    a.desc = P->desc.as<float>(); a.times = P->times.as<double>(); a.qcols = P->qcols.as<double>(); a.qmask = P->qmask.as<unsigned long long>(); a.qs = P->qs.as<PlQuery>();
    a.dist = P->dist.as<double>(); a.shift = P->shift.as<int>(); a.n = n; a.ns = ns; a.nr = nr;
    // candidates per workgroup: about 2048 workgroups in all, 4 (one per wave) to 32 (the query's columns are loaded once per workgroup)
    a.chunk = std::min(32, std::max(4, (int)(((long long)n * n_q / 2048 + 3) / 4 * 4)));
    const dim3 grid(nblocks(n, a.chunk), n_q);
    switch ((nr + 3) / 4) {
        case 1: launch_scan<4>(ctx->stream, grid, a); break;
        case 2: launch_scan<8>(ctx->stream, grid, a); break;
        case 3: launch_scan<12>(ctx->stream, grid, a); break;
        case 4: launch_scan<16>(ctx->stream, grid, a); break;
        case 5: launch_scan<20>(ctx->stream, grid, a); break;
        case 6: launch_scan<24>(ctx->stream, grid, a); break;
        case 7: launch_scan<28>(ctx->stream, grid, a); break;
        default: launch_scan<32>(ctx->stream, grid, a); break;
    }
    lili_place_match* d_m = P->out.as<lili_place_match>();
    int* d_found = reinterpret_cast<int*>(P->out.as<unsigned char>() + m_bytes);
    hipLaunchKernelGGL(lili::k_place_topk, dim3(n_q), dim3(256), 0, ctx->stream, (const double*)P->dist.as<double>(), (const int*)P->shift.as<int>(), n, k, d_m, d_found);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(P->h_out.p, P->out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const lili_place_match* hm = P->h_out.as<lili_place_match>();
    const int* hf = reinterpret_cast<const int*>(P->h_out.as<unsigned char>() + m_bytes);
    for (int q = 0; q < n_q; q++) {
        n_found[q] = hf[q];
        for (int j = 0; j < hf[q]; j++) matches[(size_t)q * k + j] = hm[(size_t)q * kPlMaxK + j];
    }
    return LILI_OK;
}

}  // extern "C"
