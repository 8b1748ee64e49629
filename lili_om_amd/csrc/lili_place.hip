// Place recognition on gfx950: a polar descriptor per archived keyframe in the manner of Scan Context (Kim & Kim, IROS 2018) — n_sector x n_ring
// maximum heights, stored sector-major — and the exact search of a batch of queries against every described keyframe at every circular shift.
// Pieces:
//   * the descriptor: ring and sector of a point by comparisons against tables the host computes once (no arctangent, no square root: lili_place_layout), the cell's
//     maximum by integer atomics on the ordered-uint form of the height.  A maximum does not depend on order: the descriptor is the same bytes on every run and for
//     every split of the work.  One launch over a segment table describes any number of keyframes (k_place_cells), one more turns the words into floats;
//   * the search: a wave holds one candidate, a lane one sector's column as a unit vector in f64; the query's unit columns lie ring-major in LDS, so that at shift s lane l
//     reads column l - s without a bank conflict.  The per-lane cosines of sixteen shifts are parked in LDS and summed per shift in a fixed order (four lanes a shift,
//     sixteen terms each, then the four parts): a pair's distance and shift depend on the two descriptors alone, never on where the candidate lies or what else is in
//     the batch.  The valid count of a shift is a rotate and a popcount of the two occupancy ballots;
//   * the k best of a query: k rounds of a block-wide minimum over (distance, id).
// No floating-point atomics anywhere.
#include "lili_launch.h"
#include "lili_device_cloud.h"

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

struct PlaceState : ExtState {
    bool has_params = false;
    lili_place_params params{};
    unsigned long long resets = 0;      // the archive's reset count the descriptors belong to
    int n_desc = 0, cap = 0;            // keyframes 0 .. n_desc - 1 are described; room for `cap`
    DevBuf desc, times;                 // [cap][n_sector * n_ring] f32, [cap] f64
    DevBuf one;                         // lili_place_describe: the image of a caller's cloud (staged rows of a pageable one: the context's staging)
    DevBuf segs, qs, ext, qcols, qmask, dist, shift, out;
    PinBuf h_in, h_out;
    size_t cells() const { return (size_t)params.n_sector * params.n_ring; }
    size_t bytes() const { return desc.cap + times.cap; }
    void drop() { n_desc = 0; }
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

template <int NR> void launch_scan(hipStream_t stream, dim3 grid, const lili::PlScan& a) { hipLaunchKernelGGL(lili::k_place_scan<NR>, grid, dim3(256), 0, stream, a); }

void quat_matrix(const double pose[7], double M[16]) {
    const double n = std::sqrt(pose[3] * pose[3] + pose[4] * pose[4] + pose[5] * pose[5] + pose[6] * pose[6]);
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
        P->cap = 0; P->n_desc = 0;
        P->params = *params; P->params.reserved_ = 0; P->has_params = true;
    }
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
    ARGCHK(cloud && desc, "place_describe: null argument");
    ARGCHK(params_ok(params), "place_describe: bad parameters (n_ring 1..32, n_sector a multiple of 4 in 4..64, max_radius > 0, kind an archive kind)");
    TRY(lili_archive_check_cloud(ctx, cloud));
    ARGCHK(cloud->stride <= (size_t)INT_MAX, "place_describe: stride too large");
    HIPCHK(hipSetDevice(ctx->device));
    PlaceState* P = place_of(ctx);
    const size_t cells = (size_t)params->n_sector * params->n_ring;
    HIPCHK(P->one.ensure(cells * 4));
    HIPCHK(P->h_in.ensure(sizeof(PlSeg) + 64));
    HIPCHK(P->h_out.ensure((size_t)kPlMaxSector * kPlMaxRing * 4));
    std::vector<PlSeg> segs;
    if (cloud->n) {
        PlSeg s{};
        s.src = static_cast<const unsigned char*>(cloud->data); s.first = 0; s.stride = (int)cloud->stride; s.slot = 0;
        if (cloud->mem == LILI_MEM_HOST) {      // page-locked rows are read where they lie, pageable ones are staged as they are
            if (void* d = lili_pinned_dev_ptr(cloud->data, 4)) s.src = static_cast<const unsigned char*>(d);
            else {
                HIPCHK(ctx->staging.ensure(cloud->n * cloud->stride));
                HIPCHK(hipMemcpyAsync(ctx->staging.p, cloud->data, cloud->n * cloud->stride, hipMemcpyHostToDevice, ctx->stream));
                s.src = ctx->staging.as<unsigned char>();
            }
        }
        segs.push_back(s);
    }
    TRY(build_images(ctx, P, *params, segs, (long long)cloud->n, P->one.as<unsigned>(), 1, 0));
    HIPCHK(hipMemcpyAsync(P->h_out.p, P->one.p, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memcpy(desc, P->h_out.p, cells * 4);
    return LILI_OK;
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
