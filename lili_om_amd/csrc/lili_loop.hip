// Loop-closure registration on gfx950: performLoopClosure — L/src/BackendFusion.cpp:2552-2642 (R/src/BackendFusion.cpp ~2320-2400).
//   * the submaps of detectLoopClosure (transformCloud + concatenation + VoxelGrid, L:2423-2550): lili_loop_assemble in lili_voxel.hip, beside transform_point
//   * pcl::IterativeClosestPoint's default pipeline restated in f64: exact 1-NN on a uniform grid of the target (shell walk with an exact stop rule, the previous
//     iteration's match as a warm start), per-block f64 partials of the Umeyama sums, ONE single-workgroup kernel per iteration that reduces them in fixed order,
//     takes the 3x3 SVD (one-sided Jacobi), updates T and runs DefaultConvergenceCriteria.  Two launches per iteration; iterations are enqueued in batches and the
//     kernels behind the end return at their first instruction; one host synchronisation per batch.
// A context owns one source, one target and its index (LoopState): nothing here touches the matcher's maps, the local map or the voxel filter's state.
#include "lili_ctx.h"
#include "lili_launch.h"
#include "lili_device_math.h"

#include <cfloat>
#include <chrono>
#include <climits>
#include <memory>

int lili_loop_assemble(lili_ctx* ctx, std::unique_ptr<ExtState>& priv, const lili_cloud* clouds, int n_clouds, const double* t, const double* q, float leaf, lili_detail::DevBuf& out, int64_t* n_raw, int64_t* n_ds);
int lili_grid_build_plain(lili_ctx* ctx, lili_detail::MapIndex& m, const float4* d_pts, int n, const double mn[3], const double mx[3], double cell, lili::GridView& out);

namespace lili {

constexpr int kIcpBlock = 256;
constexpr int kIcpPart = 17;      // per-block partials: n, sum p (3), sum q (3), sum p q^T (9, row-major), sum d2 — coordinates relative to the call's origin
constexpr int kBoxBlocks = 256;

// the device state of one align (one per context)
struct IcpDev {
    double T[16];          // accumulated transformation, row-major
    double prev_mse;       // correspondences_prev_mse_
    double fitness;
    long long n_fit;
    int iter, state, converged, done, n_logged, reserved_;
    lili_icp_iteration it[LILI_ICP_MAX_LOG];
};

struct IcpGrid {
    const float4* pts;     // cell-sorted target, w = bitcast(original index)
    const int* cs;         // [n_cells + 1]
    const float4* tgt;     // the target in its own order (warm start)
    int nx, ny, nz;
    double ox, oy, oz, cell, inv_cell;
};

__device__ __forceinline__ void icp_visit(const IcpGrid& g, int c0, int c1, float qx, float qy, float qz, float& bd, int& bi) {
    const int e = g.cs[c1 + 1];
    for (int k = g.cs[c0]; k < e; k++) {
        const float4 p = g.pts[k];
        const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int j = __float_as_int(p.w);
        if (d2 < bd || (d2 == bd && j < bi)) { bd = d2; bi = j; }
    }
}

// Exact 1-NN of (qx, qy, qz) in the target: ties go to the smaller target index.  Chebyshev shells of cells around the query's cell (clipped to the grid), from the first
// shell that meets the grid; before shell r every point not yet seen lies at least lb = (r - 1 + f) cells away (f: the query's smallest distance to a face of its cell,
// in cells) — the walk stops once the best d2 is below lb^2 (shrunk by 4e-6 for the f32 rounding of d2 and of the cell coordinates), or, gated (gate >= 0), once lb
// exceeds the gate (every point left would be rejected).  `hint` (>= 0): a target point whose d2 starts the search (the previous iteration's match).
// bi = INT_MAX: nothing found (gated: nothing within the gate may still be so).
__device__ void icp_nn(const IcpGrid& g, float qx, float qy, float qz, double gate, int hint, float& bd, int& bi) {
    bd = INFINITY; bi = INT_MAX;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) return;
    if (hint >= 0) {
        const float4 p = g.tgt[hint];
        const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 == d2) { bd = d2; bi = hint; }
    }
    const double u[3] = {((double)qx - g.ox) * g.inv_cell, ((double)qy - g.oy) * g.inv_cell, ((double)qz - g.oz) * g.inv_cell};
    const int dims[3] = {g.nx, g.ny, g.nz};
    if (!(fabs(u[0]) < 268435456.0 && fabs(u[1]) < 268435456.0 && fabs(u[2]) < 268435456.0)) {      // beyond 2^28 cells: every point
        icp_visit(g, 0, g.nx * g.ny * g.nz - 1, qx, qy, qz, bd, bi);
        return;
    }
    int c[3], r0 = 0, rmax = 0;
    double f = 0.5;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c[k] = (int)floor(u[k]);
        const double fr = u[k] - (double)c[k];
        f = fmin(f, fmin(fr, 1.0 - fr));
        r0 = max(r0, max(max(-c[k], c[k] - (dims[k] - 1)), 0));
        rmax = max(rmax, max(c[k], dims[k] - 1 - c[k]));
    }
    f = fmax(f, 0.0);
    for (int r = r0; r <= rmax; r++) {
        if (r >= 1) {
            const double lb = ((double)(r - 1) + f) * g.cell * (1.0 - 4e-6);
            if (gate >= 0.0 && lb > gate) break;
            if ((double)bd < lb * lb) break;
        }
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.nx - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.ny - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.nz - 1);
        if (x0 > x1 || y0 > y1 || z0 > z1) continue;
        for (int z = z0; z <= z1; z++) {
            const bool zf = abs(z - c[2]) == r;
            for (int y = y0; y <= y1; y++) {
                const int row = (z * g.ny + y) * g.nx;
                if (zf || abs(y - c[1]) == r) icp_visit(g, row + x0, row + x1, qx, qy, qz, bd, bi);      // a face of the shell: the whole x run
                else {
                    if (c[0] - r >= 0 && c[0] - r < g.nx) icp_visit(g, row + c[0] - r, row + c[0] - r, qx, qy, qz, bd, bi);
                    if (r > 0 && c[0] + r >= 0 && c[0] + r < g.nx) icp_visit(g, row + c[0] + r, row + c[0] + r, qx, qy, qz, bd, bi);
                }
            }
        }
    }
}

// the source point under T: ((r0 x + r1 y) + r2 z) + t in f64 (no contraction: -ffp-contract=off), rounded to f32
__device__ __forceinline__ float3 icp_apply(const double* T, float4 p) {
    const double x = p.x, y = p.y, z = p.z;
    return make_float3((float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]), (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]),
                       (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]));
}

// fixed-order sum of NV doubles over the workgroup (wave butterflies, then the waves in order) -> out[0..NV) from thread 0's view
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* out) {
    __shared__ double w[kIcpBlock / 64][NV];
#pragma unroll
    for (int k = 0; k < NV; k++)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; k++) w[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = w[0][threadIdx.x];
        for (int q = 1; q < kIcpBlock / 64; q++) s += w[q][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

struct IcpCorrArgs {
    IcpGrid g;
    const float4* src;
    int n;
    IcpDev* st;
    int* hint;
    int* out_idx;
    float* out_d2;
    double* part;
    double gate, gate2;
    double o[3];
};

// one iteration's correspondences (determineCorrespondences) and the block's partials of the Umeyama sums
__global__ __launch_bounds__(kIcpBlock) void k_icp_corr(IcpCorrArgs a) {
    if (a.st->done) return;
    const int i = blockIdx.x * kIcpBlock + threadIdx.x;
    double v[kIcpPart];
#pragma unroll
    for (int k = 0; k < kIcpPart; k++) v[k] = 0.0;
    if (i < a.n) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = a.st->T[k];
        const float3 p = icp_apply(T, a.src[i]);
        float bd; int bi;
        icp_nn(a.g, p.x, p.y, p.z, a.gate, a.hint[i], bd, bi);
        a.hint[i] = bi == INT_MAX ? -1 : bi;
        const bool acc = bi != INT_MAX && (double)bd <= a.gate2;
        a.out_idx[i] = acc ? bi : -1;
        a.out_d2[i] = acc ? bd : INFINITY;
        if (acc) {
            const float4 q = a.g.tgt[bi];
            const double P[3] = {(double)p.x - a.o[0], (double)p.y - a.o[1], (double)p.z - a.o[2]};
            const double Q[3] = {(double)q.x - a.o[0], (double)q.y - a.o[1], (double)q.z - a.o[2]};
            v[0] = 1.0;
#pragma unroll
            for (int k = 0; k < 3; k++) { v[1 + k] = P[k]; v[4 + k] = Q[k]; }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int s = 0; s < 3; s++) v[7 + 3 * r + s] = P[r] * Q[s];
            v[16] = (double)bd;
        }
    }
    block_sum<kIcpPart>(v, a.part + (size_t)blockIdx.x * kIcpPart);
}

// Rotation of the SVD solution without scale (TransformationEstimationSVD / Umeyama): H = U S V^T, R = V diag(1, 1, d) U^T with d = sign(det U det V) (PCL negates
// V's third column when det U det V < 0).  One-sided Jacobi on the columns of H gives H V = [s_i u_i]; with u3 := u1 x u2 (= det U * u3) that R is
// v1 u1^T + v2 u2^T + det V * v3 u3^T — u3 never comes from a vanishing singular value (planar source: rank 2).  Rank 1 (collinear): u2 is any unit vector normal to u1.
__device__ void icp_rotation(const double H[9], double R[9]) {
    double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; k++) A[k] = H[k];
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int pr = 0; pr < 3; pr++) {
            const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
            double al = 0, be = 0, ga = 0;
            for (int k = 0; k < 3; k++) { al += A[3 * k + i] * A[3 * k + i]; be += A[3 * k + j] * A[3 * k + j]; ga += A[3 * k + i] * A[3 * k + j]; }
            if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
            for (int k = 0; k < 3; k++) {
                const double ai = A[3 * k + i], aj = A[3 * k + j];
                A[3 * k + i] = c * ai - s * aj; A[3 * k + j] = s * ai + c * aj;
                const double vi = V[3 * k + i], vj = V[3 * k + j];
                V[3 * k + i] = c * vi - s * vj; V[3 * k + j] = s * vi + c * vj;
            }
        }
        if (!rotated) break;
    }
    double sv[3];
    for (int j = 0; j < 3; j++) sv[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    int o[3] = {0, 1, 2};
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2 - a; b++)
            if (sv[o[b]] < sv[o[b + 1]]) { const int tmp = o[b]; o[b] = o[b + 1]; o[b + 1] = tmp; }
    for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (!(sv[o[0]] > 0.0)) return;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
    for (int k = 0; k < 3; k++) { u1[k] = A[3 * k + o[0]] / sv[o[0]]; v1[k] = V[3 * k + o[0]]; v2[k] = V[3 * k + o[1]]; v3[k] = V[3 * k + o[2]]; }
    {
        const double d = u1[0] * A[o[1]] + u1[1] * A[3 + o[1]] + u1[2] * A[6 + o[1]];
        double w[3], nw = 0;
        for (int k = 0; k < 3; k++) { w[k] = A[3 * k + o[1]] - d * u1[k]; nw += w[k] * w[k]; }
        nw = sqrt(nw);
        if (!(nw > 1e-12 * sv[o[0]])) {      // rank 1: the axis u1 has least of, made normal to u1
            int e = 0;
            for (int k = 1; k < 3; k++) if (fabs(u1[k]) < fabs(u1[e])) e = k;
            nw = 0;
            for (int k = 0; k < 3; k++) { w[k] = (k == e ? 1.0 : 0.0) - u1[e] * u1[k]; nw += w[k] * w[k]; }
            nw = sqrt(nw);
        }
        for (int k = 0; k < 3; k++) u2[k] = w[k] / nw;
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double detV = v1[0] * (v2[1] * v3[2] - v2[2] * v3[1]) - v1[1] * (v2[0] * v3[2] - v2[2] * v3[0]) + v1[2] * (v2[0] * v3[1] - v2[1] * v3[0]);
    const double sg = detV < 0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; r++)
        for (int s = 0; s < 3; s++) R[3 * r + s] = (v1[r] * u1[s] + v2[r] * u2[s]) + sg * v3[r] * u3[s];
}

struct IcpStepArgs {
    IcpDev* st;
    const double* part;
    int nb, max_iter;
    double teps, feps;
    double o[3];
};

// one iteration's reduction, increment, update and DefaultConvergenceCriteria (max_iterations_similar_transforms_ = 0, failure_after_max_iter_ = false)
__global__ __launch_bounds__(kIcpBlock) void k_icp_step(IcpStepArgs a) {
    IcpDev* st = a.st;
    if (st->done) return;
    double v[kIcpPart];
#pragma unroll
    for (int k = 0; k < kIcpPart; k++) v[k] = 0.0;
    for (int b = threadIdx.x; b < a.nb; b += kIcpBlock)
#pragma unroll
        for (int k = 0; k < kIcpPart; k++) v[k] += a.part[(size_t)b * kIcpPart + k];
    __shared__ double S[kIcpPart];
    block_sum<kIcpPart>(v, S);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = S[0];
    const int n_corr = (int)n;
    lili_icp_iteration e{};
    e.n_corr = n_corr;
    e.mse = n > 0 ? S[16] / n : 0.0;
    int state;
    if (n_corr < 3) {
        state = LILI_ICP_NO_CORRESPONDENCES;
    } else {
        double pm[3], qm[3], H[9], R[9];
        for (int k = 0; k < 3; k++) { pm[k] = S[1 + k] / n; qm[k] = S[4 + k] / n; }
        for (int r = 0; r < 3; r++)
            for (int s = 0; s < 3; s++) H[3 * r + s] = S[7 + 3 * r + s] - n * pm[r] * qm[s];
        // rank 0 (every accepted source point the same point, or every partner): what the subtraction leaves is the rounding of the sums (about one ulp of
        // them, whatever n: they are tree sums) — no rotation can be read from it, and icp_rotation would make one of the noise.  H = 0 gives R = I.
        double hmax = 0.0, smax = 0.0;
        for (int k = 0; k < 9; k++) { hmax = fmax(hmax, fabs(H[k])); smax = fmax(smax, fabs(S[7 + k])); }
        if (hmax <= 64.0 * DBL_EPSILON * smax)
            for (int k = 0; k < 9; k++) H[k] = 0.0;
        icp_rotation(H, R);
        double t[3];
        for (int r = 0; r < 3; r++) {
            const double P0 = pm[0] + a.o[0], P1 = pm[1] + a.o[1], P2 = pm[2] + a.o[2];
            t[r] = (qm[r] + a.o[r]) - ((R[3 * r] * P0 + R[3 * r + 1] * P1) + R[3 * r + 2] * P2);
        }
        double T0[16], T1[16];
        for (int k = 0; k < 16; k++) T0[k] = st->T[k];
        for (int r = 0; r < 3; r++)
            for (int s = 0; s < 4; s++) T1[4 * r + s] = ((R[3 * r] * T0[s] + R[3 * r + 1] * T0[4 + s]) + R[3 * r + 2] * T0[8 + s]) + t[r] * T0[12 + s];
        for (int s = 0; s < 4; s++) T1[12 + s] = T0[12 + s];
        for (int k = 0; k < 16; k++) st->T[k] = T1[k];
        const int iter = st->iter + 1;
        st->iter = iter;
        e.cos_angle = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
        e.translation_sqr = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
        const double prev = st->prev_mse;
        if (iter >= a.max_iter) state = LILI_ICP_ITERATIONS;
        else if (e.cos_angle >= 1.0 - a.teps && e.translation_sqr <= a.teps) state = LILI_ICP_TRANSFORM;
        else if (fabs(e.mse - prev) < 1e-12) state = LILI_ICP_ABS_MSE;
        else if (fabs(e.mse - prev) / prev < a.feps) state = LILI_ICP_REL_MSE;
        else state = LILI_ICP_NOT_CONVERGED;
        st->prev_mse = e.mse;
    }
    e.state = state;
    if (st->n_logged < LILI_ICP_MAX_LOG) st->it[st->n_logged++] = e;
    st->state = state;
    st->converged = state != LILI_ICP_NOT_CONVERGED && state != LILI_ICP_NO_CORRESPONDENCES;
    if (state != LILI_ICP_NOT_CONVERGED) st->done = 1;
}

struct IcpFitArgs {
    IcpGrid g;
    const float4* src;
    int n;
    const IcpDev* st;
    int behind;            // 1: behind a batch — T from the state, nothing to do until the align is done
    double T[12];
    const int* hint;
    double max_range;
    double* part;
};
// getFitnessScore: the exact, ungated 1-NN d2 of every source point under the final T, summed where d2 <= max_range
__global__ __launch_bounds__(kIcpBlock) void k_icp_fit(IcpFitArgs a) {
    if (a.behind && !a.st->done) return;
    const int i = blockIdx.x * kIcpBlock + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (i < a.n) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = a.behind ? a.st->T[k] : a.T[k];
        const float3 p = icp_apply(T, a.src[i]);
        float bd; int bi;
        icp_nn(a.g, p.x, p.y, p.z, -1.0, a.hint ? a.hint[i] : -1, bd, bi);
        if (bi != INT_MAX && (double)bd <= a.max_range) { v[0] = (double)bd; v[1] = 1.0; }
    }
    block_sum<2>(v, a.part + (size_t)blockIdx.x * 2);
}
__global__ __launch_bounds__(kIcpBlock) void k_icp_fit_reduce(IcpDev* st, const double* part, int nb, int behind) {
    if (behind && !st->done) return;
    double v[2] = {0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += kIcpBlock) { v[0] += part[2 * b]; v[1] += part[2 * b + 1]; }
    __shared__ double S[2];
    block_sum<2>(v, S);
    __syncthreads();
    if (threadIdx.x == 0) { st->n_fit = (long long)S[1]; st->fitness = S[1] > 0 ? S[0] / S[1] : DBL_MAX; }
}

// bounding box and sums of the finite points, per block (fixed grid, fixed order): [min xyz, max xyz] floats, [sum xyz, count] doubles
__global__ __launch_bounds__(kIcpBlock) void k_icp_box(const float4* __restrict__ pts, int n, float* __restrict__ mm, double* __restrict__ sums) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double v[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * kIcpBlock + threadIdx.x; i < n; i += gridDim.x * kIcpBlock) {
        const float4 p = pts[i];
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
        v[0] += p.x; v[1] += p.y; v[2] += p.z; v[3] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        for (int o = 32; o > 0; o >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], o)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o)); }
    __shared__ float w[kIcpBlock / 64][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) for (int k = 0; k < 3; k++) { w[wave][k] = lo[k]; w[wave][3 + k] = hi[k]; }
    block_sum<4>(v, sums + (size_t)blockIdx.x * 4);
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = w[0][threadIdx.x];
        for (int q = 1; q < kIcpBlock / 64; q++) r = threadIdx.x < 3 ? fminf(r, w[q][threadIdx.x]) : fmaxf(r, w[q][threadIdx.x]);
        mm[(size_t)blockIdx.x * 6 + threadIdx.x] = r;
    }
}

}  // namespace lili

namespace {

struct LoopState : ExtState {
    std::unique_ptr<ExtState> vox;               // the assembly's own VoxelGrid buffers (lili_voxel.hip)
    DevBuf cloud[2];
    int64_t n[2] = {0, 0};
    bool has[2] = {false, false};
    MapIndex idx;
    double origin[3] = {0, 0, 0};
    DevBuf hint, out_idx, out_d2, part, fpart, dev, box_mm, box_sums;
    bool has_corr = false;
    std::unique_ptr<lili::IcpDev> h_dev{new lili::IcpDev()}, h_init{new lili::IcpDev()};
};

LoopState* loop_of(lili_ctx* ctx) { return ext_of<LoopState>(ctx, lili_ctx::kExtLoop); }

// the target's index: cells sized from the density (about one point per cell of the box), the centroid as the origin of the partials.  Blocking.
int index_target(lili_ctx* ctx, LoopState* L) {
    const int n = (int)L->n[LILI_LOOP_TARGET];
    L->idx.valid = false;
    if (n == 0) return LILI_OK;
    const float4* pts = L->cloud[LILI_LOOP_TARGET].as<float4>();
    const int nb = std::min(nblocks(n, lili::kIcpBlock), lili::kBoxBlocks);
    HIPCHK(L->box_mm.ensure((size_t)nb * 6 * sizeof(float)));
    HIPCHK(L->box_sums.ensure((size_t)nb * 4 * sizeof(double)));
    hipLaunchKernelGGL(lili::k_icp_box, dim3(nb), dim3(lili::kIcpBlock), 0, ctx->stream, pts, n, L->box_mm.as<float>(), L->box_sums.as<double>());
    HIPCHK(hipGetLastError());
    std::vector<float> mm((size_t)nb * 6);
    std::vector<double> sums((size_t)nb * 4);
    HIPCHK(hipMemcpyAsync(mm.data(), L->box_mm.p, mm.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(sums.data(), L->box_sums.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, s[4] = {0, 0, 0, 0};
    for (int b = 0; b < nb; b++) {
        for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], (double)mm[6 * b + k]); mx[k] = std::max(mx[k], (double)mm[6 * b + 3 + k]); }
        for (int k = 0; k < 4; k++) s[k] += sums[4 * b + k];
    }
    double vol = 1.0;
    if (s[3] > 0) {
        for (int k = 0; k < 3; k++) { L->origin[k] = s[k] / s[3]; vol *= std::max(mx[k] - mn[k], 1.0); }
    } else {
        for (int k = 0; k < 3; k++) { L->origin[k] = 0; mn[k] = mx[k] = 0; }
    }
    double cell = std::cbrt(vol / std::max(s[3], 1.0));
    cell = std::min(std::max(cell, 0.05), 50.0);
    int rc = lili_grid_build_plain(ctx, L->idx, pts, n, mn, mx, cell, L->idx.view);
    if (rc != LILI_OK) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

lili::IcpGrid grid_of(LoopState* L) {
    const GridView& v = L->idx.view;
    lili::IcpGrid g{};
    g.pts = v.pts; g.cs = v.cell_start; g.tgt = L->cloud[LILI_LOOP_TARGET].as<float4>();
    g.nx = v.nx; g.ny = v.ny; g.nz = v.nz; g.ox = v.ox; g.oy = v.oy; g.oz = v.oz; g.cell = v.cell; g.inv_cell = v.inv_cell;
    return g;
}

void enqueue_fitness(lili_ctx* ctx, LoopState* L, bool behind, const double* T, double max_range) {
    const int n = (int)L->n[LILI_LOOP_SOURCE], nb = std::max(nblocks(n, lili::kIcpBlock), 1);
    lili::IcpFitArgs f{};
    f.g = grid_of(L); f.src = L->cloud[LILI_LOOP_SOURCE].as<float4>(); f.n = n; f.st = L->dev.as<lili::IcpDev>(); f.behind = behind ? 1 : 0;
    for (int k = 0; k < 12; k++) f.T[k] = T ? T[k] : 0.0;
    f.hint = behind ? L->hint.as<int>() : nullptr; f.max_range = max_range; f.part = L->fpart.as<double>();
    hipLaunchKernelGGL(lili::k_icp_fit, dim3(nb), dim3(lili::kIcpBlock), 0, ctx->stream, f);
    hipLaunchKernelGGL(lili::k_icp_fit_reduce, dim3(1), dim3(lili::kIcpBlock), 0, ctx->stream, L->dev.as<lili::IcpDev>(), (const double*)L->fpart.as<double>(), nb, behind ? 1 : 0);
}

int ensure_work(lili_ctx* ctx, LoopState* L) {
    const size_t n = (size_t)std::max<int64_t>(L->n[LILI_LOOP_SOURCE], 1), nb = (size_t)nblocks((int64_t)n, lili::kIcpBlock);
    HIPCHK(L->hint.ensure(n * 4)); HIPCHK(L->out_idx.ensure(n * 4)); HIPCHK(L->out_d2.ensure(n * 4));
    HIPCHK(L->part.ensure(nb * lili::kIcpPart * sizeof(double))); HIPCHK(L->fpart.ensure(nb * 2 * sizeof(double)));
    HIPCHK(L->dev.ensure(sizeof(lili::IcpDev)));
    return LILI_OK;
}

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

extern "C" {

void lili_icp_default_params(lili_icp_params* p) {
    if (!p) return;
    *p = lili_icp_params{};
    p->max_corr_dist = 30.0;
    p->max_iterations = 100;
    p->transformation_epsilon = 1e-6;
    p->euclidean_fitness_epsilon = 1e-6;
}

int lili_loop_cloud(lili_ctx* ctx, int which, const lili_cloud* clouds, int n_clouds, const double* t, const double* q, float leaf, int64_t* n_raw, int64_t* n_ds) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(which == LILI_LOOP_SOURCE || which == LILI_LOOP_TARGET, "loop_cloud: bad which");
    ARGCHK(n_clouds >= 1 && clouds && t && q, "loop_cloud: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    LoopState* L = loop_of(ctx);
    L->has[which] = false; L->has_corr = false;
    int64_t nd = 0;
    int rc = lili_loop_assemble(ctx, L->vox, clouds, n_clouds, t, q, leaf, L->cloud[which], n_raw, &nd);
    if (rc != LILI_OK) return rc;
    L->n[which] = nd;
    if (n_ds) *n_ds = nd;
    if (which == LILI_LOOP_TARGET && (rc = index_target(ctx, L)) != LILI_OK) return rc;
    L->has[which] = true;
    return LILI_OK;
}

int lili_icp_set_cloud(lili_ctx* ctx, int which, const lili_cloud* cloud) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(which == LILI_LOOP_SOURCE || which == LILI_LOOP_TARGET, "icp_set_cloud: bad which");
    ARGCHK(cloud, "icp_set_cloud: null cloud");
    HIPCHK(hipSetDevice(ctx->device));
    LoopState* L = loop_of(ctx);
    L->has[which] = false; L->has_corr = false;
    int rc = lili_ingest_cloud(ctx, cloud, L->cloud[which]);
    if (rc != LILI_OK) return rc;
    L->n[which] = (int64_t)cloud->n;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (which == LILI_LOOP_TARGET && (rc = index_target(ctx, L)) != LILI_OK) return rc;
    L->has[which] = true;
    return LILI_OK;
}

int lili_icp_get_cloud(lili_ctx* ctx, int which, lili_feature_out* out) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(which == LILI_LOOP_SOURCE || which == LILI_LOOP_TARGET, "icp_get_cloud: bad which");
    ARGCHK(out, "icp_get_cloud: null out");
    LoopState* L = loop_of(ctx);
    if (!L->has[which]) return ctx->fail(LILI_E_STATE, "icp_get_cloud: no such cloud yet");
    HIPCHK(hipSetDevice(ctx->device));
    size_t k = 0;
    const int rc = copy_rows_enqueue(ctx, L->cloud[which].p, (size_t)L->n[which], out, "icp_get_cloud", &k);
    if (rc != LILI_OK) return rc;
    if (k) HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

int lili_icp_align(lili_ctx* ctx, const lili_icp_params* p, const double guess[16], lili_icp_result* res) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(p && res, "icp_align: null argument");
    ARGCHK(p->max_iterations >= 1 && p->max_corr_dist > 0 && std::isfinite(p->max_corr_dist), "icp_align: max_iterations >= 1 and a positive finite max_corr_dist");
    LoopState* L = loop_of(ctx);
    if (!L->has[LILI_LOOP_SOURCE] || !L->has[LILI_LOOP_TARGET]) return ctx->fail(LILI_E_STATE, "icp_align: set the source and the target first");
    if (L->n[LILI_LOOP_TARGET] == 0 || !L->idx.valid) return ctx->fail(LILI_E_STATE, "icp_align: the target holds no point");
    HIPCHK(hipSetDevice(ctx->device));
    const double t0 = now_us();
    int rc = ensure_work(ctx, L);
    if (rc != LILI_OK) return rc;
    const int n = (int)L->n[LILI_LOOP_SOURCE], nb = std::max(nblocks(n, lili::kIcpBlock), 1);
    lili::IcpDev& init = *L->h_init;
    init = lili::IcpDev{};
    for (int k = 0; k < 16; k++) init.T[k] = guess ? guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
    init.prev_mse = DBL_MAX;
    init.fitness = DBL_MAX;
    init.state = LILI_ICP_NOT_CONVERGED;
    HIPCHK(hipMemcpyAsync(L->dev.p, &init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(L->hint.p, 0xFF, (size_t)std::max(n, 1) * 4, ctx->stream));
    L->has_corr = false;
    lili::IcpCorrArgs ca{};
    ca.g = grid_of(L); ca.src = L->cloud[LILI_LOOP_SOURCE].as<float4>(); ca.n = n; ca.st = L->dev.as<lili::IcpDev>();
    ca.hint = L->hint.as<int>(); ca.out_idx = L->out_idx.as<int>(); ca.out_d2 = L->out_d2.as<float>(); ca.part = L->part.as<double>();
    ca.gate = p->max_corr_dist; ca.gate2 = p->max_corr_dist * p->max_corr_dist;
    lili::IcpStepArgs sa{};
    sa.st = ca.st; sa.part = ca.part; sa.nb = nb; sa.max_iter = p->max_iterations; sa.teps = p->transformation_epsilon; sa.feps = p->euclidean_fitness_epsilon;
    for (int k = 0; k < 3; k++) ca.o[k] = sa.o[k] = L->origin[k];
    // batches of 8, 16, 32, ... iterations: the kernels behind the converged one return at their first instruction; the fitness pass rides behind every batch and
    // does its work behind the one in which the align ended
    int launched = 0, batch = 8, syncs = 0;
    lili::IcpDev& h = *L->h_dev;
    for (;;) {
        const int k = std::min(batch, p->max_iterations - launched);
        for (int j = 0; j < k; j++) {
            hipLaunchKernelGGL(lili::k_icp_corr, dim3(nb), dim3(lili::kIcpBlock), 0, ctx->stream, ca);
            hipLaunchKernelGGL(lili::k_icp_step, dim3(1), dim3(lili::kIcpBlock), 0, ctx->stream, sa);
        }
        launched += k;
        enqueue_fitness(ctx, L, true, nullptr, DBL_MAX);
        HIPCHK(hipGetLastError());
        TRY(lili_readback_now(ctx, &h, L->dev.p, sizeof(h)));
        syncs++;
        if (h.done) break;
        if (launched >= p->max_iterations) return ctx->fail(LILI_E_STATE, "icp_align: internal: the iterations ran out without an end state");
        batch *= 2;
    }
    L->has_corr = true;
    *res = lili_icp_result{};
    for (int k = 0; k < 16; k++) res->transform[k] = h.T[k];
    res->converged = h.converged; res->state = h.state; res->iterations = h.iter; res->n_logged = h.n_logged;
    res->fitness = h.fitness;
    for (int k = 0; k < h.n_logged && k < LILI_ICP_MAX_LOG; k++) res->it[k] = h.it[k];
    res->stage_us[0] = now_us() - t0;
    res->stage_us[1] = (double)syncs;
    res->stage_us[2] = (double)launched;
    return LILI_OK;
}

int lili_icp_fitness(lili_ctx* ctx, const double T[16], double max_range, double* fitness, int64_t* n_used) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(T && fitness, "icp_fitness: null argument");
    LoopState* L = loop_of(ctx);
    if (!L->has[LILI_LOOP_SOURCE] || !L->has[LILI_LOOP_TARGET]) return ctx->fail(LILI_E_STATE, "icp_fitness: set the source and the target first");
    if (L->n[LILI_LOOP_TARGET] == 0 || !L->idx.valid) return ctx->fail(LILI_E_STATE, "icp_fitness: the target holds no point");
    HIPCHK(hipSetDevice(ctx->device));
    int rc = ensure_work(ctx, L);
    if (rc != LILI_OK) return rc;
    enqueue_fitness(ctx, L, false, T, max_range);
    HIPCHK(hipGetLastError());
    lili::IcpDev& h = *L->h_dev;
    TRY(lili_readback_now(ctx, &h, L->dev.p, sizeof(h)));
    *fitness = h.fitness;
    if (n_used) *n_used = h.n_fit;
    return LILI_OK;
}

int lili_icp_get_correspondences(lili_ctx* ctx, size_t capacity, int32_t* target_idx, float* d2) {
    if (!ctx) return LILI_E_ARG;
    LoopState* L = loop_of(ctx);
    if (!L->has_corr) return ctx->fail(LILI_E_STATE, "icp_get_correspondences: no align since the clouds were set");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t k = std::min(capacity, (size_t)L->n[LILI_LOOP_SOURCE]);
    if (k && target_idx) HIPCHK(hipMemcpyAsync(target_idx, L->out_idx.p, k * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (k && d2) HIPCHK(hipMemcpyAsync(d2, L->out_d2.p, k * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

}  // extern "C"
