// Per-frame trajectory on the device (include/lili_hip.h: lili_local_graph*): what buildLocalPoseGraph and optimizeLocalGraph
// (L/src/BackendFusion.cpp:1892-2175, 1309-1384; L/include/factors/LidarPoseFactor.h) compute after a window solve, ONE workgroup of one wave, f64, no contraction.
//
//   walk      lane 0: the IMU propagation from the left keyframe through every non-keyframe scan to the right keyframe, statement for statement (the sample
//             rows staged in LDS by the whole wave first); then one lane per measurement: the relative poses of consecutive nodes;
//   factors   two lanes per factor: the even one the residual and the Jacobian block of the factor's first node, the odd one the block of its second node;
//             analytic, in the local coordinates of ceres::QuaternionParameterization;
//   solve     TrustRegionMinimizer + DoglegStrategy (TRADITIONAL_DOGLEG, Jacobi scaling) of Ceres 2.0, the rules as DESIGN.md §7j lists them.  H = Js^T Js is block
//             tridiagonal with 6 x 6 blocks, kept as a band of kLocalBand entries per row; (H + mu diag^2) x = Js^T r by a left-looking banded Cholesky
//             factorisation (one lane per row of the band under the pivot), the two substitutions by lane 0.  The bookkeeping (gate, order of the checks, log
//             row, summary) is lili_solve_dev.h's, shared with the Levenberg-Marquardt solvers; only how the radius moves is DoglegStrategy's own.
// Nothing waits for another workgroup; every loop is bounded by the sample count, max_iterations, 9 mu rounds or the problem size.
#include "lili_launch.h"
#include "lili_device_math.h"
#include "lili_solve_dev.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

namespace lili {

struct LocalShared {
    double rows[kLocalStageRows * kLocalRow];
    double T[kLocalMaxFrames + 2];
    double left[7], right[7], end_pose[7];
    double x[kLocalMaxFrames][7], xn[kLocalMaxFrames][7];      // accepted point, candidate
    double meas[kLocalMaxFactors][7];
    double r[kLocalMaxFactors][6];
    double J[kLocalMaxFactors][2][36];      // [k][0] = d r_k / d node k, [k][1] = d r_k / d node k + 1 (local coordinates, row-major 6 x 6), at the accepted point
    double colsq[kLocalMaxN], gj[kLocalMaxN];      // |J col|^2 and J^T r, unscaled
    double scale[kLocalMaxN], diag[kLocalMaxN], g[kLocalMaxN], gn[kLocalMaxN], delta[kLocalMaxN], y[kLocalMaxN];
    double H[kLocalMaxN * kLocalBand], L[kLocalMaxN * kLocalBand];
    double tmp[kLocalMaxFactors * 6];
    double mu, alpha, g_norm, gn_norm, g_dot_gn;      // DoglegStrategy's subproblem, kept for the candidates that reuse it
    int reuse;
    LmTrust t;
    int counts[2];
};

__device__ __forceinline__ double lg_wave_sum(double v) {      // every lane gets the same sum
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
// Eigen's inverse(): conjugate / squared norm, the norm summed in coefficient order (x, y, z, w)
__device__ __forceinline__ dq lg_qinv(const dq q) {
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    return dq{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
}
__device__ __forceinline__ dq lg_quat(const double* p) { return dq{p[3], p[4], p[5], p[6]}; }
template <int R, int K, int C>
__device__ __forceinline__ void lg_mm(const double* A, const double* B, double* O) {      // O (R x C) = A (R x K) B (K x C)
#pragma unroll
    for (int i = 0; i < R; i++)
#pragma unroll
        for (int j = 0; j < C; j++) {
            double s = A[i * K] * B[j];
#pragma unroll
            for (int k = 1; k < K; k++) s += A[i * K + k] * B[k * C + j];
            O[i * C + j] = s;
        }
}
__device__ __forceinline__ void lg_plus_jacobian(const dq q, double P[12]) {      // ceres::QuaternionParameterization::ComputeJacobian, 4 x 3
    P[0] = -q.x; P[1] = -q.y; P[2] = -q.z;
    P[3] = q.w; P[4] = q.z; P[5] = -q.y;
    P[6] = -q.z; P[7] = q.w; P[8] = q.x;
    P[9] = q.y; P[10] = -q.x; P[11] = q.w;
}
// rows 1 .. 3 of L(q): (q p)[1..3] = Lv p
__device__ __forceinline__ void lg_lmat_vec(const dq q, double Lv[12]) {
    Lv[0] = q.x; Lv[1] = q.w; Lv[2] = -q.z; Lv[3] = q.y;
    Lv[4] = q.y; Lv[5] = q.z; Lv[6] = q.w; Lv[7] = -q.x;
    Lv[8] = q.z; Lv[9] = -q.y; Lv[10] = q.x; Lv[11] = q.w;
}
// d (q v) / d v for Eigen's q v = v + w (2 u x v) + u x (2 u x v), q not assumed unit: I + 2 w [u]x + 2 (u u^T - |u|^2 I)
__device__ __forceinline__ void lg_rot_matrix(const dq q, double M[9]) {
    const double u[3] = {q.x, q.y, q.z};
    const double uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const double S[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = (i == j ? 1.0 : 0.0) + 2.0 * q.w * S[3 * i + j] + 2.0 * (u[i] * u[j] - (i == j ? uu : 0.0));
}

// 2 vec(dq^-1 qa^-1 qb), then qa^-1 (pb - pa) - dp (LidarPoseFactor.h:23-31); a, b = the poses of the two nodes, m = (dp, dq)
__device__ __forceinline__ void lg_residual(const double* a, const double* b, const double* m, double r[6]) {
    const dq ia = lg_qinv(lg_quat(a)), di = lg_qinv(lg_quat(m));
    const dq e = qmul(qmul(di, ia), lg_quat(b));
    const d3 t = qrot(ia, d3{b[0] - a[0], b[1] - a[1], b[2] - a[2]});
    r[0] = 2.0 * e.x; r[1] = 2.0 * e.y; r[2] = 2.0 * e.z;
    r[3] = t.x - m[0]; r[4] = t.y - m[1]; r[5] = t.z - m[2];
}
// d residual / d local coordinates of the FIRST node (translation block, rotation block): [0, 2 (L(dq^-1) R(qb))_vec D P; -M, Dq D P] with D = d qa^-1 / d qa,
// P = the plus Jacobian at qa, M = lg_rot_matrix(qa^-1), Dq = d (q v) / d q at q = qa^-1, v = pb - pa
__device__ __forceinline__ void lg_jacobian_a(const double* a, const double* b, const double* m, double* J) {
    const dq qa = lg_quat(a), qb = lg_quat(b);
    const double n2 = qa.x * qa.x + qa.y * qa.y + qa.z * qa.z + qa.w * qa.w;
    const dq ia = lg_qinv(qa), di = lg_qinv(lg_quat(m));
    const double iav[4] = {ia.w, ia.x, ia.y, ia.z}, qav[4] = {qa.w, qa.x, qa.y, qa.z};
    double D[16], P[12], K[12];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) D[4 * i + j] = ((i == j ? (i == 0 ? 1.0 : -1.0) : 0.0) - 2.0 * iav[i] * qav[j]) / n2;
    lg_plus_jacobian(qa, P);
    lg_mm<4, 4, 3>(D, P, K);
    // rotation rows: di * ia * qb = L(di) R(qb) ia; rows 1 .. 3 of L(di) R(qb)
    double Lv[12], A[12], Jr[9];
    lg_lmat_vec(di, Lv);
    const double Rb[16] = {qb.w, -qb.x, -qb.y, -qb.z, qb.x, qb.w, qb.z, -qb.y, qb.y, -qb.z, qb.w, qb.x, qb.z, qb.y, -qb.x, qb.w};
    lg_mm<3, 4, 4>(Lv, Rb, A);
    lg_mm<3, 4, 3>(A, K, Jr);
    // translation rows
    const double v[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, u[3] = {ia.x, ia.y, ia.z};
    const double uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    const double Sv[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
    double Dq[12], Jt[9], M[9];
    Dq[0] = 2.0 * (u[1] * v[2] - u[2] * v[1]); Dq[4] = 2.0 * (u[2] * v[0] - u[0] * v[2]); Dq[8] = 2.0 * (u[0] * v[1] - u[1] * v[0]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Dq[4 * i + 1 + j] = -2.0 * ia.w * Sv[3 * i + j] + 2.0 * ((i == j ? uv : 0.0) + u[i] * v[j] - 2.0 * v[i] * u[j]);
    lg_mm<3, 4, 3>(Dq, K, Jt);
    lg_rot_matrix(ia, M);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            J[6 * i + j] = 0.0; J[6 * i + 3 + j] = 2.0 * Jr[3 * i + j];
            J[6 * (3 + i) + j] = -M[3 * i + j]; J[6 * (3 + i) + 3 + j] = Jt[3 * i + j];
        }
}
// ... of the SECOND node: [0, 2 L(dq^-1 qa^-1)_vec P(qb); M, 0]
__device__ __forceinline__ void lg_jacobian_b(const double* a, const double* b, const double* m, double* J) {
    const dq ia = lg_qinv(lg_quat(a)), di = lg_qinv(lg_quat(m));
    double Lv[12], P[12], Jr[9], M[9];
    lg_lmat_vec(qmul(di, ia), Lv);
    lg_plus_jacobian(lg_quat(b), P);
    lg_mm<3, 4, 3>(Lv, P, Jr);
    lg_rot_matrix(ia, M);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            J[6 * i + j] = 0.0; J[6 * i + 3 + j] = 2.0 * Jr[3 * i + j];
            J[6 * (3 + i) + j] = M[3 * i + j]; J[6 * (3 + i) + 3 + j] = 0.0;
        }
}

__device__ __forceinline__ const double* lg_node(const LocalShared& sh, const double (*x)[7], const int n, const int node) {      // node 0 = L, n + 1 = R
    return node == 0 ? sh.left : node == n + 1 ? sh.right : x[node - 1];
}
// residuals, Jacobian blocks, J^T r and the squared column norms at sh.x; returns the cost (every lane the same value)
__device__ __forceinline__ double lg_linearize(LocalShared& sh, const int n) {
    const int lane = threadIdx.x;
    const int N = 6 * n;
    if (lane < 2 * (n + 1)) {
        const int k = lane >> 1;
        const double* a = lg_node(sh, sh.x, n, k);
        const double* b = lg_node(sh, sh.x, n, k + 1);
        if ((lane & 1) == 0) {
            double r[6];
            lg_residual(a, b, sh.meas[k], r);
#pragma unroll
            for (int i = 0; i < 6; i++) sh.r[k][i] = r[i];
            if (k >= 1) lg_jacobian_a(a, b, sh.meas[k], sh.J[k][0]);
        } else if (k < n) lg_jacobian_b(a, b, sh.meas[k], sh.J[k][1]);
    }
    __syncthreads();
    for (int i = lane; i < N; i += kLocalThreads) {      // unknown u is the second node of factor u and the first of factor u + 1
        const int u = i / 6, c = i - 6 * u;
        double gs = 0.0, cs = 0.0;
        for (int row = 0; row < 6; row++) { const double j = sh.J[u][1][6 * row + c]; gs += j * sh.r[u][row]; cs += j * j; }
        for (int row = 0; row < 6; row++) { const double j = sh.J[u + 1][0][6 * row + c]; gs += j * sh.r[u + 1][row]; cs += j * j; }
        sh.gj[i] = gs; sh.colsq[i] = cs;
    }
    double c = 0.0;
    for (int e = lane; e < 6 * (n + 1); e += kLocalThreads) { const double v = sh.r[e / 6][e % 6]; c += v * v; }
    __syncthreads();
    return 0.5 * lg_wave_sum(c);
}
// the lower band of J^T J, columns scaled by s (s == nullptr: unscaled), into out
__device__ __forceinline__ void lg_band(const LocalShared& sh, const int n, const double* s, double* out) {
    const int N = 6 * n;
    for (int e = threadIdx.x; e < N * kLocalBand; e += kLocalThreads) {
        const int i = e / kLocalBand, j = i - (e - kLocalBand * i);
        double v = 0.0;
        if (j >= 0) {
            const int bi = i / 6, ci = i - 6 * bi, bj = j / 6, cj = j - 6 * bj;
            if (bi == bj) {
                for (int row = 0; row < 6; row++) v += sh.J[bi][1][6 * row + ci] * sh.J[bi][1][6 * row + cj];
                for (int row = 0; row < 6; row++) v += sh.J[bi + 1][0][6 * row + ci] * sh.J[bi + 1][0][6 * row + cj];
            } else if (bi == bj + 1) {
                for (int row = 0; row < 6; row++) v += sh.J[bi][1][6 * row + ci] * sh.J[bi][0][6 * row + cj];
            }
            if (s) v = v * s[i] * s[j];
        }
        out[e] = v;
    }
}
// (J d)[row] for the 6 (n + 1) residual rows, d in the unscaled local coordinates
__device__ __forceinline__ double lg_jrow(const LocalShared& sh, const int n, const double* d, const int e) {
    const int k = e / 6, row = e - 6 * k;
    double s = 0.0;
    if (k >= 1) for (int c = 0; c < 6; c++) s += sh.J[k][0][6 * row + c] * d[6 * (k - 1) + c];
    if (k < n) for (int c = 0; c < 6; c++) s += sh.J[k][1][6 * row + c] * d[6 * k + c];
    return s;
}
// sh.L = L L^T in place, left-looking: for column j the lanes 0 .. 11 own the rows j .. j + 11; false = a pivot was not positive
__device__ __forceinline__ bool lg_cholesky(LocalShared& sh, const int N) {
    const int lane = threadIdx.x;
    bool ok = true;
    for (int j = 0; j < N; j++) {
        const int i = j + lane;
        const bool mine = lane < kLocalBand && i < N;
        double acc = 0.0;
        if (mine) {
            acc = sh.L[i * kLocalBand + lane];
            for (int k = max(0, i - (kLocalBand - 1)); k < j; k++) acc -= sh.L[i * kLocalBand + (i - k)] * sh.L[j * kLocalBand + (j - k)];
        }
        const double piv = __shfl(acc, 0);
        ok = ok && (piv > 0.0);
        const double l = sqrt(piv);
        if (mine) sh.L[i * kLocalBand + lane] = lane == 0 ? l : acc / l;
        __syncthreads();
    }
    return ok;
}
// L L^T y = y in place, by ONE lane
__device__ __forceinline__ void lg_substitute(LocalShared& sh, const int N) {
    for (int i = 0; i < N; i++) {
        double s = sh.y[i];
        for (int k = max(0, i - (kLocalBand - 1)); k < i; k++) s -= sh.L[i * kLocalBand + (i - k)] * sh.y[k];
        sh.y[i] = s / sh.L[i * kLocalBand];
    }
    for (int i = N - 1; i >= 0; i--) {
        double s = sh.y[i];
        for (int k = i + 1; k < min(N, i + kLocalBand); k++) s -= sh.L[k * kLocalBand + (k - i)] * sh.y[k];
        sh.y[i] = s / sh.L[i * kLocalBand];
    }
}

// Eigen 3.3's quaternion of a 3 x 3 matrix (the matrix as it is), the branch whose largest diagonal entry is I
template <int I>
__device__ __forceinline__ void lg_m2q_branch(const double* m, double* q) {
    constexpr int Jx = (I + 1) % 3, Kx = (Jx + 1) % 3;
    double t = sqrt(m[3 * I + I] - m[3 * Jx + Jx] - m[3 * Kx + Kx] + 1.0);
    q[1 + I] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[3 * Kx + Jx] - m[3 * Jx + Kx]) * t;
    q[1 + Jx] = (m[3 * Jx + I] + m[3 * I + Jx]) * t;
    q[1 + Kx] = (m[3 * Kx + I] + m[3 * I + Kx]) * t;
}
__device__ __forceinline__ void lg_mat_to_quat(const double* m, double* q) {
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t; q[2] = (m[2] - m[6]) * t; q[3] = (m[3] - m[1]) * t;
    } else if (m[8] > (m[4] > m[0] ? m[4] : m[0])) lg_m2q_branch<2>(m, q);
    else if (m[4] > m[0]) lg_m2q_branch<1>(m, q);
    else lg_m2q_branch<0>(m, q);
}
__device__ __forceinline__ void lg_clamp(double d[3]) {
    if (d[0] > 15.0) d[0] = 15.0;
    if (d[1] > 15.0) d[1] = 15.0;
    if (d[2] > 18.0) d[2] = 18.0;
    if (d[0] < -15.0) d[0] = -15.0;
    if (d[1] < -15.0) d[1] = -15.0;
    if (d[2] < -18.0) d[2] = -18.0;
}
// the mid-point step of L:1947-1953 with zero biases: R is multiplied by the matrix of the un-normalised deltaQ and never re-normalised
__device__ __forceinline__ void lg_step(double P[3], double R[9], double V[3], const double g[3], const double a0[3], const double gy0[3], const double a1[3],
                                        const double gy1[3], const double dt) {
    double u0[3], u1[3], M[9], Rn[9];
#pragma unroll
    for (int i = 0; i < 3; i++) u0[i] = ((R[3 * i] * a0[0] + R[3 * i + 1] * a0[1]) + R[3 * i + 2] * a0[2]) - g[i];
    const double hq[4] = {1.0, (0.5 * (gy0[0] + gy1[0])) * dt / 2.0, (0.5 * (gy0[1] + gy1[1])) * dt / 2.0, (0.5 * (gy0[2] + gy1[2])) * dt / 2.0};
    quat_to_mat(hq, M);
    lg_mm<3, 3, 3>(R, M, Rn);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
#pragma unroll
    for (int i = 0; i < 3; i++) u1[i] = ((R[3 * i] * a1[0] + R[3 * i + 1] * a1[1]) + R[3 * i + 2] * a1[2]) - g[i];
    const double hdd = 0.5 * dt * dt;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double ua = 0.5 * (u0[i] + u1[i]);
        P[i] = P[i] + (dt * V[i] + hdd * ua);
        V[i] = V[i] + dt * ua;
    }
}
// L:1897-2108 by ONE lane: the frames' poses into sh.x, the end state into end_state (P, R, V) and sh.end_pose.  rows = n_rows sample rows (stamp, acc, gyr), row 0 = sample ii0;
// the host has walked the same indices over the stamps and refused a call that would leave the rows — the index is clamped all the same.
__device__ __forceinline__ void lg_walk(LocalShared& sh, const LocalGraphIn& in, const double* rows, double* end_state) {
    const int n = in.n, n_rows = in.n_rows;
    double P[3], V[3], R[9], g[3], d[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, a0[3], gy0[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { P[i] = in.P0[i]; V[i] = in.V0[i]; g[i] = in.g[i]; }
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = in.R0[i];
    auto row = [&](int i) { return rows + (size_t)(i < 0 ? 0 : i < n_rows ? i : n_rows - 1) * kLocalRow; };
    int ii = 0;
    for (int f = 1; f <= n + 1; f++) {
        const bool last = f == n + 1;
        const double tp = sh.T[f - 1], tf = sh.T[f];
        {
            const double* s0 = row(ii);
            const double* s1 = row(ii + 1);
            const double dt1 = tp - s0[0], dt2 = s1[0] - tp;
            const double w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2);
#pragma unroll
            for (int i = 0; i < 3; i++) { d[i] = w1 * s0[1 + i] + w2 * s1[1 + i]; w[i] = w1 * s0[4 + i] + w2 * s1[4 + i]; }
        }
        if (last) lg_clamp(d);      // L:2029-2035; the opening interpolation of a frame's interval (L:1912-1918) is not clamped
#pragma unroll
        for (int i = 0; i < 3; i++) { a0[i] = d[i]; gy0[i] = w[i]; }
        ii++;
        double t_start = tp;
        for (int guard = 0; guard < n_rows && row(ii)[0] < tf; guard++) {
            const double* s = row(ii);
            const double dt = s[0] - t_start;
            t_start = s[0];
#pragma unroll
            for (int i = 0; i < 3; i++) { d[i] = s[1 + i]; w[i] = s[4 + i]; }
            lg_clamp(d);
            lg_step(P, R, V, g, a0, gy0, d, w, dt);
#pragma unroll
            for (int i = 0; i < 3; i++) { a0[i] = d[i]; gy0[i] = w[i]; }
            ii++;
        }
        {
            const double* sp = row(ii - 1);
            const double* s = row(ii);
            const double dt1 = tf - sp[0], dt2 = s[0] - tf;
            const double w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2);
#pragma unroll
            for (int i = 0; i < 3; i++) { d[i] = w1 * d[i] + w2 * s[1 + i]; w[i] = w1 * w[i] + w2 * s[4 + i]; }
            lg_clamp(d);
            lg_step(P, R, V, g, a0, gy0, d, w, dt1);
        }
        double* pose = last ? sh.end_pose : sh.x[f - 1];
        if (!last) ii--;
#pragma unroll
        for (int i = 0; i < 3; i++) pose[i] = (!last && in.f32_positions) ? (double)(float)P[i] : P[i];
        lg_mat_to_quat(R, pose + 3);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { end_state[i] = P[i]; end_state[12 + i] = V[i]; }
#pragma unroll
    for (int i = 0; i < 9; i++) end_state[3 + i] = R[i];
}

__global__ __launch_bounds__(kLocalThreads) void k_local_graph(const LocalGraphIn* __restrict__ inp, LocalGraphOut* __restrict__ out) {
    __shared__ LocalShared sh;
    const int lane = threadIdx.x;
    const LocalGraphIn& in = *inp;
    const int n = in.n, N = 6 * n, mode = in.mode;
    const double* g_rows = reinterpret_cast<const double*>(inp + 1);
    // ---- load
    if (lane < n + 2) sh.T[lane] = in.T[lane];
    if (lane < 7) { sh.left[lane] = in.left[lane]; sh.right[lane] = in.right[lane]; }
    if (!(mode & kLocalWalk)) {
        for (int e = lane; e < 7 * n; e += kLocalThreads) sh.x[e / 7][e % 7] = in.poses[e];
        for (int e = lane; e < 7 * (n + 1); e += kLocalThreads) sh.meas[e / 7][e % 7] = in.meas[e];
    } else if (in.n_rows <= kLocalStageRows) {
        for (int e = lane; e < in.n_rows * kLocalRow; e += kLocalThreads) sh.rows[e] = g_rows[e];
    }
    if (lane == 0) {
        lm_trust_init(sh.t, in.opt);
        sh.mu = 1e-8; sh.reuse = 0; sh.counts[0] = 0; sh.counts[1] = 0;
        sh.alpha = 0.0; sh.g_norm = 0.0; sh.gn_norm = 0.0; sh.g_dot_gn = 0.0;
    }
    __syncthreads();
    // ---- walk and measurements (L:1897-2170)
    if (mode & kLocalWalk) {
        if (lane == 0) lg_walk(sh, in, in.n_rows <= kLocalStageRows ? sh.rows : g_rows, out->end_state);
        __syncthreads();
        if (lane <= n) {      // measurement `lane`: node lane + 1 relative to node lane; the last node is the propagated end state, not the right anchor
            const double* a = lane == 0 ? sh.left : sh.x[lane - 1];
            const double* b = lane < n ? sh.x[lane] : sh.end_pose;
            const dq ia = lg_qinv(lg_quat(a));
            const d3 dp = qrot(ia, d3{b[0] - a[0], b[1] - a[1], b[2] - a[2]});
            const dq dq_ = qmul(ia, lg_quat(b));
            double* m = sh.meas[lane];
            m[0] = dp.x; m[1] = dp.y; m[2] = dp.z; m[3] = dq_.w; m[4] = dq_.x; m[5] = dq_.y; m[6] = dq_.z;
        }
        __syncthreads();
        for (int e = lane; e < 7 * (n + 1); e += kLocalThreads) out->meas[e] = sh.meas[e / 7][e % 7];
        if (!(mode & kLocalSolve)) for (int e = lane; e < 7 * n; e += kLocalThreads) out->poses[e] = sh.x[e / 7][e % 7];
    }
    if (!(mode & (kLocalEvaluate | kLocalSolve))) return;
    // ---- the factors at the given state
    const double cost0 = lg_linearize(sh, n);
    if (mode & kLocalEvaluate) {
        lg_band(sh, n, nullptr, sh.H);
        __syncthreads();
        if (lane == 0) out->cost = cost0;
        for (int i = lane; i < N; i += kLocalThreads) out->gradient[i] = sh.gj[i];
        for (int e = lane; e < N * N; e += kLocalThreads) {
            const int i = e / N, j = e - N * i;
            const int hi = i > j ? i : j, lo = i > j ? j : i;
            out->jtj[e] = hi - lo < kLocalBand ? sh.H[hi * kLocalBand + (hi - lo)] : 0.0;
        }
        return;
    }
    // ---- solve
    lili_local_graph_summary* summary = &out->summary;
    LmTrust& t = sh.t;
    int n_log = 0;
    for (int i = lane; i < N; i += kLocalThreads) sh.scale[i] = 1.0 / (1.0 + sqrt(sh.colsq[i]));      // Jacobi scaling, kept for the whole solve
    if (lane == 0) { t.cost = cost0; if (n == 0) { t.term = LILI_LM_GRADIENT_TOLERANCE; t.go = 0; } }
    __syncthreads();
    while (t.go) {
        // head of the loop: max iterations, gradient max-norm of the unscaled J^T r, radius
        double gmax = 0.0;
        for (int i = 0; i < N; i++) gmax = fmax(gmax, fabs(sh.gj[i]));
        const int it = t.it;
        const double radius = t.radius;
        const bool reuse = sh.reuse != 0;
        double mu = sh.mu;
        const bool go_on = lm_trust_gate(t, gmax, lane);
        __syncthreads();
        if (!go_on) break;
        bool valid = true;
        if (!reuse) {
            // ---- DoglegStrategy's subproblem at a new linearisation: diag, the scaled gradient, alpha, the Gauss-Newton step
            for (int i = lane; i < N; i += kLocalThreads) {
                const double s = sh.scale[i];
                const double dg = sqrt(fmin(fmax(sh.colsq[i] * s * s, t.min_lm_diagonal), t.max_lm_diagonal));
                const double gi = (sh.gj[i] * s) / dg;
                sh.diag[i] = dg; sh.g[i] = gi;
                sh.delta[i] = (gi / dg) * s;      // Js (g / diag) = J (scale g / diag)
            }
            lg_band(sh, n, sh.scale, sh.H);
            __syncthreads();
            double gg = 0.0, jj = 0.0;
            for (int i = lane; i < N; i += kLocalThreads) gg += sh.g[i] * sh.g[i];
            for (int e = lane; e < 6 * (n + 1); e += kLocalThreads) { const double v = lg_jrow(sh, n, sh.delta, e); jj += v * v; }
            gg = lg_wave_sum(gg); jj = lg_wave_sum(jj);
            const double alpha = gg / jj;
            valid = false;
            for (int round = 0; round < 9 && mu < 1.0; round++) {
                __syncthreads();
                for (int e = lane; e < N * kLocalBand; e += kLocalThreads) {
                    const int i = e / kLocalBand;
                    sh.L[e] = sh.H[e] + (e == i * kLocalBand ? mu * (sh.diag[i] * sh.diag[i]) : 0.0);
                }
                for (int i = lane; i < N; i += kLocalThreads) sh.y[i] = sh.gj[i] * sh.scale[i];
                __syncthreads();
                bool ok = lg_cholesky(sh, N);
                if (lane == 0) lg_substitute(sh, N);
                __syncthreads();
                for (int i = lane; i < N; i += kLocalThreads) ok = ok && (sh.y[i] - sh.y[i] == 0.0);      // finite
                if (__all(ok)) { valid = true; break; }
                mu *= 10.0;
            }
            double nn = 0.0, gd = 0.0;
            if (valid) {
                for (int i = lane; i < N; i += kLocalThreads) { const double v = -(sh.y[i] * sh.diag[i]); sh.gn[i] = v; nn += v * v; gd += sh.g[i] * v; }
                mu = fmax(1e-8, 2.0 * mu / 10.0);
            }
            nn = lg_wave_sum(nn); gd = lg_wave_sum(gd);
            __syncthreads();
            if (lane == 0) { sh.alpha = alpha; sh.g_norm = sqrt(gg); sh.gn_norm = sqrt(nn); sh.g_dot_gn = gd; sh.mu = mu; }
            __syncthreads();
        }
        int dcase = 0;
        double mc = 0.0, dogleg_norm = 0.0, step_norm = 0.0;
        if (valid) {
            // ---- the step for this radius, in the diag-scaled space
            const double alpha = sh.alpha, g_norm = sh.g_norm, gn_norm = sh.gn_norm;
            double cg = 0.0, cn = 0.0;      // step = cg g + cn gn
            if (gn_norm <= radius) { dcase = 1; cn = 1.0; }
            else if (alpha * g_norm >= radius) { dcase = 2; cg = -(radius / g_norm); }
            else {
                dcase = 3;
                const double b_dot_a = -alpha * sh.g_dot_gn;
                const double a2 = (alpha * g_norm) * (alpha * g_norm);
                const double bma2 = a2 - 2.0 * b_dot_a + gn_norm * gn_norm;
                const double c = b_dot_a - a2;
                const double d = sqrt(c * c + bma2 * (radius * radius - a2));
                const double beta = c <= 0.0 ? (d - c) / bma2 : (radius * radius - a2) / (d + c);
                cg = -alpha * (1.0 - beta); cn = beta;
            }
            double sn = 0.0, dn = 0.0;
            for (int i = lane; i < N; i += kLocalThreads) {
                const double s = dcase == 1 ? sh.gn[i] : dcase == 2 ? cg * sh.g[i] : cg * sh.g[i] + cn * sh.gn[i];
                const double dl = s / sh.diag[i] * sh.scale[i];
                sh.delta[i] = dl;
                sn += s * s; dn += dl * dl;
            }
            dogleg_norm = sqrt(lg_wave_sum(sn)); step_norm = sqrt(lg_wave_sum(dn));
            __syncthreads();
            // model_cost_change = -(Js d) . (r + Js d / 2), Js d = J delta
            for (int e = lane; e < 6 * (n + 1); e += kLocalThreads) { const double jd = lg_jrow(sh, n, sh.delta, e); mc += jd * (sh.r[e / 6][e % 6] + 0.5 * jd); }
            mc = -lg_wave_sum(mc);
            valid = mc > 0.0;
        }
        if (!valid) {
            // INVALID step (no factorisation, or the model does not descend): DoglegStrategy::StepIsInvalid, the iteration counts, five in a row end the solve
            const int n_inv = t.n_invalid + 1;
            __syncthreads();
            if (lane == 0) {
                sh.mu = sh.mu * 10.0; sh.reuse = 0;
                t.n_invalid = n_inv; t.it = it + 1;
                if (n_inv >= 5) { t.term = LILI_LM_NUMERICAL_FAILURE; t.go = 0; }
            }
            __syncthreads();
            continue;
        }
        // ---- the candidate and its cost
        if (lane < n) {
            const double* d = sh.delta + 6 * lane;
            const double* x = sh.x[lane];
            double* xn = sh.xn[lane];
            for (int i = 0; i < 3; i++) xn[i] = x[i] + d[i];
            quat_plus(x + 3, d + 3, xn + 3, sinc_cos_halving);
        }
        __syncthreads();
        double c = 0.0;
        if (lane <= n) {
            double r[6];
            lg_residual(lg_node(sh, sh.xn, n, lane), lg_node(sh, sh.xn, n, lane + 1), sh.meas[lane], r);
#pragma unroll
            for (int i = 0; i < 6; i++) c += r[i] * r[i];
        }
        const double new_cost = 0.5 * lg_wave_sum(c);
        if (lane == 0) {
            double xn2 = 0.0;
            for (int k = 0; k < n; k++) for (int i = 0; i < 7; i++) xn2 += sh.x[k][i] * sh.x[k][i];
            t.n_invalid = 0; t.model_change = mc; t.step_norm = step_norm;
            const int row = n_log;
            // DoglegStrategy::StepAccepted / StepRejected: halve below 0.25, max(radius, 3 |step|) above 0.75 (no clamp to max_radius); halve
            const int accepted = lm_trust_judge_with(t, new_cost, sqrt(xn2), &summary->lm, n_log, true,
                [dogleg_norm](LmTrust& s, const double rho) {
                    if (rho < 0.25) s.radius *= 0.5;
                    if (rho > 0.75) s.radius = fmax(s.radius, 3.0 * dogleg_norm);
                },
                [](LmTrust& s) { s.radius *= 0.5; });
            if (row < LILI_LM_MAX_LOG) { summary->dogleg_case[row] = dcase; summary->reused[row] = reuse ? 1 : 0; }
            sh.reuse = accepted ? 0 : 1;
        }
        __syncthreads();
        if (t.take) {
            for (int e = lane; e < 7 * n; e += kLocalThreads) sh.x[e / 7][e % 7] = sh.xn[e / 7][e % 7];
            __syncthreads();
            lg_linearize(sh, n);
        }
    }
    __syncthreads();
    for (int e = lane; e < 7 * n; e += kLocalThreads) out->poses[e] = sh.x[e / 7][e % 7];
    if (lane == 0) {      // (n_log is lane 0's: it alone judges)
        if (n == 0) t.it = 0;
        lm_write_summary(&summary->lm, t, cost0, n_log, sh.counts);
        summary->final_mu = sh.mu;
        for (int i = n_log; i < LILI_LM_MAX_LOG; i++) { summary->lm.it[i] = lili_lm_iteration{}; summary->dogleg_case[i] = 0; summary->reused[i] = 0; }      // no row of an earlier call stays
    }
}

}  // namespace lili

namespace {
// The sample indices the walk reads, from the stamps alone (the device walks them the same way): false where the text would read at or beyond n_imu or divide by
// dt1 + dt2 == 0; *hi = the highest index read.
bool walk_indices(const double* st, int64_t n_imu, int64_t ii0, const double* T, int n, int64_t* hi) {
    int64_t ii = ii0;
    *hi = ii0;
    for (int f = 1; f <= n + 1; f++) {
        if (ii + 1 >= n_imu) return false;
        if ((T[f - 1] - st[ii]) + (st[ii + 1] - T[f - 1]) == 0.0) return false;
        ii++;
        for (;;) {
            if (ii >= n_imu) return false;
            if (!(st[ii] < T[f])) break;
            ii++;
        }
        if ((T[f] - st[ii - 1]) + (st[ii] - T[f]) == 0.0) return false;
        if (ii > *hi) *hi = ii;
        if (f != n + 1) ii--;
    }
    return true;
}
int check_options(lili_ctx* ctx, const lili_lm_options* options, lili_lm_options* opt) {
    TRY(lm_options_checked(ctx, "local_graph", options, opt));
    ARGCHK(std::isfinite(opt->function_tolerance) && std::isfinite(opt->gradient_tolerance) && std::isfinite(opt->parameter_tolerance) && std::isfinite(opt->initial_radius) &&
           std::isfinite(opt->max_radius) && std::isfinite(opt->min_relative_decrease) && std::isfinite(opt->max_lm_diagonal), "local_graph: an option is not finite");
    return LILI_OK;
}
int check_walk(lili_ctx* ctx, const lili_local_walk* w, int n, int64_t* hi) {
    ARGCHK(w && w->stamps && w->acc && w->gyr && w->scan_stamps, "local_graph: null argument");
    ARGCHK(n >= 0 && n <= LILI_LOCAL_MAX_FRAMES, "local_graph: n must be in 0 .. 16");
    ARGCHK(w->n_imu >= 2 && w->ii0 >= 0 && w->ii0 < w->n_imu, "local_graph: ii0 outside the sample buffer");
    ARGCHK(finite_n(w->scan_stamps, (size_t)n + 2) && finite_n(w->P0, 3) && finite_n(w->R0, 9) && finite_n(w->V0, 3) && finite_n(w->g, 3) && finite_n(w->left, 7),
           "local_graph: an input is not finite");
    for (int f = 1; f <= n + 1; f++) ARGCHK(w->scan_stamps[f] > w->scan_stamps[f - 1], "local_graph: scan stamps must be strictly increasing");
    ARGCHK(walk_indices(w->stamps, w->n_imu, w->ii0, w->scan_stamps, n, hi), "local_graph: the walk would read a sample at or beyond n_imu, or interpolate with dt1 + dt2 == 0");
    const size_t rows = (size_t)(*hi - w->ii0) + 1;
    ARGCHK(rows <= LILI_IMU_MAX_SAMPLES, "local_graph: more than 4096 samples between the keyframes");
    ARGCHK(finite_n(w->stamps + w->ii0, rows) && finite_n(w->acc + 3 * w->ii0, 3 * rows) && finite_n(w->gyr + 3 * w->ii0, 3 * rows), "local_graph: a sample is not finite");
    return LILI_OK;
}
// fills the header's walk part and returns the number of sample rows; the rows themselves go behind the header
void pack_walk(const lili_local_walk* w, int n, int64_t hi, LocalGraphIn* H, double* rows) {
    const int n_rows = (int)(hi - w->ii0) + 1;
    H->n_rows = n_rows; H->f32_positions = w->f32_positions ? 1 : 0;
    std::memcpy(H->T, w->scan_stamps, sizeof(double) * (n + 2));
    std::memcpy(H->P0, w->P0, sizeof H->P0); std::memcpy(H->R0, w->R0, sizeof H->R0); std::memcpy(H->V0, w->V0, sizeof H->V0); std::memcpy(H->g, w->g, sizeof H->g);
    std::memcpy(H->left, w->left, sizeof H->left);
    for (int k = 0; k < n_rows; k++) {
        double* r = rows + (size_t)k * kLocalRow;
        const int64_t s = w->ii0 + k;
        r[0] = w->stamps[s];
        for (int i = 0; i < 3; i++) { r[1 + i] = w->acc[3 * s + i]; r[4 + i] = w->gyr[3 * s + i]; }
    }
}
// staging sized for n_rows sample rows; the header zeroed, n / mode / options set
int local_begin(lili_ctx* ctx, int n, int mode, int n_rows, const lili_lm_options* opt, StagedJob** Bp, LocalGraphIn** Hp) {
    HIPCHK(hipSetDevice(ctx->device));
    StagedJob* B = ext_of<StagedJob>(ctx, lili_ctx::kExtLocal);
    TRY(B->size(ctx, sizeof(LocalGraphIn) + (size_t)n_rows * kLocalRow * sizeof(double), sizeof(LocalGraphOut)));
    LocalGraphIn* H = B->in.as<LocalGraphIn>();
    std::memset(H, 0, sizeof *H);
    H->n = n; H->mode = mode; H->n_rows = 0;
    if (opt) {
        LocalOptDev& o = H->opt;
        o.max_iter = opt->max_iterations;
        o.function_tolerance = opt->function_tolerance; o.gradient_tolerance = opt->gradient_tolerance; o.parameter_tolerance = opt->parameter_tolerance;
        o.initial_radius = opt->initial_radius; o.max_radius = opt->max_radius; o.min_radius = opt->min_radius; o.min_relative_decrease = opt->min_relative_decrease;
        o.min_lm_diagonal = opt->min_lm_diagonal; o.max_lm_diagonal = opt->max_lm_diagonal;
    }
    *Bp = B; *Hp = H;
    return LILI_OK;
}
// upload, launch, read `out_bytes` of the result back, synchronise
int local_run(lili_ctx* ctx, StagedJob* B, size_t out_bytes) {
    const size_t in_bytes = sizeof(LocalGraphIn) + (size_t)B->in.as<LocalGraphIn>()->n_rows * kLocalRow * sizeof(double);
    return B->run(ctx, ctx->local_graph_time, in_bytes, out_bytes, [&] {
        hipLaunchKernelGGL(k_local_graph, dim3(1), dim3(kLocalThreads), 0, ctx->stream, B->d_in.as<LocalGraphIn>(), B->d_out.as<LocalGraphOut>());
    });
}
const LocalGraphOut* local_out(const StagedJob* B) { return B->out.as<LocalGraphOut>(); }
constexpr size_t kOutSmall = offsetof(LocalGraphOut, jtj);
int check_chain(lili_ctx* ctx, int n, const double* anchors, const double* meas, const double* poses) {
    ARGCHK(n >= 0 && n <= LILI_LOCAL_MAX_FRAMES, "local_graph: n must be in 0 .. 16");
    ARGCHK(anchors && meas && (n == 0 || poses), "local_graph: null argument");
    ARGCHK(finite_n(anchors, 14) && finite_n(meas, 7 * ((size_t)n + 1)) && finite_n(poses, 7 * (size_t)n), "local_graph: an input is not finite");
    return LILI_OK;
}
}  // namespace

extern "C" {

int lili_local_graph_propagate(lili_ctx* ctx, const lili_local_walk* walk, int n, double* poses, double* end_state, double* meas) {
    if (!ctx) return LILI_E_ARG;
    int64_t hi = 0;
    TRY(check_walk(ctx, walk, n, &hi));
    ARGCHK((n == 0 || poses) && end_state && meas, "local_graph_propagate: null argument");
    StagedJob* B; LocalGraphIn* H;
    TRY(local_begin(ctx, n, kLocalWalk, (int)(hi - walk->ii0) + 1, nullptr, &B, &H));
    pack_walk(walk, n, hi, H, reinterpret_cast<double*>(H + 1));
    TRY(local_run(ctx, B, kOutSmall));
    if (n) std::memcpy(poses, local_out(B)->poses, sizeof(double) * 7 * n);
    std::memcpy(end_state, local_out(B)->end_state, sizeof local_out(B)->end_state);
    std::memcpy(meas, local_out(B)->meas, sizeof(double) * 7 * (n + 1));
    return LILI_OK;
}

int lili_local_graph_evaluate(lili_ctx* ctx, int n, const double* anchors, const double* meas, const double* poses, double* cost, double* gradient, double* jtj) {
    if (!ctx) return LILI_E_ARG;
    TRY(check_chain(ctx, n, anchors, meas, poses));
    ARGCHK(cost && (n == 0 || (gradient && jtj)), "local_graph_evaluate: null argument");
    StagedJob* B; LocalGraphIn* H;
    TRY(local_begin(ctx, n, kLocalEvaluate, 0, nullptr, &B, &H));
    std::memcpy(H->left, anchors, sizeof H->left); std::memcpy(H->right, anchors + 7, sizeof H->right);
    std::memcpy(H->meas, meas, sizeof(double) * 7 * (n + 1));
    if (n) std::memcpy(H->poses, poses, sizeof(double) * 7 * n);
    const size_t N = 6 * (size_t)n;
    TRY(local_run(ctx, B, kOutSmall + N * N * sizeof(double)));
    *cost = local_out(B)->cost;
    if (n) { std::memcpy(gradient, local_out(B)->gradient, sizeof(double) * N); std::memcpy(jtj, local_out(B)->jtj, sizeof(double) * N * N); }
    return LILI_OK;
}

int lili_local_graph_solve(lili_ctx* ctx, int n, const double* anchors, const double* meas, double* poses, const lili_lm_options* options,
                           lili_local_graph_summary* summary) {
    if (!ctx) return LILI_E_ARG;
    TRY(check_chain(ctx, n, anchors, meas, poses));
    ARGCHK(summary, "local_graph_solve: null summary");
    lili_lm_options opt;
    TRY(check_options(ctx, options, &opt));
    StagedJob* B; LocalGraphIn* H;
    TRY(local_begin(ctx, n, kLocalSolve, 0, &opt, &B, &H));
    std::memcpy(H->left, anchors, sizeof H->left); std::memcpy(H->right, anchors + 7, sizeof H->right);
    std::memcpy(H->meas, meas, sizeof(double) * 7 * (n + 1));
    if (n) std::memcpy(H->poses, poses, sizeof(double) * 7 * n);
    TRY(local_run(ctx, B, kOutSmall));
    if (n) std::memcpy(poses, local_out(B)->poses, sizeof(double) * 7 * n);
    *summary = local_out(B)->summary;
    return LILI_OK;
}

int lili_local_graph(lili_ctx* ctx, const lili_local_walk* walk, int n, const double* right, const lili_lm_options* options, double* poses, double* meas,
                     lili_local_graph_summary* summary) {
    if (!ctx) return LILI_E_ARG;
    int64_t hi = 0;
    TRY(check_walk(ctx, walk, n, &hi));
    ARGCHK(right && (n == 0 || poses) && meas && summary, "local_graph: null argument");
    ARGCHK(finite_n(right, 7), "local_graph: an input is not finite");
    lili_lm_options opt;
    TRY(check_options(ctx, options, &opt));
    StagedJob* B; LocalGraphIn* H;
    TRY(local_begin(ctx, n, kLocalWalk | kLocalSolve, (int)(hi - walk->ii0) + 1, &opt, &B, &H));
    pack_walk(walk, n, hi, H, reinterpret_cast<double*>(H + 1));
    std::memcpy(H->right, right, sizeof H->right);
    TRY(local_run(ctx, B, kOutSmall));
    if (n) std::memcpy(poses, local_out(B)->poses, sizeof(double) * 7 * n);
    std::memcpy(meas, local_out(B)->meas, sizeof(double) * 7 * (n + 1));
    *summary = local_out(B)->summary;
    return LILI_OK;
}

int lili_local_graph_kernel_ms(lili_ctx* ctx, float* ms) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(ms, "local_graph_kernel_ms: null argument");
    const StagedJob* B = static_cast<const StagedJob*>(ctx->ext[lili_ctx::kExtLocal].get());
    if (!B || B->last_ms < 0.f) return ctx->fail(LILI_E_STATE, "local_graph_kernel_ms: no timed lili_local_graph* call yet (option local_graph_time)");
    *ms = B->last_ms;
    return LILI_OK;
}

}  // extern "C"
