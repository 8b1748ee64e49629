// IMU pre-integration on the device (include/lili_hip.h: lili_imu_preintegrate): what the constructor plus one push_back(dt, acc, gyr)
// per sample leave in a Preintegration object (L/include/factors/Preintegration.h:27-173), one workgroup per segment, f64, no contraction.
//
// Per chunk of kImuChunk samples, five steps separated by workgroup barriers:
//   load     the chunk's sample rows (and the row in front of them: acc0 / gyr0 of its first sample) into LDS;
//   half     one lane per sample: the half rotation un_gyr * dt / 2 — it does not depend on the state;
//   chain    lane 0: delta_q <- normalize(delta_q * (1, half)) sample after sample, the only serial part that divides; every sample's delta_q before the
//            step and the un-normalised result are kept.  Lane 64 (another wave, at the same time): the state propagation of processIMU, if asked for;
//   blocks   one lane per sample: the rotated accelerations, the increments of delta_p / delta_v, and the 3 x 3 blocks of F and V, statement for statement;
//   apply    225 threads own one entry of the 15 x 15 matrices and take the samples in order: A = F P and J <- F J, barrier, P <- A F^T + V N V^T, barrier.
//            Each thread knows, from before the first sample, where in a record the coefficients of its two rows of F and V lie (a row of F has at most
//            11 entries that are not structurally zero, the rows of V meet in at most 12 columns; shorter lists are padded with a stored 0.0), so a
//            sample is a straight run of LDS loads and multiply-adds without a branch.  Thread 255 adds the sample's increments to delta_p / delta_v /
//            sum_dt inside the same loop.
// Every sum runs in ascending index order and leaves out only terms whose factor is a structural zero of F, V or N — the order of the reference's own
// products compiled with textbook loops.  The state values therefore come out of the same IEEE operations in the same order as on the host.
#include "lili_launch.h"
#include "lili_device_math.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

static_assert(offsetof(lili::ImuOutDev, P1) == sizeof(lili_window_imu), "ImuOutDev starts with lili_window_imu's numbers");
static_assert(sizeof(lili::ImuOutDev) - offsetof(lili::ImuOutDev, P1) == sizeof(lili_imu_prediction), "... and ends with lili_imu_prediction's");

namespace lili {

// one record per sample of the chunk, doubles.  While the chain runs: [0] dt, [1..3] half rotation, [4..7] delta_q before the step, [8..11] the un-normalised
// result.  After `blocks`: [0] dt, [1..3] increment of delta_p, [4..6] of delta_v, then the blocks.
constexpr int kRecDt = 0, kRecHalf = 1, kRecDq = 4, kRecRq = 8, kRecIncP = 1, kRecIncV = 4;
constexpr int kF03 = 7, kF09 = 16, kF0C = 25, kF33 = 34, kF63 = 43, kF69 = 52, kF6C = 61, kV00 = 70, kV03 = 79, kV06 = 88, kV60 = 97, kV63 = 106, kV66 = 115;
constexpr int kC0 = 124, kC1 = 125, kCNegDt = 126, kCHalfDt = 127;      // 0.0, 1.0, -dt, 0.5 dt: the multiples of the identity read like any other coefficient
constexpr int kImuRec = 129;                                             // (odd: the lanes of `blocks` write their records side by side without bank conflicts)
// A row of F as the list of its entries that are not structurally zero, in ascending column order, by row block (rows 3 rb .. 3 rb + 2; r = row - 3 rb):
// mode 0 = entry of a stored block: coefficient at base + 3 r, column k; mode 1 = multiple of the identity: coefficient at base, column k + r; mode 2 = padding.
constexpr int kImuFTerms = 11;
struct ImuTerm { short base, k, mode; };
#define BLK(b, c) {(short)((b) + 0), (short)(c), 0}, {(short)((b) + 1), (short)((c) + 1), 0}, {(short)((b) + 2), (short)((c) + 2), 0}
#define DIA(b, c) {(short)(b), (short)(c), 1}
#define PAD {(short)kC0, 0, 2}
__device__ const ImuTerm kImuFRow[5][kImuFTerms] = {
    {DIA(kC1, 0), BLK(kF03, 3), DIA(kRecDt, 6), BLK(kF09, 9), BLK(kF0C, 12)},
    {BLK(kF33, 3), DIA(kCNegDt, 12), PAD, PAD, PAD, PAD, PAD, PAD, PAD},
    {BLK(kF63, 3), DIA(kC1, 6), BLK(kF69, 9), BLK(kF6C, 12), PAD},
    {DIA(kC1, 9), PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD},
    {DIA(kC1, 12), PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD}};
#undef BLK
#undef DIA
#undef PAD
// The first four column blocks of V by row block: a stored block (offset), zero, or 0.5 dt I.  Rows 9 .. 14 have one entry each, dt in column 12 + (row - 9): it
// meets no other row, so V N V^T has dt n dt on those diagonal entries and nothing else there.
constexpr int kVZero = -1, kVHalfDt = -2;
__device__ const int kImuVRow[5][4] = {{kV00, kV03, kV06, kV03}, {kVZero, kVHalfDt, kVZero, kVHalfDt}, {kV60, kV63, kV66, kV63}, {kVZero, kVZero, kVZero, kVZero},
                                       {kVZero, kVZero, kVZero, kVZero}};

// Eigen 3.3's formulas, as the reference's build evaluates them
__device__ __forceinline__ void imu_quat_rotate(const double q[4], const double v[3], double o[3]) {      // QuaternionBase::_transformVector
    const double u0 = q[1], u1 = q[2], u2 = q[3];
    double c0 = u1 * v[2] - u2 * v[1], c1 = u2 * v[0] - u0 * v[2], c2 = u0 * v[1] - u1 * v[0];
    c0 = c0 + c0; c1 = c1 + c1; c2 = c2 + c2;
    const double d0 = u1 * c2 - u2 * c1, d1 = u2 * c0 - u0 * c2, d2 = u0 * c1 - u1 * c0;
    o[0] = (v[0] + c0 * q[0]) + d0; o[1] = (v[1] + c1 * q[0]) + d1; o[2] = (v[2] + c2 * q[0]) + d2;
}
__device__ __forceinline__ void imu_skew(const double v[3], double S[9]) {
    S[0] = 0.0; S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2]; S[4] = 0.0; S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0]; S[8] = 0.0;
}
__device__ __forceinline__ void imu_mul(const double A[9], const double B[9], double C[9]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { double s = A[3 * i] * B[j]; s += A[3 * i + 1] * B[3 + j]; s += A[3 * i + 2] * B[6 + j]; C[3 * i + j] = s; }
}
__device__ __forceinline__ void imu_lscale(double s, const double A[9], double C[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = s * A[i];
}
__device__ __forceinline__ void imu_rscale(const double A[9], double s, double C[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = A[i] * s;
}
__device__ __forceinline__ void imu_add(const double A[9], const double B[9], double C[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = A[i] + B[i];
}
__device__ __forceinline__ void imu_store(double* dst, const double A[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) dst[i] = A[i];
}

// MidPointIntegration's F and V blocks (Preintegration.h:98-143) and the state increments of one sample; rec holds dt, delta_q and the un-normalised result
__device__ void imu_blocks(double* rec, const double* prev, const double* cur, const double ba[3], const double bg[3]) {
    const double dt = rec[kRecDt];
    double dqv[4], rq[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { dqv[i] = rec[kRecDq + i]; rq[i] = rec[kRecRq + i]; }
    double a0[3], a1[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { a0[i] = prev[1 + i] - ba[i]; a1[i] = cur[1 + i] - ba[i]; w[i] = 0.5 * (prev[4 + i] + cur[4 + i]) - bg[i]; }
    // the state: un_acc = 0.5 (delta_q a0 + result_delta_q a1); delta_p + delta_v dt + [0.5 un_acc dt dt]; delta_v + [un_acc dt]
    double u0[3], u1[3];
    imu_quat_rotate(dqv, a0, u0);
    imu_quat_rotate(rq, a1, u1);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double ua = 0.5 * (u0[i] + u1[i]);
        rec[kRecIncP + i] = 0.5 * ua * dt * dt;
        rec[kRecIncV + i] = ua * dt;
    }
    double Rd[9], Rr[9], A0[9], A1[9], W[9], IW[9], T[9], U[9], X[9];
    quat_to_mat(dqv, Rd);
    quat_to_mat(rq, Rr);
    imu_skew(a0, A0); imu_skew(a1, A1); imu_skew(w, W);
    const double ndt = -dt;
    rec[kC0] = 0.0; rec[kC1] = 1.0; rec[kCNegDt] = ndt; rec[kCHalfDt] = 0.5 * dt;      // 1, -1 dt, (0.5 * 1) dt: the diagonal entries of F and V that are no stored block
#pragma unroll
    for (int i = 0; i < 9; i++) IW[i] = ((i % 4 == 0) ? 1.0 : 0.0) - W[i] * dt;      // Matrix3d::Identity() - R_w_x * dt
    imu_store(rec + kF33, IW);
    // F(0,3) = -0.25 Rd Ra0 dt dt + -0.25 Rr Ra1 (I - Rw dt) dt dt
    imu_lscale(-0.25, Rd, T); imu_mul(T, A0, U); imu_rscale(U, dt, T); imu_rscale(T, dt, U);                  // U = first summand
    double Q1[9];                                                                                              // Q1 = -0.25 Rr Ra1, kept for V(0,3)
    imu_lscale(-0.25, Rr, T); imu_mul(T, A1, Q1);
    imu_mul(Q1, IW, T); imu_rscale(T, dt, X); imu_rscale(X, dt, T);
    imu_add(U, T, X); imu_store(rec + kF03, X);
    // V(0,3) = -0.25 Rr Ra1 dt dt 0.5 dt
    imu_rscale(Q1, dt, T); imu_rscale(T, dt, U); imu_rscale(U, 0.5, T); imu_rscale(T, dt, U); imu_store(rec + kV03, U);
    // F(0,9) = -0.25 (Rd + Rr) dt dt,  F(6,9) = -0.5 (Rd + Rr) dt
    imu_add(Rd, Rr, X);
    imu_lscale(-0.25, X, T); imu_rscale(T, dt, U); imu_rscale(U, dt, T); imu_store(rec + kF09, T);
    imu_lscale(-0.5, X, T); imu_rscale(T, dt, U); imu_store(rec + kF69, U);
    // F(0,12) = -0.1667 Rr Ra1 dt dt (-dt)
    imu_lscale(-0.1667, Rr, T); imu_mul(T, A1, U); imu_rscale(U, dt, T); imu_rscale(T, dt, U); imu_rscale(U, ndt, T); imu_store(rec + kF0C, T);
    // F(6,3) = -0.5 Rd Ra0 dt + -0.5 Rr Ra1 (I - Rw dt) dt
    imu_lscale(-0.5, Rd, T); imu_mul(T, A0, U); imu_rscale(U, dt, X);                                          // X = first summand
    double H1[9];                                                                                              // H1 = -0.5 Rr Ra1 (= 0.5 (-Rr) Ra1 of V(6,3), same bits)
    imu_lscale(-0.5, Rr, T); imu_mul(T, A1, H1);
    imu_mul(H1, IW, T); imu_rscale(T, dt, U);
    imu_add(X, U, T); imu_store(rec + kF63, T);
    // F(6,12) = -0.5 Rr Ra1 dt (-dt),  V(6,3) = 0.5 (-Rr) Ra1 dt 0.5 dt
    imu_rscale(H1, dt, T);
    imu_rscale(T, ndt, U); imu_store(rec + kF6C, U);
    imu_rscale(T, 0.5, U); imu_rscale(U, dt, X); imu_store(rec + kV63, X);
    // V(0,0) = 0.5 Rd dt dt, V(6,0) = 0.5 Rd dt, V(0,6) = 0.5 Rr dt dt, V(6,6) = 0.5 Rr dt
    imu_lscale(0.5, Rd, T); imu_rscale(T, dt, U); imu_store(rec + kV60, U); imu_rscale(U, dt, T); imu_store(rec + kV00, T);
    imu_lscale(0.5, Rr, T); imu_rscale(T, dt, U); imu_store(rec + kV66, U); imu_rscale(U, dt, T); imu_store(rec + kV06, T);
}

__global__ __launch_bounds__(kImuThreads) void k_imu_preintegrate(const ImuSegDev* __restrict__ segs, const double* __restrict__ rows, ImuOutDev* __restrict__ out) {
    __shared__ double s_rec[kImuChunk * kImuRec];
    __shared__ double s_smp[(kImuChunk + 1) * kImuRow];
    __shared__ double s_J[2][225], s_P[225], s_A[225];
    const int tid = threadIdx.x;
    const ImuSegDev& S = segs[blockIdx.x];
    ImuOutDev& O = out[blockIdx.x];
    const int n = S.n;
    const double* seg_rows = rows + S.first_row * kImuRow;
    double ba[3], bg[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { ba[i] = S.ba[i]; bg[i] = S.bg[i]; }
    // the noise diagonal per column block of V: acc_n, gyr_n, acc_n, gyr_n (then acc_w, gyr_w), squared (Preintegration.h:40-54)
    const double acc_n = 0.00059, gyr_n = 0.000061, acc_w = 0.000011, gyr_w = 0.000001;
    const double nz[4] = {acc_n * acc_n, gyr_n * gyr_n, acc_n * acc_n, gyr_n * gyr_n};      // columns 12 .. 14 / 15 .. 17: acc_w, gyr_w (nzd below)
    // the thread's matrix entry and where the coefficients of its two rows lie in a record
    const int ti = tid < 225 ? tid / 15 : 0, tj = tid < 225 ? tid % 15 : 0;
    const int bi = ti / 3, ri = ti % 3, bj = tj / 3, rj = tj % 3;
    int fiOff[kImuFTerms], fiX[kImuFTerms], fjOff[kImuFTerms], fjA[kImuFTerms];      // rows ti and tj of F: coefficient offsets, and where the other factor lies (P / J column tj; A row ti)
#pragma unroll
    for (int t = 0; t < kImuFTerms; t++) {
        const ImuTerm a = kImuFRow[bi][t], b = kImuFRow[bj][t];
        fiOff[t] = a.base + (a.mode == 0 ? 3 * ri : 0);
        fiX[t] = (a.k + (a.mode == 1 ? ri : 0)) * 15 + tj;
        fjOff[t] = b.base + (b.mode == 0 ? 3 * rj : 0);
        fjA[t] = ti * 15 + b.k + (b.mode == 1 ? rj : 0);
    }
    int viOff[12], vjOff[12];                                                         // columns 0 .. 11 of rows ti and tj of V
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const int ci = kImuVRow[bi][k / 3], cj = kImuVRow[bj][k / 3], kc = k % 3;
        viOff[k] = ci >= 0 ? ci + 3 * ri + kc : (ci == kVHalfDt && kc == ri) ? kCHalfDt : kC0;
        vjOff[k] = cj >= 0 ? cj + 3 * rj + kc : (cj == kVHalfDt && kc == rj) ? kCHalfDt : kC0;
    }
    const int vdOff = (ti == tj && ti >= 9) ? kRecDt : kC0;                          // rows 9 .. 14: dt in a column of their own
    const double nzd = ti < 12 ? acc_w * acc_w : gyr_w * gyr_w;
    if (tid < 225) { s_J[0][tid] = ti == tj ? 1.0 : 0.0; s_P[tid] = 0.0001 * (ti == tj ? 1.0 : 0.0); }
    // the serial states, each in the registers of the one thread that advances it
    double q[4] = {1.0, 0.0, 0.0, 0.0};                                    // thread 0
    double dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, sum_dt = 0.0;   // thread 255
    double pP[3], pR[9], pV[3], g[3];                                       // thread 64; g = processIMU's g: the factor's g_vec_ is -g (L:807)
#pragma unroll
    for (int i = 0; i < 3; i++) { pP[i] = S.P0[i]; pV[i] = S.V0[i]; g[i] = -S.g[i]; }
#pragma unroll
    for (int i = 0; i < 9; i++) pR[i] = S.R0[i];
    const bool predict = S.predict != 0;
    int cur = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += kImuChunk) {
        const int nc = min(kImuChunk, n - c0);
        // ---- load: rows c0 .. c0 + nc of the segment (row c0 = the sample in front of the chunk)
        for (int e = tid; e < (nc + 1) * kImuRow; e += kImuThreads) s_smp[e] = seg_rows[(size_t)c0 * kImuRow + e];
        __syncthreads();
        // ---- half: un_gyr = 0.5 (gyr0 + gyr1) - bg; (un_gyr dt) / 2
        if (tid < nc) {
            const double* p = s_smp + tid * kImuRow;
            const double* c = p + kImuRow;
            double* rec = s_rec + tid * kImuRec;
            const double dt = c[0];
            rec[kRecDt] = dt;
#pragma unroll
            for (int i = 0; i < 3; i++) { const double ug = 0.5 * (p[4 + i] + c[4 + i]) - bg[i]; rec[kRecHalf + i] = ug * dt / 2.0; }
        }
        __syncthreads();
        // ---- chain
        if (tid == 0) {
            for (int k = 0; k < nc; k++) {
                double* rec = s_rec + k * kImuRec;
                const double bx = rec[kRecHalf], by = rec[kRecHalf + 1], bz = rec[kRecHalf + 2], bw = 1.0;
                const double aw = q[0], ax = q[1], ay = q[2], az = q[3];
                double r[4];      // internal::quat_product, generic path
                r[0] = aw * bw - ax * bx - ay * by - az * bz;
                r[1] = aw * bx + ax * bw + ay * bz - az * by;
                r[2] = aw * by + ay * bw + az * bx - ax * bz;
                r[3] = aw * bz + az * bw + ax * by - ay * bx;
#pragma unroll
                for (int i = 0; i < 4; i++) { rec[kRecDq + i] = q[i]; rec[kRecRq + i] = r[i]; }
                const double nrm = sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[0] * r[0]);      // delta_q_.normalize()
                q[1] = r[1] / nrm; q[2] = r[2] / nrm; q[3] = r[3] / nrm; q[0] = r[0] / nrm;
            }
        } else if (tid == 64 && predict) {      // processIMU, L/src/BackendFusion.cpp:815-821
            for (int k = 0; k < nc; k++) {
                const double* p = s_smp + k * kImuRow;
                const double* c = p + kImuRow;
                const double* rec = s_rec + k * kImuRec;
                const double dt = c[0];
                double v[3], u0[3], u1[3];
#pragma unroll
                for (int i = 0; i < 3; i++) v[i] = p[1 + i] - ba[i];
#pragma unroll
                for (int i = 0; i < 3; i++) u0[i] = ((pR[3 * i] * v[0] + pR[3 * i + 1] * v[1]) + pR[3 * i + 2] * v[2]) - g[i];
                const double hq[4] = {1.0, rec[kRecHalf], rec[kRecHalf + 1], rec[kRecHalf + 2]};      // deltaQ(un_gyr * dt)
                double M[9], Rn[9];
                quat_to_mat(hq, M);
                imu_mul(pR, M, Rn);
#pragma unroll
                for (int i = 0; i < 9; i++) pR[i] = Rn[i];
#pragma unroll
                for (int i = 0; i < 3; i++) v[i] = c[1 + i] - ba[i];
#pragma unroll
                for (int i = 0; i < 3; i++) u1[i] = ((pR[3 * i] * v[0] + pR[3 * i + 1] * v[1]) + pR[3 * i + 2] * v[2]) - g[i];
                const double hdd = 0.5 * dt * dt;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double ua = 0.5 * (u0[i] + u1[i]);
                    pP[i] = pP[i] + (dt * pV[i] + hdd * ua);
                    pV[i] = pV[i] + dt * ua;
                }
            }
        }
        __syncthreads();
        // ---- blocks
        if (tid < nc) imu_blocks(s_rec + tid * kImuRec, s_smp + tid * kImuRow, s_smp + (tid + 1) * kImuRow, ba, bg);
        __syncthreads();
        // ---- apply
        for (int k = 0; k < nc; k++) {
            const double* rec = s_rec + k * kImuRec;
            const double dt = rec[kRecDt];
            if (tid < 225) {
                const double* Jc = s_J[cur];
                double sa = 0.0, sj = 0.0;      // (F P)(i, j), (F J)(i, j)
#pragma unroll
                for (int t = 0; t < kImuFTerms; t++) { const double f = rec[fiOff[t]]; sa += f * s_P[fiX[t]]; sj += f * Jc[fiX[t]]; }
                s_A[tid] = sa;
                s_J[cur ^ 1][tid] = sj;
            } else if (tid == 255) {      // delta_p + delta_v dt + 0.5 un_acc dt dt;  delta_v + un_acc dt;  sum_dt += dt
#pragma unroll
                for (int i = 0; i < 3; i++) { dp[i] = dp[i] + dv[i] * dt + rec[kRecIncP + i]; dv[i] = dv[i] + rec[kRecIncV + i]; }
                sum_dt += dt;
            }
            __syncthreads();
            if (tid < 225) {
                double sb = 0.0, sq = 0.0;      // (A F^T)(i, j), (V N V^T)(i, j)
#pragma unroll
                for (int t = 0; t < kImuFTerms; t++) sb += s_A[fjA[t]] * rec[fjOff[t]];
#pragma unroll
                for (int c = 0; c < 12; c++) sq += (rec[viOff[c]] * nz[c / 3]) * rec[vjOff[c]];
                sq += (rec[vdOff] * nzd) * rec[vdOff];
                s_P[tid] = sb + sq;
            }
            cur ^= 1;
            __syncthreads();
        }
    }
    // ---- results
    if (tid < 225) { O.jacobian[tid] = s_J[cur][tid]; O.covariance[tid] = s_P[tid]; }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) O.delta_q[i] = q[i];
    }
    if (tid == 255) {
        O.sum_dt = sum_dt;
#pragma unroll
        for (int i = 0; i < 3; i++) { O.delta_p[i] = dp[i]; O.delta_v[i] = dv[i]; }
    }
    if (tid == 64) {
#pragma unroll
        for (int i = 0; i < 3; i++) { O.P1[i] = pP[i]; O.V1[i] = pV[i]; O.g[i] = S.g[i]; O.lin_ba[i] = ba[i]; O.lin_bg[i] = bg[i]; }
#pragma unroll
        for (int i = 0; i < 9; i++) O.R1[i] = pR[i];
    }
}

}  // namespace lili

extern "C" {

int lili_imu_preintegrate(lili_ctx* ctx, const lili_imu_segment* seg, int n_seg, lili_window_imu* out, lili_imu_prediction* pred) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(seg && out, "imu_preintegrate: null argument");
    ARGCHK(n_seg >= 1 && n_seg <= LILI_IMU_MAX_SEGMENTS, "imu_preintegrate: n_seg must be in 1 .. 64");
    size_t n_rows = 0;
    for (int s = 0; s < n_seg; s++) {
        const lili_imu_segment& g = seg[s];
        ARGCHK(g.n >= 0 && g.n <= LILI_IMU_MAX_SAMPLES, "imu_preintegrate: n must be in 0 .. 4096");
        ARGCHK(g.n == 0 || (g.dt && g.acc && g.gyr), "imu_preintegrate: null sample array");
        ARGCHK(!g.predict || pred, "imu_preintegrate: a segment predicts but pred is null");
        ARGCHK(finite_n(g.acc0, 3) && finite_n(g.gyr0, 3) && finite_n(g.lin_ba, 3) && finite_n(g.lin_bg, 3) && finite_n(g.g, 3), "imu_preintegrate: a constructor argument is not finite");
        ARGCHK(!g.predict || (finite_n(g.P0, 3) && finite_n(g.R0, 9) && finite_n(g.V0, 3)), "imu_preintegrate: a start state is not finite");
        ARGCHK(finite_n(g.dt, g.n) && finite_n(g.acc, 3 * (size_t)g.n) && finite_n(g.gyr, 3 * (size_t)g.n), "imu_preintegrate: a sample is not finite");
        for (int k = 0; k < g.n; k++) ARGCHK(g.dt[k] >= 0.0, "imu_preintegrate: negative dt");
        n_rows += (size_t)g.n + 1;
    }
    HIPCHK(hipSetDevice(ctx->device));
    StagedJob* B = ext_of<StagedJob>(ctx, lili_ctx::kExtImu);
    const size_t hdr_bytes = sizeof(ImuSegDev) * LILI_IMU_MAX_SEGMENTS, in_bytes = hdr_bytes + n_rows * kImuRow * sizeof(double), out_bytes = sizeof(ImuOutDev) * n_seg;
    TRY(B->size(ctx, in_bytes, sizeof(ImuOutDev) * LILI_IMU_MAX_SEGMENTS));
    // ---- pack: headers, then n + 1 rows per segment
    ImuSegDev* H = B->in.as<ImuSegDev>();
    double* R = reinterpret_cast<double*>(B->in.as<unsigned char>() + hdr_bytes);
    size_t row = 0;
    for (int s = 0; s < n_seg; s++) {
        const lili_imu_segment& g = seg[s];
        ImuSegDev& h = H[s];
        std::memset(&h, 0, sizeof h);
        h.first_row = (long long)row; h.n = g.n; h.predict = g.predict ? 1 : 0;
        std::memcpy(h.ba, g.lin_ba, sizeof h.ba); std::memcpy(h.bg, g.lin_bg, sizeof h.bg); std::memcpy(h.g, g.g, sizeof h.g);
        if (g.predict) { std::memcpy(h.P0, g.P0, sizeof h.P0); std::memcpy(h.R0, g.R0, sizeof h.R0); std::memcpy(h.V0, g.V0, sizeof h.V0); }
        double* r = R + row * kImuRow;
        r[0] = 0.0;
        for (int i = 0; i < 3; i++) { r[1 + i] = g.acc0[i]; r[4 + i] = g.gyr0[i]; }
        for (int k = 0; k < g.n; k++) {
            r += kImuRow;
            r[0] = g.dt[k];
            for (int i = 0; i < 3; i++) { r[1 + i] = g.acc[3 * k + i]; r[4 + i] = g.gyr[3 * k + i]; }
        }
        row += (size_t)g.n + 1;
    }
    TRY(B->run(ctx, ctx->imu_time, in_bytes, out_bytes, [&] {
        hipLaunchKernelGGL(k_imu_preintegrate, dim3(n_seg), dim3(kImuThreads), 0, ctx->stream, B->d_in.as<ImuSegDev>(),
                           reinterpret_cast<const double*>(B->d_in.as<unsigned char>() + hdr_bytes), B->d_out.as<ImuOutDev>());
    }));
    const ImuOutDev* o = B->out.as<ImuOutDev>();
    for (int s = 0; s < n_seg; s++) {
        std::memcpy(&out[s], &o[s], sizeof(lili_window_imu));
        if (seg[s].predict) std::memcpy(&pred[s], o[s].P1, sizeof(lili_imu_prediction));
    }
    return LILI_OK;
}

int lili_imu_kernel_ms(lili_ctx* ctx, float* ms) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(ms, "imu_kernel_ms: null argument");
    const StagedJob* B = static_cast<const StagedJob*>(ctx->ext[lili_ctx::kExtImu].get());
    if (!B || B->last_ms < 0.f) return ctx->fail(LILI_E_STATE, "imu_kernel_ms: no timed lili_imu_preintegrate yet (option imu_time)");
    *ms = B->last_ms;
    return LILI_OK;
}

}  // extern "C"
