// The joint keyframe window on the device (include/lili_hip.h: lili_window_*): what ceres::Solve gets in optimizeSlidingWindowWithLandMark
// (L/src/BackendFusion.cpp:843-1007) — n_kf keyframes x (t, q, speed-bias), the lidar blocks of every keyframe, the IMU factors between consecutive
// keyframes (ImuFactor.h:18-144), the marginalisation prior (MarginalizationFactor.cpp:233-286) or the speed-bias priors (PriorFactor.h:13-23).
//
//   lili_window_evaluate   cost, gradient and J^T J in local coordinates at one state: the lidar part is the per-slot Gram of lili_s2m_linearize_window
//                          (same launches, same fixed-order reduction), k_window_evaluate (ONE wave) projects it to local coordinates and adds the
//                          O(1) factors in f64 (win_build).
//   lili_window_solve      Ceres' trust-region loop as lili_s2m_lm.hip restates it, on 15 n_kf local dimensions, ONE persistent launch: the workgroups
//                          of slot k evaluate that keyframe's records at the candidate (lin_surf_body / lin_edge_body, partials published as keyed
//                          granules), wave 0 of EVERY workgroup gathers the partials of ALL slots in index order (<= kWinGroup workgroups per slot: one
//                          hop), runs win_build, takes the accept / reject decision and proposes the next candidate from a Cholesky factorisation of
//                          the Jacobi-scaled J^T J + D^2 / radius in LDS — the same instructions on the same bits in every workgroup, so no decision
//                          is broadcast.  Partial buffers are double-buffered by the evaluation's parity as in k_solve_lm; every wait is bounded
//                          (xchg_gather) and ends the launch with LILI_LM_STALLED.
//
//   lili_window_marginalize  the NEXT window's prior (MarginalizationInfo::PreMarginalize + Marginalize, L/src/BackendFusion.cpp:1009-1184): the lidar launches of
//                          lili_window_evaluate, then k_window_marg (ONE workgroup): win_build<true> forms the reference's factor set with the "last three columns"
//                          convention, marg_schur takes the Schur complement over keyframe 0 and the square-root form through two Jacobi eigen-decompositions
//                          in LDS.  lili_marg_schur uploads a host system into the same kernel.
//
// The factors are restated from the semantics SURVEY records; the checker's restatement (tests/test_window_solve_gpu.py) is the referee.
#include "lili_solve_dev.h"
#include "lili_launch.h"

#include <cmath>
#include <cstddef>
#include <cstring>

namespace lili {

constexpr int kWinMaxKf = LILI_WINDOW_MAX_KF, kWinMaxN = 15 * kWinMaxKf, kWinMaxBlocks = 3 * kWinMaxKf;
constexpr int kWinThreads = kLmThreads;      // k_solve_lm's workgroup, for its reason: 8 waves, the launch may use 256 VGPRs per lane
constexpr int kWinGroup = 16;         // workgroups per slot at most: every slot's partials are gathered in ONE hop

struct WinImuDev {
    double sum_dt, g[3], dp[3], dq[4], dv[3], ba[3], bg[3];
    double dp_dba[9], dp_dbg[9], dq_dbg[9], dv_dba[9], dv_dbg[9];      // blocks of the pre-integration's Jacobian
    double sqrt_info[225];
};
struct WinDev {      // the problem as the kernels read it (one upload per call)
    int n_kf, n_imu, has_prior, n_rows, n_cols, n_blocks, pad0_, pad1_;
    int blk_kind[kWinMaxBlocks], blk_kf[kWinMaxBlocks], blk_col[kWinMaxBlocks] /* first column in J0 */, blk_x0[kWinMaxBlocks] /* offset in x0 */;
    int col_blk[kWinMaxN];      // block of every column of J0
    int sb_has[kWinMaxKf];
    double sb_mean[9 * kWinMaxKf];
    double state[16 * kWinMaxKf];
    double x0[16 * kWinMaxKf];
    double r0[kWinMaxN];
    double J0[kWinMaxN * kWinMaxN];      // n_rows x n_cols, tight
    double A0[kWinMaxN * kWinMaxN];      // J0^T J0, n_cols x n_cols (host, once per call)
    WinImuDev imu[kWinMaxKf - 1];
};

// one evaluation of the window in LDS: inputs x and lid, outputs H, g, cost; the rest is scratch of win_build
struct WinSys {
    double H[kWinMaxN * kWinMaxN];      // N x N, N = 15 n_kf
    double g[kWinMaxN];
    double cost;
    double x[kWinMaxKf][16];            // t, q, speed-bias per keyframe
    double lid[kWinMaxKf][72];          // per keyframe: the 8x8 lidar Gram (rows J0..J6, r), [64] = its robust cost
    double Jraw[kWinMaxKf - 1][15][31]; // IMU factors: un-whitened local Jacobian (30 columns: keyframe i, keyframe j) and residual (column 30)
    double Jw[15][31];                  // one factor, whitened
    double pr[kWinMaxN], dx[kWinMaxN], pv[kWinMaxN];
    double T[kWinMaxBlocks][9];         // prior, quaternion blocks: d dx / d local (3x3)
};

__device__ __forceinline__ dq qnormalized(dq q) {
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return {q.w / n, q.x / n, q.y / n, q.z / n};
}
// rows 1..3 of Qleft(q) (math_tools.h): [v | w I + [v]x]
__device__ __forceinline__ void qleft_rows(dq q, double m[3][4]) {
    m[0][0] = q.x; m[0][1] = q.w; m[0][2] = -q.z; m[0][3] = q.y;
    m[1][0] = q.y; m[1][1] = q.z; m[1][2] = q.w; m[1][3] = -q.x;
    m[2][0] = q.z; m[2][1] = -q.y; m[2][2] = q.x; m[2][3] = q.w;
}
// ceres::QuaternionParameterization::ComputeJacobian (4x3)
__device__ __forceinline__ void plus_jac(const double* q, double m[4][3]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    m[0][0] = -x; m[0][1] = -y; m[0][2] = -z;
    m[1][0] = w; m[1][1] = z; m[1][2] = -y;
    m[2][0] = -z; m[2][1] = w; m[2][2] = x;
    m[3][0] = y; m[3][1] = -x; m[3][2] = w;
}
__device__ __forceinline__ d3 m3v(const double* m, d3 v) {
    return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z};
}
__device__ __forceinline__ double d3c(d3 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : v.z; }

// ImuFactor::Evaluate of ONE factor by ONE lane, un-whitened, Jacobians in local coordinates: J[15][31] (zeroed by the caller), column 30 = residual.
// kLast3: the quaternion blocks enter by the last three of their four global columns (MarginalizationFactor.cpp:9-17) instead of through Ceres' plus-Jacobian
template <bool kLast3, int kWho = 0>
__device__ __noinline__ void win_imu_raw(const WinImuDev& f, const double* xi, const double* xj, double (*J)[31]) {
    const d3 Pi{xi[0], xi[1], xi[2]}, Pj{xj[0], xj[1], xj[2]};
    const dq Qi = qnormalized(dq{xi[3], xi[4], xi[5], xi[6]}), Qj = qnormalized(dq{xj[3], xj[4], xj[5], xj[6]});
    const d3 Vi{xi[7], xi[8], xi[9]}, Bai{xi[10], xi[11], xi[12]}, Bgi{xi[13], xi[14], xi[15]};
    const d3 Vj{xj[7], xj[8], xj[9]}, Baj{xj[10], xj[11], xj[12]}, Bgj{xj[13], xj[14], xj[15]};
    const d3 g{f.g[0], f.g[1], f.g[2]};
    const double s = f.sum_dt;
    const d3 dba = Bai - d3{f.ba[0], f.ba[1], f.ba[2]}, dbg = Bgi - d3{f.bg[0], f.bg[1], f.bg[2]};
    const d3 th = m3v(f.dq_dbg, dbg);
    const dq cq = qmul(dq{f.dq[0], f.dq[1], f.dq[2], f.dq[3]}, dq{1.0, 0.5 * th.x, 0.5 * th.y, 0.5 * th.z});
    const d3 cv = (d3{f.dv[0], f.dv[1], f.dv[2]} + m3v(f.dv_dba, dba)) + m3v(f.dv_dbg, dbg);
    const d3 cp = (d3{f.dp[0], f.dp[1], f.dp[2]} + m3v(f.dp_dba, dba)) + m3v(f.dp_dbg, dbg);
    const dq Qi_inv = qinv(Qi);
    const d3 tmp = (((-0.5 * s * s) * g + Pj) - Pi) - s * Vi;
    const d3 tmp1 = ((-s) * g + Vj) - Vi;
    const d3 rp = qrot(Qi_inv, tmp) - cp;
    const dq rq = qnormalized(qmul(qinv(cq), qmul(Qi_inv, Qj)));
    const d3 rv = qrot(Qi_inv, tmp1) - cv;
    const d3 rba = Baj - Bai, rbg = Bgj - Bgi;
    for (int i = 0; i < 3; i++) {
        J[i][30] = d3c(rp, i); J[3 + i][30] = 2.0 * (i == 0 ? rq.x : i == 1 ? rq.y : rq.z); J[6 + i][30] = d3c(rv, i);
        J[9 + i][30] = d3c(rba, i); J[12 + i][30] = d3c(rbg, i);
    }
    const double qi[4] = {Qi_inv.w, Qi_inv.x, Qi_inv.y, Qi_inv.z};
    double Ri[9];
    quat_to_mat(qi, Ri);
    double Pq_i[4][3], Pq_j[4][3];
    plus_jac(xi + 3, Pq_i);
    plus_jac(xj + 3, Pq_j);
    const d3 u{Qi.x, Qi.y, Qi.z};
    // d(Qi^-1 v) / d(w | x y z) as the reference writes it (ImuFactor.h:63-64, 71-72), times the plus-Jacobian of Qi: rows r0.., local columns 3..5
    auto dq_block = [&](d3 v, int r0) {
        const d3 uxv = cross3(u, v);
        const double uv = dot3(u, v);
        double m[3][4];
        for (int i = 0; i < 3; i++) {
            m[i][0] = 2.0 * (Qi.w * d3c(v, i) + d3c(uxv, i));
            for (int c = 0; c < 3; c++) {
                // u.v I + u v^T - v u^T - w [v]x
                const double sk = (i == c) ? 0.0 : ((c == (i + 1) % 3) ? -d3c(v, 3 - i - c) : d3c(v, 3 - i - c));
                m[i][1 + c] = 2.0 * ((((i == c ? uv : 0.0) + d3c(u, i) * d3c(v, c)) - d3c(v, i) * d3c(u, c)) - Qi.w * sk);
            }
        }
        for (int i = 0; i < 3; i++) for (int c = 0; c < 3; c++) {
            if constexpr (kLast3) J[r0 + i][3 + c] = m[i][1 + c];
            else J[r0 + i][3 + c] = ((m[i][0] * Pq_i[0][c] + m[i][1] * Pq_i[1][c]) + m[i][2] * Pq_i[2][c]) + m[i][3] * Pq_i[3][c];
        }
    };
    dq_block(tmp, 0);
    dq_block(tmp1, 6);
    for (int i = 0; i < 3; i++) for (int c = 0; c < 3; c++) {
        J[i][c] = -Ri[3 * i + c];                    // d r_p / d Pi
        J[i][6 + c] = -Ri[3 * i + c] * s;            // d r_p / d Vi
        J[i][9 + c] = -f.dp_dba[3 * i + c];
        J[i][12 + c] = -f.dp_dbg[3 * i + c];
        J[6 + i][6 + c] = -Ri[3 * i + c];            // d r_v / d Vi
        J[6 + i][9 + c] = -f.dv_dba[3 * i + c];
        J[6 + i][12 + c] = -f.dv_dbg[3 * i + c];
        J[9 + i][9 + c] = i == c ? -1.0 : 0.0;
        J[12 + i][12 + c] = i == c ? -1.0 : 0.0;
        J[i][15 + c] = Ri[3 * i + c];                // d r_p / d Pj
        J[6 + i][21 + c] = Ri[3 * i + c];            // d r_v / d Vj
        J[9 + i][24 + c] = i == c ? 1.0 : 0.0;
        J[12 + i][27 + c] = i == c ? 1.0 : 0.0;
    }
    {   // d r_q / d Qi = -2 (Qleft(Qj^-1) Qright(cq)) rows 1..3, times the plus-Jacobian of Qi
        double L[3][4];
        qleft_rows(qinv(Qj), L);
        // Qright(p): [p0, -pv^T; pv, p0 I - [pv]x]
        const double R[4][4] = {{cq.w, -cq.x, -cq.y, -cq.z}, {cq.x, cq.w, cq.z, -cq.y}, {cq.y, -cq.z, cq.w, cq.x}, {cq.z, cq.y, -cq.x, cq.w}};
        for (int i = 0; i < 3; i++) {
            double m[4];
            for (int c = 0; c < 4; c++) m[c] = -2.0 * (((L[i][0] * R[0][c] + L[i][1] * R[1][c]) + L[i][2] * R[2][c]) + L[i][3] * R[3][c]);
            for (int c = 0; c < 3; c++) {
                if constexpr (kLast3) J[3 + i][3 + c] = m[1 + c];
                else J[3 + i][3 + c] = ((m[0] * Pq_i[0][c] + m[1] * Pq_i[1][c]) + m[2] * Pq_i[2][c]) + m[3] * Pq_i[3][c];
            }
        }
    }
    {   // d r_q / d Bgi = -LeftQuatMatrix(Qj^-1 Qi cq)[0:3, 0:3] dq_dbg,  [0:3, 0:3] = w I + [v]x
        const dq a = qmul(qmul(qinv(Qj), Qi), cq);
        const double M[3][3] = {{a.w, -a.z, a.y}, {a.z, a.w, -a.x}, {-a.y, a.x, a.w}};
        for (int i = 0; i < 3; i++) for (int c = 0; c < 3; c++)
            J[3 + i][12 + c] = -((M[i][0] * f.dq_dbg[c] + M[i][1] * f.dq_dbg[3 + c]) + M[i][2] * f.dq_dbg[6 + c]);
    }
    {   // d r_q / d Qj = 2 Qleft(cq^-1 Qi^-1) rows 1..3, times the plus-Jacobian of Qj
        double L[3][4];
        qleft_rows(qmul(qinv(cq), Qi_inv), L);
        for (int i = 0; i < 3; i++) for (int c = 0; c < 3; c++) {
            if constexpr (kLast3) J[3 + i][18 + c] = 2.0 * L[i][1 + c];
            else J[3 + i][18 + c] = 2.0 * (((L[i][0] * Pq_j[0][c] + L[i][1] * Pq_j[1][c]) + L[i][2] * Pq_j[2][c]) + L[i][3] * Pq_j[3][c]);
        }
    }
}

// MarginalizationFactor::Evaluate, block b by ONE lane: dx of the block, and for a quaternion block T = +-2 Qleft(q0^-1)[1:4, :] * plus(q) — the reference's own
// Jacobian of dx in global columns times Ceres' plus-Jacobian, not the derivative of the normalised expression.  kLast3: the last three of those four
// global columns instead (what MarginalizationInfo takes of every quaternion block)
template <bool kLast3, int kWho = 0>
__device__ __noinline__ void win_prior_block(const WinDev* pb, WinSys& s, int b) {
    const int kind = pb->blk_kind[b], kf = pb->blk_kf[b], col = pb->blk_col[b];
    const double* x0 = pb->x0 + pb->blk_x0[b];
    if (kind == 0) { for (int i = 0; i < 3; i++) s.dx[col + i] = s.x[kf][i] - x0[i]; }
    else if (kind == 2) { for (int i = 0; i < 9; i++) s.dx[col + i] = s.x[kf][7 + i] - x0[i]; }
    else {
        const dq q0i = qinv(dq{x0[0], x0[1], x0[2], x0[3]});
        const dq d = qmul(q0i, dq{s.x[kf][3], s.x[kf][4], s.x[kf][5], s.x[kf][6]});
        const double sg = d.w >= 0.0 ? 2.0 : -2.0;
        const dq n = qnormalized(d);
        s.dx[col] = sg * n.x; s.dx[col + 1] = sg * n.y; s.dx[col + 2] = sg * n.z;
        double L[3][4], Pq[4][3];
        qleft_rows(q0i, L);
        plus_jac(&s.x[kf][3], Pq);
        for (int i = 0; i < 3; i++) for (int c = 0; c < 3; c++) {
            if constexpr (kLast3) s.T[b][3 * i + c] = sg * L[i][1 + c];
            else s.T[b][3 * i + c] = sg * (((L[i][0] * Pq[0][c] + L[i][1] * Pq[1][c]) + L[i][2] * Pq[2][c]) + L[i][3] * Pq[3][c]);
        }
    }
}
__device__ __forceinline__ int win_blk_local(const WinDev* pb, int b) { return 15 * pb->blk_kf[b] + (pb->blk_kind[b] == 0 ? 0 : pb->blk_kind[b] == 1 ? 3 : 6); }

// The local system of the window at s.x by ONE wave (all 64 lanes call it, control flow uniform): s.H = J^T J, s.g = J^T r, s.cost.  Every sum runs in a
// fixed order, so every workgroup of the solve holds the same bits.
// kMarg: the system MarginalizationInfo::PreMarginalize + ThreadsConstructA form at s.x instead (L/src/BackendFusion.cpp:1009-1165) — every quaternion block by the
// last three of its four global columns, and of the IMU factors only the one between keyframes 0 and 1; s.cost is then without meaning.
// kWho: whose copy this is (0: the kernels up to k_window_marg, 1: k_window_marg_cycle's own — see there); it changes nothing in the code
template <bool kMarg, int kWho = 0>
__device__ __noinline__ void win_build(const WinDev* __restrict__ pb, WinSys& s) {
    const int lane = threadIdx.x & 63;
    const int n_kf = pb->n_kf, N = 15 * n_kf, n_imu = kMarg ? (pb->n_imu < 1 ? pb->n_imu : 1) : pb->n_imu;
    for (int e = lane; e < N * N; e += 64) s.H[e] = 0.0;
    if (lane < N) s.g[lane] = 0.0;
    for (int e = lane; e < n_imu * 15 * 31; e += 64) (&s.Jraw[0][0][0])[e] = 0.0;
    LILI_WAVE_SYNC();
    double cost = 0.0;      // lane 0's is the one that counts
    // ---- lidar: H_kk = P^T G77 P, g_k = P^T G7r with P = diag(I3, plus-Jacobian(q_k)) (pose_local_entry)
    for (int k = 0; k < n_kf; k++) {
        const double* gram = s.lid[k];
        if (lane < 42) {
            const int a = lane < 36 ? lane / 6 : lane - 36, b = lane < 36 ? lane % 6 : 7;
            double v;
            if constexpr (kMarg) v = gram[(a < 3 ? a : a + 1) * 8 + (b < 3 || b == 7 ? b : b + 1)];      // rows / columns {0,1,2}, {4,5,6} and column 7, as lili_marg_add_lidar takes them
            else v = pose_local_entry(gram, s.x[k] + 3, a, b);
            if (lane < 36) s.H[(15 * k + a) * N + 15 * k + b] = v; else s.g[15 * k + a] = v;
        }
        cost += gram[64];
    }
    // ---- speed-bias priors: r = 15 (sb - mean), J = 15 I
    if (lane < 9 * n_kf) {
        const int k = lane / 9, i = lane - 9 * k;
        double r = 0.0;
        if (pb->sb_has[k]) {
            r = 15.0 * (s.x[k][7 + i] - pb->sb_mean[9 * k + i]);
            const int c = 15 * k + 6 + i;
            s.H[c * N + c] = 225.0;
            s.g[c] = 15.0 * r;
        }
        s.pr[lane] = r;
    }
    // ---- IMU factors, raw: one lane per factor
    if (lane < n_imu) win_imu_raw<kMarg, kWho>(pb->imu[lane], s.x[lane], s.x[lane + 1], s.Jraw[lane]);
    LILI_WAVE_SYNC();
    {
        double c = 0.0;
        for (int i = 0; i < 9 * n_kf; i++) c += s.pr[i] * s.pr[i];
        cost += 0.5 * c;
    }
    for (int f = 0; f < n_imu; f++) {
        const double* S = pb->imu[f].sqrt_info;
        LILI_WAVE_SYNC();
        for (int e = lane; e < 15 * 31; e += 64) {
            const int i = e / 31, c = e - 31 * i;
            double v = 0.0;
            for (int j = 0; j < 15; j++) v += S[15 * i + j] * s.Jraw[f][j][c];
            s.Jw[i][c] = v;
        }
        LILI_WAVE_SYNC();
        for (int e = lane; e < 900; e += 64) {
            const int a = e / 30, b = e - 30 * a;
            double v = 0.0;
            for (int i = 0; i < 15; i++) v += s.Jw[i][a] * s.Jw[i][b];
            s.H[(15 * f + a) * N + 15 * f + b] += v;
        }
        if (lane < 30) {
            double v = 0.0;
            for (int i = 0; i < 15; i++) v += s.Jw[i][lane] * s.Jw[i][30];
            s.g[15 * f + lane] += v;
        }
        double c = 0.0;
        for (int i = 0; i < 15; i++) c += s.Jw[i][30] * s.Jw[i][30];
        cost += 0.5 * c;
    }
    // ---- marginalisation prior: r = r0 + J0 dx; H += T^T (J0^T J0) T, g += T^T J0^T r
    if (pb->has_prior) {
        const int n_rows = pb->n_rows, n_cols = pb->n_cols, n_blocks = pb->n_blocks;
        LILI_WAVE_SYNC();
        if (lane < n_blocks) win_prior_block<kMarg, kWho>(pb, s, lane);
        LILI_WAVE_SYNC();
        if (lane < n_rows) {
            double r = pb->r0[lane];
            for (int c = 0; c < n_cols; c++) r += pb->J0[lane * n_cols + c] * s.dx[c];
            s.pr[lane] = r;
        }
        LILI_WAVE_SYNC();
        if (lane < n_cols) {
            double v = 0.0;
            for (int r = 0; r < n_rows; r++) v += pb->J0[r * n_cols + lane] * s.pr[r];
            s.pv[lane] = v;
        }
        LILI_WAVE_SYNC();
        if (lane < n_cols) {
            const int b = pb->col_blk[lane], a = lane - pb->blk_col[b];
            double v = s.pv[lane];
            if (pb->blk_kind[b] == 1) { const int c0 = pb->blk_col[b]; v = (s.T[b][a] * s.pv[c0] + s.T[b][3 + a] * s.pv[c0 + 1]) + s.T[b][6 + a] * s.pv[c0 + 2]; }
            s.g[win_blk_local(pb, b) + a] += v;
        }
        for (int e = lane; e < n_cols * n_cols; e += 64) {
            const int ca = e / n_cols, cb = e - n_cols * ca;
            const int ba = pb->col_blk[ca], bb = pb->col_blk[cb];
            const int ia = ca - pb->blk_col[ba], ib = cb - pb->blk_col[bb];
            const bool qa = pb->blk_kind[ba] == 1, qb = pb->blk_kind[bb] == 1;
            double v = 0.0;
            for (int i = 0; i < (qa ? 3 : 1); i++) {
                const int ra = qa ? pb->blk_col[ba] + i : ca;
                const double wa = qa ? s.T[ba][3 * i + ia] : 1.0;
                double row = 0.0;
                for (int j = 0; j < (qb ? 3 : 1); j++) {
                    const int rb = qb ? pb->blk_col[bb] + j : cb;
                    row += pb->A0[ra * n_cols + rb] * (qb ? s.T[bb][3 * j + ib] : 1.0);
                }
                v += wa * row;
            }
            s.H[(win_blk_local(pb, ba) + ia) * N + win_blk_local(pb, bb) + ib] += v;
        }
        double c = 0.0;
        for (int r = 0; r < n_rows; r++) c += s.pr[r] * s.pr[r];
        cost += 0.5 * c;
    }
    if (lane == 0) s.cost = cost;
    LILI_WAVE_SYNC();
}

// lili_window_evaluate: one workgroup of one wave.  rec: n_kf lidar records of k_window_reduce (64 Gram + cost + counts) or nullptr; out: cost, g[N], H[N * N]
__global__ __launch_bounds__(64) void k_window_evaluate(const WinDev* __restrict__ pb, const double* __restrict__ rec, double* __restrict__ out, int want_h) {
    __shared__ WinSys s;
    const int lane = threadIdx.x;
    const int n_kf = pb->n_kf, N = 15 * n_kf;
    for (int e = lane; e < 16 * n_kf; e += 64) s.x[e / 16][e % 16] = pb->state[e];
    for (int e = lane; e < 72 * n_kf; e += 64) s.lid[e / 72][e % 72] = rec ? rec[e] : 0.0;
    LILI_WAVE_SYNC();
    win_build<false>(pb, s);
    if (lane == 0) out[0] = s.cost;
    if (lane < N) out[1 + lane] = s.g[lane];
    if (want_h) for (int e = lane; e < N * N; e += 64) out[1 + N + e] = s.H[e];
}

struct WinSolveArgs {
    LmArgs a[kWinMaxKf];
    int first_block[kWinMaxKf];
    int n;
    const WinDev* prob;
    double* state_out;             // n x 16 doubles
    lili_lm_summary* summary;
};
struct WinShared {
    WinSys sys;                    // the candidate: sys.x is what the workgroups evaluate next; sys.H doubles as the work matrix of the Cholesky factorisation
    double H[kWinMaxN * kWinMaxN], g[kWinMaxN];      // the system at the accepted point
    double scale[kWinMaxN], d[kWinMaxN], tr[kWinMaxN];
    double x[kWinMaxKf][16];       // accepted point
    double vals[kWinGroup][40];
    double tot[kWinMaxKf][40];
    LmTrust t;                     // trust-region state and options (those of W.a[0])
    int counts[2];
};

// The trust-region step from the accepted point by ONE wave (lm_propose of lili_s2m_lm.hip on N dimensions, the same LmTrust bookkeeping): returns with sh.t.go = 1 and
// sh.sys.x = candidate, or sh.t.go = 0.  (H_s + D^2) d = -g_s by a left-looking Cholesky factorisation, lane = row; a non-positive pivot is an INVALID step like a model that does
// not descend (radius halved, five in a row end the solve with LILI_LM_NUMERICAL_FAILURE).
__device__ __noinline__ void win_propose(WinShared& sh, const int n_kf) {
    const int lane = threadIdx.x & 63;
    const int N = 15 * n_kf;
    const bool in = lane < N;
    double* A = sh.sys.H;
    LmTrust& t = sh.t;
    for (;;) {
        const int it = t.it;
        double gmax = 0.0;
        for (int i = 0; i < N; i++) gmax = fmax(gmax, fabs(sh.g[i]));
        if (!lm_trust_gate(t, gmax, lane)) return;
        const double radius = t.radius;
        for (int e = lane; e < N * N; e += 64) {
            const int i = e / N, j = e - N * i;
            double v = sh.H[e] * sh.scale[i] * sh.scale[j];
            if (i == j) v += fmin(fmax(v, t.min_lm_diagonal), t.max_lm_diagonal) / radius;      // D^2 = clamp(diag H_s) / radius
            A[e] = v;
        }
        LILI_WAVE_SYNC();
        bool okc = true;
        for (int j = 0; j < N; j++) {
            double acc = 0.0;
            if (in && lane >= j) {
                acc = A[lane * N + j];
                for (int k = 0; k < j; k++) acc -= A[lane * N + k] * A[j * N + k];
            }
            const double piv = __shfl(acc, j);
            okc = okc && (piv > 0.0);
            const double l = sqrt(piv);
            if (in && lane >= j) A[lane * N + j] = lane == j ? l : acc / l;
            LILI_WAVE_SYNC();
        }
        double bv = in ? -(sh.g[lane] * sh.scale[lane]) : 0.0;
        for (int j = 0; j < N; j++) {                // L y = -g_s
            const double yj = __shfl(bv, j) / A[j * N + j];
            if (lane == j) bv = yj; else if (in && lane > j) bv -= A[lane * N + j] * yj;
        }
        for (int j = N - 1; j >= 0; j--) {           // L^T d = y
            const double dj = __shfl(bv, j) / A[j * N + j];
            if (lane == j) bv = dj; else if (lane < j) bv -= A[j * N + lane] * dj;
        }
        okc = okc && __all(bv == bv);
        if (in) sh.d[lane] = bv;
        LILI_WAVE_SYNC();
        // model_cost_change = -d^T (g_s + H_s d / 2)
        if (in) {
            double hd = 0.0;
            for (int j = 0; j < N; j++) hd += (sh.H[lane * N + j] * sh.scale[lane] * sh.scale[j]) * sh.d[j];
            sh.tr[lane] = bv * (sh.g[lane] * sh.scale[lane] + 0.5 * hd);
        }
        LILI_WAVE_SYNC();
        double mc = 0.0;
        for (int i = 0; i < N; i++) mc += sh.tr[i];
        mc = -mc;
        if (!okc || !(mc > 0.0)) {
            if (!lm_trust_invalid(t, radius, it, lane)) return;
            continue;
        }
        if (in) sh.d[lane] = bv * sh.scale[lane];          // delta in the unscaled local coordinates
        LILI_WAVE_SYNC();
        if (lane < n_kf) {                                  // x (+) delta of keyframe `lane`
            const double* d = sh.d + 15 * lane;
            const double* x = sh.x[lane];
            double* xn = sh.sys.x[lane];
            for (int i = 0; i < 3; i++) xn[i] = x[i] + d[i];
            for (int i = 0; i < 9; i++) xn[7 + i] = x[7 + i] + d[6 + i];
            quat_plus(x + 3, d + 3, xn + 3, sinc_cos_halving);
        }
        if (lane == 0) {
            double n2 = 0.0;
            for (int i = 0; i < N; i++) n2 += sh.d[i] * sh.d[i];
            t.model_change = mc; t.n_invalid = 0; t.step_norm = sqrt(n2);
            t.go = 1;
        }
        return;
    }
}

// persistent launch: workgroup bid belongs to the last slot whose first_block <= bid; dynamic LDS = kWinThreads * kRow doubles (Gram staging rows)
__global__ __launch_bounds__(kWinThreads) void k_window_solve(WinSolveArgs W, MatchParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ WinShared sh;
    const int bid = (int)blockIdx.x;
    int slot = 0;
#pragma unroll
    for (int k = 1; k < kWinMaxKf; k++) if (k < W.n && bid >= W.first_block[k]) slot = k;
    const LmArgs& a = W.a[slot];
    const int b = bid - W.first_block[slot];
    const WinDev* pb = W.prob;
    const int n_kf = W.n, N = 15 * n_kf;
    const bool surf = b < a.S.nb;
    const bool wave0 = threadIdx.x < 64;
    const bool boss = bid == 0 && threadIdx.x == 0;
    {
        const int n_s = (a.S.n_q > 0 && a.S.block_counts) ? sum_block_counts(a.S.block_counts, a.S.n_bc) : 0;
        __syncthreads();
        const int n_e = (a.E.n_q > 0 && a.E.block_counts) ? sum_block_counts(a.E.block_counts, a.E.n_bc) : 0;
        for (int e = threadIdx.x; e < 16 * n_kf; e += blockDim.x) { sh.x[e / 16][e % 16] = pb->state[e]; sh.sys.x[e / 16][e % 16] = pb->state[e]; }
        if (threadIdx.x == 0) {
            sh.counts[0] = n_s; sh.counts[1] = n_e;
            lm_trust_init(sh.t, W.a[0]);
        }
        __syncthreads();
    }
    LinArgs S = a.S, E = a.E;
    S.block_counts = nullptr; E.block_counts = nullptr;         // the bodies then take N from n_global (= sh.counts)
    int n_log = 0;
    double cost0 = 0.0;
    for (int eval = 0;; eval++) {
        const int par = eval & 1;
        const unsigned long long key = xchg_key(W.a[0].launch, eval);
        double* part = a.part + (size_t)par * a.nb * kPartialStride;
        PoseArg pa{};
        for (int i = 0; i < 3; i++) pa.t[i] = sh.sys.x[slot][i];
        for (int i = 0; i < 4; i++) pa.q[i] = sh.sys.x[slot][3 + i];
        pa.state = nullptr; pa.derive_assoc = 0;
        // ---- this workgroup's share of its keyframe's records at the candidate, published as granules
        S.partials = part; E.partials = part + (size_t)a.S.nb * kPartialStride;
        if (surf) lin_surf_body(S, b, pa, P, a.state, sh.counts, lds, key);
        else lin_edge_body(E, b - a.S.nb, pa, P, a.state, sh.counts, lds, key);
        if (wave0) {
            // ---- exchange: the partials of EVERY slot, slot by slot, each in index order
            bool ok = true;
            for (int k = 0; k < n_kf; k++)
                ok = xchg_gather<40>(W.a[k].part + (size_t)par * W.a[k].nb * kPartialStride, W.a[k].nb, key, sh.vals, sh.tot[k]) && ok;
            if (!ok && threadIdx.x == 0) sh.t.stalled = 1;
            for (int k = 0; k < n_kf; k++) {
                gram_tri_to_full(sh.tot[k], sh.sys.lid[k]);
                if (threadIdx.x == 0) sh.sys.lid[k][64] = sh.tot[k][36];
            }
            LILI_WAVE_SYNC();
            win_build<false>(pb, sh.sys);
            // ---- step logic, identical in every workgroup
            if (eval == 0) {
                for (int e = threadIdx.x; e < N * N; e += 64) sh.H[e] = sh.sys.H[e];
                if (threadIdx.x < N) { sh.g[threadIdx.x] = sh.sys.g[threadIdx.x]; sh.scale[threadIdx.x] = 1.0 / (1.0 + sqrt(sh.sys.H[threadIdx.x * N + threadIdx.x])); }      // Jacobi scaling, kept for the whole solve
                if (threadIdx.x == 0) { sh.t.cost = sh.sys.cost; cost0 = sh.t.cost; if (sh.t.stalled) { sh.t.term = LILI_LM_STALLED; sh.t.go = 0; } }
            } else {
                if (threadIdx.x == 0) {
                    double xn2 = 0.0;
                    for (int k = 0; k < n_kf; k++) for (int i = 0; i < 16; i++) xn2 += sh.x[k][i] * sh.x[k][i];
                    lm_trust_judge(sh.t, sh.sys.cost, sqrt(xn2), W.summary, n_log, boss);
                }
                LILI_WAVE_SYNC();
                if (sh.t.take) {
                    for (int e = threadIdx.x; e < N * N; e += 64) sh.H[e] = sh.sys.H[e];
                    if (threadIdx.x < N) sh.g[threadIdx.x] = sh.sys.g[threadIdx.x];
                    for (int e = threadIdx.x; e < 16 * n_kf; e += 64) sh.x[e / 16][e % 16] = sh.sys.x[e / 16][e % 16];
                }
            }
            LILI_WAVE_SYNC();
            if (sh.t.go) win_propose(sh, n_kf);      // the next candidate (or the end), from the accepted point
            LILI_WAVE_SYNC();
        }
        __syncthreads();
        if (!sh.t.go) break;
    }
    if (bid == 0 && threadIdx.x < 64) {
        const int lane = threadIdx.x;
        for (int e = lane; e < 16 * n_kf; e += 64) W.state_out[e] = sh.x[e / 16][e % 16];
        if (lane < n_kf) {
            SlotState* st = W.a[lane].state;
            for (int i = 0; i < 7; i++) st->pose[i] = sh.x[lane][i];
            st->gn_status = (sh.t.term == LILI_LM_STALLED || sh.t.term == LILI_LM_NUMERICAL_FAILURE) ? 1 : 0;
            st->iters += sh.t.n_ok;
        }
        if (lane == 0 && W.summary) lm_write_summary(W.summary, sh.t, cost0, n_log, sh.counts);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The window's next prior (include/lili_hip.h: lili_marg_schur, lili_window_marginalize): MarginalizationInfo::Marginalize
// (L/src/MarginalizationFactor.cpp:176-201) in f64 by ONE workgroup — no other workgroup exists, nothing is waited for, every loop is bounded.
//   k_window_marg   wave 0 forms the system of the reference's factor set at the solved state (win_build<true>) and the workgroup picks the touched columns,
//                   or the workgroup loads a system the host uploaded (lili_marg_schur); then marg_schur: Amm = (Amm + Amm^T) / 2, its eigen-decomposition,
//                   the pseudo-inverse with the ABSOLUTE threshold 1e-8, the Schur complement, its eigen-decomposition, J0 = sqrt(S) V^T, r0 = sqrt(S^-1) V^T b.
//   marg_jacobi     the eigen-solver: cyclic two-sided Jacobi, parallel round-robin ordering (n - 1 rounds of n / 2 disjoint pairs per sweep).  A round
//                   writes every entry of J^T A J from the previous round's matrix into a second buffer (upper triangle computed, mirrored: the matrix stays
//                   symmetric bit for bit), so nothing in it depends on which wave runs first; sums and the order of rotations are fixed: two calls give
//                   the same bits.  At most kMargMaxSweeps sweeps; a cap that is reached is reported and nothing is written.
// LDS: the assembly's WinSys (49 288 B; its H is the eigen-solver's second buffer afterwards) + three 60 x 60 f64 matrices (system, matrix under rotation,
// eigenvectors: 3 x 28 800 B) + 3 840 B of vectors = 139 528 B = 136.3 KiB of the CU's 160 KiB: one workgroup per CU, which is all this launch has.
// Rows come out by ascending eigenvalue, each eigenvector with its largest-magnitude component positive (the first one on ties); nothing may depend on either.
constexpr int kMargThreads = 256;
constexpr int kMargMaxSweeps = 30;            // f64 Jacobi converges quadratically: 4 .. 6 sweeps per decomposition measured on the harness windows (reported in lili_window_prior_storage)
constexpr double kMargEps = 1e-8;             // MarginalizationInfo::eps
// converged: sum of squares above the diagonal <= (1e-20)^2 x the matrix' squared Frobenius norm.  Far below the rounding of the diagonal on purpose: what is left
// above the diagonal turns the eigenvectors by (entry / eigenvalue gap), and the gaps here are small against the norm (eigenvalues 2e2 beside 5e7, clusters such as a
// ninefold 225) — at 1e-20 no gap above 1e-4 of an ulp of the norm matters.  Reachable because annihilated entries are set to exactly 0 and the others only ever shrink
// quadratically; it costs at most one sweep over a bound of 1e-32.
constexpr double kMargTol2 = 1e-40;

struct MargArgs { int pos, m; int sel[kWinMaxN]; };      // window mode: column sel[i] of the 15 n_kf local columns is dimension i of the system (dropped first)
struct MargOut {
    int status /* 0, 1 = sweep cap reached */, rank, sweeps[2];
    double r0[kWinMaxN];
    double J0[kWinMaxN * kWinMaxN];           // n x n, tight
};
struct MargShared {
    WinSys sys;
    double A[kWinMaxN * kWinMaxN], M[kWinMaxN * kWinMaxN], V[kWinMaxN * kWinMaxN];
    double b[kWinMaxN], w[kWinMaxN], bs[kWinMaxN], red[kWinMaxN];
    double cs[kWinMaxN], bt[kWinMaxN], dd[kWinMaxN];      // this round, per index: cosine, coefficient of the partner's row / column, change of the diagonal entry
    int partner[kWinMaxN], pp[kWinMaxN / 2], qq[kWinMaxN / 2];
};

// sum of squares of the n x n matrix A (or of its part above the diagonal) in a fixed order; every thread returns the same bits
__device__ __forceinline__ double marg_sumsq(MargShared& sh, const double* A, const int n, const bool upper) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < n) {
        double v = 0.0;
        for (int j = upper ? tid + 1 : 0; j < n; j++) v += A[tid * n + j] * A[tid * n + j];
        sh.red[tid] = v;
    }
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < n; i++) t += sh.red[i];
    return t;
}

// Eigen-decomposition of the symmetric n x n matrix in A0 (tight) by the whole workgroup: on return A0 holds the rotated matrix (eigenvalues on its diagonal),
// V the eigenvectors as columns; A1 is scratch of the same size.  Returns the number of sweeps, or -1 when kMargMaxSweeps did not suffice (uniform).
template <int kWho = 0>
__device__ __noinline__ int marg_jacobi(MargShared& sh, double* A0, double* A1, double* V, const int n) {
    const int tid = threadIdx.x;
    const int np = n + (n & 1), hp = np >> 1;      // an odd n plays with a bye: the pair that holds index n rests
    for (int e = tid; e < n * n; e += kMargThreads) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    double* cur = A0;
    double* nxt = A1;
    const double tot2 = marg_sumsq(sh, cur, n, false);
    int sweeps = -1;
    for (int sweep = 0; sweep <= kMargMaxSweeps; sweep++) {
        const double off2 = marg_sumsq(sh, cur, n, true);
        if (off2 <= kMargTol2 * tot2) { sweeps = sweep; break; }
        if (sweep == kMargMaxSweeps) break;
        for (int r = 0; r < np - 1; r++) {
            // ---- the round's pairs (circle method: index np - 1 stays, the others turn) and their rotations, from the matrix as the last round left it
            if (tid < hp) {
                const int a = tid == 0 ? r : (r + tid) % (np - 1), b = tid == 0 ? np - 1 : (r + (np - 1) - tid) % (np - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, s = 0.0, d = 0.0;
                bool rot = false;
                if (q < n) {
                    const double apq = cur[p * n + q];
                    if (apq != 0.0) {
                        const double th = (cur[q * n + q] - cur[p * n + p]) / (2.0 * apq);
                        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0); s = t * c; d = t * apq; rot = true;
                    }
                    sh.cs[q] = c; sh.bt[q] = s; sh.dd[q] = d; sh.partner[q] = p;
                }
                sh.cs[p] = c; sh.bt[p] = -s; sh.dd[p] = -d; sh.partner[p] = q < n ? q : p;
                sh.pp[tid] = p; sh.qq[tid] = rot ? q : -1;
            }
            __syncthreads();
            // ---- J^T A J, entry by entry: new row / column i = cs[i] * old i + bt[i] * old partner[i]
            for (int e = tid; e < n * n; e += kMargThreads) {
                const int i = e / n, j = e - i * n;
                if (i > j) continue;
                const int pi = sh.partner[i], pj = sh.partner[j];
                double v;
                if (i == j) v = cur[e] + sh.dd[i];          // a_pp - t a_pq, a_qq + t a_pq
                else if (pi == j) v = 0.0;                  // the entry the rotation annihilates
                else {
                    const double ci = sh.cs[i], bi = sh.bt[i], cj = sh.cs[j], bj = sh.bt[j];
                    v = ci * (cj * cur[i * n + j] + bj * cur[i * n + pj]) + bi * (cj * cur[pi * n + j] + bj * cur[pi * n + pj]);
                }
                nxt[i * n + j] = v; nxt[j * n + i] = v;
            }
            // ---- V J: both columns of a pair by one thread per row
            for (int e = tid; e < n * hp; e += kMargThreads) {
                const int i = e / hp, k = e - i * hp;
                const int q = sh.qq[k];
                if (q < 0) continue;
                const int p = sh.pp[k];
                const double c = sh.cs[p], s = sh.bt[q], vp = V[i * n + p], vq = V[i * n + q];
                V[i * n + p] = c * vp - s * vq; V[i * n + q] = s * vp + c * vq;
            }
            __syncthreads();
            double* t = cur; cur = nxt; nxt = t;
        }
    }
    if (cur != A0) {
        __syncthreads();
        for (int e = tid; e < n * n; e += kMargThreads) A0[e] = cur[e];
    }
    __syncthreads();
    return sweeps;
}

// MarginalizationFactor.cpp:176-201 on sh.A (pos x pos, tight), sh.b: the first m dimensions go.  `work`: pos x pos doubles of scratch.
template <int kWho = 0>
__device__ __noinline__ void marg_schur(MargShared& sh, double* work, const int pos, const int m, MargOut* __restrict__ out) {
    const int tid = threadIdx.x;
    const int n = pos - m;
    const double* A = sh.A;
    double* M = sh.M;
    double* V = sh.V;
    for (int e = tid; e < m * m; e += kMargThreads) { const int i = e / m, j = e - i * m; M[e] = 0.5 * (A[i * pos + j] + A[j * pos + i]); }
    const int sw1 = marg_jacobi<kWho>(sh, M, work, V, m);
    if (sw1 < 0) { if (tid == 0) { out->status = 1; out->rank = 0; out->sweeps[0] = sw1; out->sweeps[1] = 0; } return; }
    if (tid < m) { const double l = M[tid * m + tid]; sh.w[tid] = l > kMargEps ? 1.0 / l : 0.0; }
    __syncthreads();
    for (int e = tid; e < m * m; e += kMargThreads) {                  // Amm^+ = V diag(1 / lambda, 0 where lambda <= eps) V^T
        const int i = e / m, j = e - i * m;
        double v = 0.0;
        for (int k = 0; k < m; k++) v += (V[i * m + k] * sh.w[k]) * V[j * m + k];
        M[e] = v;
    }
    __syncthreads();
    double* W = work;                                                   // Amm^+ [Amr | bmm], m x (n + 1)
    for (int e = tid; e < m * (n + 1); e += kMargThreads) {
        const int i = e / (n + 1), c = e - i * (n + 1);
        double v = 0.0;
        for (int j = 0; j < m; j++) v += M[i * m + j] * (c < n ? A[j * pos + m + c] : sh.b[j]);
        W[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += kMargThreads) {                  // S = Arr - Arm Amm^+ Amr: the lower triangle, mirrored (an eigen-solver reads one triangle)
        const int i = e / n, j = e - i * n;
        if (i < j) continue;
        double v = 0.0;
        for (int k = 0; k < m; k++) v += A[(m + i) * pos + k] * W[k * (n + 1) + j];
        v = A[(m + i) * pos + m + j] - v;
        M[i * n + j] = v; M[j * n + i] = v;
    }
    if (tid < n) {
        double v = 0.0;
        for (int k = 0; k < m; k++) v += A[(m + tid) * pos + k] * W[k * (n + 1) + n];
        sh.bs[tid] = sh.b[m + tid] - v;
    }
    const int sw2 = marg_jacobi<kWho>(sh, M, work, V, n);
    if (sw2 < 0) { if (tid == 0) { out->status = 1; out->rank = 0; out->sweeps[0] = sw1; out->sweeps[1] = sw2; } return; }
    if (tid < n) sh.w[tid] = M[tid * n + tid];
    __syncthreads();
    if (tid < n) {
        const double l = sh.w[tid];
        int row = 0, big = 0;
        for (int j = 0; j < n; j++) row += (sh.w[j] < l || (sh.w[j] == l && j < tid)) ? 1 : 0;      // ascending eigenvalue, ties by index
        for (int c = 1; c < n; c++) if (fabs(V[c * n + tid]) > fabs(V[big * n + tid])) big = c;
        const double sg = V[big * n + tid] < 0.0 ? -1.0 : 1.0;
        const bool keep = l > kMargEps;
        const double sq = keep ? sqrt(l) : 0.0, sqi = keep ? sqrt(1.0 / l) : 0.0;
        double d = 0.0;
        for (int c = 0; c < n; c++) d += (sg * V[c * n + tid]) * sh.bs[c];
        out->r0[row] = keep ? sqi * d : 0.0;
        for (int c = 0; c < n; c++) out->J0[row * n + c] = keep ? sq * (sg * V[c * n + tid]) : 0.0;
    }
    if (tid == 0) {
        int rank = 0;
        for (int j = 0; j < n; j++) rank += sh.w[j] > kMargEps ? 1 : 0;
        out->status = 0; out->rank = rank; out->sweeps[0] = sw1; out->sweeps[1] = sw2;
    }
}

// pb != nullptr: the window's system at pb->state (rec: the n_kf lidar records of k_window_reduce, or nullptr), dimensions a.sel; pb == nullptr: the system
// the host uploaded (sys_in: pos x pos tight, then b).  One workgroup.
__global__ __launch_bounds__(kMargThreads) void k_window_marg(const WinDev* __restrict__ pb, const double* __restrict__ rec, const double* __restrict__ sys_in, MargArgs a,
                                                              MargOut* __restrict__ out) {
    __shared__ MargShared sh;
    const int tid = threadIdx.x;
    const int pos = a.pos;
    if (pb) {
        const int n_kf = pb->n_kf, N = 15 * n_kf;
        if (tid < 64) {
            for (int e = tid; e < 16 * n_kf; e += 64) sh.sys.x[e / 16][e % 16] = pb->state[e];
            for (int e = tid; e < 72 * n_kf; e += 64) sh.sys.lid[e / 72][e % 72] = rec ? rec[e] : 0.0;
            LILI_WAVE_SYNC();
            win_build<true>(pb, sh.sys);
        }
        __syncthreads();
        for (int e = tid; e < pos * pos; e += kMargThreads) { const int i = e / pos, j = e - i * pos; sh.A[e] = sh.sys.H[a.sel[i] * N + a.sel[j]]; }
        if (tid < pos) sh.b[tid] = sh.sys.g[a.sel[tid]];
    } else {
        for (int e = tid; e < pos * pos; e += kMargThreads) sh.A[e] = sys_in[e];
        if (tid < pos) sh.b[tid] = sys_in[pos * pos + tid];
    }
    __syncthreads();
    marg_schur(sh, sh.sys.H, pos, a.m, out);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The cycle (include/lili_hip.h: lili_window_cycle): behind k_window_solve on the same stream, k_window_writeback (sign unification, gates), the lidar launches at the
// slots' device poses, k_window_marg_cycle (the next prior, left in the context's resident buffer).  Nothing here waits for another workgroup; every loop is bounded.
// ------------------------------------------------------------------------------------------------------------------------------------
struct WinPriorDev { double x0[16 * kWinMaxKf], r0[kWinMaxN], J0[kWinMaxN * kWinMaxN], A0[kWinMaxN * kWinMaxN]; };      // the resident prior: WinDev's members x0 .. A0, one device-to-device copy apart
static_assert(offsetof(WinDev, r0) - offsetof(WinDev, x0) == offsetof(WinPriorDev, r0) && offsetof(WinDev, J0) - offsetof(WinDev, x0) == offsetof(WinPriorDev, J0) &&
              offsetof(WinDev, A0) - offsetof(WinDev, x0) == offsetof(WinPriorDev, A0) && offsetof(WinDev, imu) - offsetof(WinDev, x0) == sizeof(WinPriorDev),
              "WinPriorDev is the run of WinDev from x0 to A0");
struct WinWbArgs { SlotState* st[kWinMaxKf]; int n, summary_words; double gate_p, gate_q, gate_v, gate_ba, gate_bg; };
struct WinCycleMargArgs { MargArgs a; int n_blocks, kind[kWinMaxBlocks], kf[kWinMaxBlocks]; };

// Eigen's quaternion product, sums left to right
__device__ __forceinline__ void wb_qmul(const double* a, const double* b, double* o) {
    o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
    o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
    o[2] = ((a[0] * b[2] + a[2] * b[0]) + a[3] * b[1]) - a[1] * b[3];
    o[3] = ((a[0] * b[3] + a[3] * b[0]) + a[1] * b[2]) - a[2] * b[1];
}
// the general branch of Eigen 3.3's matrix -> quaternion for the largest diagonal entry i (j, k its successors): returns w, writes the three vector components
__device__ __forceinline__ double wb_branch(double Rii, double Rjj, double Rkk, double Rkj, double Rjk, double Rji, double Rij, double Rki, double Rik, double& qi, double& qj, double& qk) {
    double t = sqrt(((Rii - Rjj) - Rkk) + 1.0);
    qi = 0.5 * t;
    t = 0.5 / t;
    qj = (Rji + Rij) * t;
    qk = (Rki + Rik) * t;
    return (Rkj - Rjk) * t;
}
// Quaterniond(q.toRotationMatrix()) of a normalised q (w x y z): the formulas lili_om_amd/loop.py restates (_matrix_from_quat, quat_from_matrix)
__device__ __forceinline__ void wb_round_trip(const double* q, double* o) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R00 = 1.0 - 2.0 * (y * y + z * z), R01 = 2.0 * (x * y - w * z), R02 = 2.0 * (x * z + w * y);
    const double R10 = 2.0 * (x * y + w * z), R11 = 1.0 - 2.0 * (x * x + z * z), R12 = 2.0 * (y * z - w * x);
    const double R20 = 2.0 * (x * z - w * y), R21 = 2.0 * (y * z + w * x), R22 = 1.0 - 2.0 * (x * x + y * y);
    const double tr = (R00 + R11) + R22;
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        o[0] = 0.5 * t;
        t = 0.5 / t;
        o[1] = (R21 - R12) * t; o[2] = (R02 - R20) * t; o[3] = (R10 - R01) * t;
        return;
    }
    int i = 0;
    if (R11 > R00) i = 1;
    if (R22 > (i == 0 ? R00 : R11)) i = 2;
    if (i == 0) o[0] = wb_branch(R00, R11, R22, R21, R12, R10, R01, R20, R02, o[1], o[2], o[3]);
    else if (i == 1) o[0] = wb_branch(R11, R22, R00, R02, R20, R21, R12, R01, R10, o[2], o[3], o[1]);
    else o[0] = wb_branch(R22, R00, R11, R10, R01, R02, R20, R12, R21, o[3], o[1], o[2]);
}

// ONE wave behind k_window_solve: lane k < n unifies keyframe k's q where the solve left it (`state`, in place) and in its slot's device pose, moves the mean of its
// speed-bias prior (if it has one) to the solved speed-bias for the marginalisation behind it, then applies the
// gates of L/src/BackendFusion.cpp:1187-1284 against pb->state; the wave copies the solve's summary into the result and clears the prior's fields (k_window_marg_cycle sets them)
__global__ __launch_bounds__(64) void k_window_writeback(WinDev* __restrict__ pb, double* __restrict__ state, const lili_lm_summary* __restrict__ summary, WinWbArgs a,
                                                         lili_window_cycle_result* __restrict__ out) {
    const int lane = threadIdx.x;
    {
        const double* s = reinterpret_cast<const double*>(summary);
        double* d = reinterpret_cast<double*>(&out->summary);
        for (int e = lane; e < a.summary_words; e += 64) d[e] = s[e];
    }
    if (lane == 0) { out->prior_updated = 0; out->prior_n = 0; out->prior_blocks = 0; out->rank = 0; out->sweeps_mm = 0; out->sweeps_s = 0; }
    if (lane >= a.n) return;
    double x[16], in[16];
    for (int i = 0; i < 16; i++) { x[i] = state[16 * lane + i]; in[i] = pb->state[16 * lane + i]; }
    if (x[3] < 0.0) {
        for (int i = 3; i < 7; i++) { x[i] = -x[i]; state[16 * lane + i] = x[i]; }
    }
    for (int i = 3; i < 7; i++) a.st[lane]->pose[i] = x[i];
    // the marginalisation's speed-bias priors take the SOLVED speed-bias as their mean (L/src/BackendFusion.cpp:1045-1057: residual 0, information 225 I); the solve is over,
    // so the uploaded problem block is this launch's to change
    if (pb->sb_has[lane]) for (int i = 0; i < 9; i++) pb->sb_mean[9 * lane + i] = x[7 + i];
    const double dp0 = in[0] - x[0], dp1 = in[1] - x[1], dp2 = in[2] - x[2];
    const double pnorm = sqrt((dp0 * dp0 + dp1 * dp1) + dp2 * dp2);
    const double dv0 = in[7] - x[7], dv1 = in[8] - x[8], dv2 = in[9] - x[9];
    const double vnorm = sqrt((dv0 * dv0 + dv1 * dv1) + dv2 * dv2);
    double qn[4], qi[4], dq[4];
    {
        const double n = sqrt(((x[4] * x[4] + x[5] * x[5]) + x[6] * x[6]) + x[3] * x[3]);
        for (int i = 0; i < 4; i++) qn[i] = x[3 + i] / n;
        const double n2 = ((qn[1] * qn[1] + qn[2] * qn[2]) + qn[3] * qn[3]) + qn[0] * qn[0];
        qi[0] = qn[0] / n2; qi[1] = -qn[1] / n2; qi[2] = -qn[2] / n2; qi[3] = -qn[3] / n2;
        wb_qmul(qi, in + 3, dq);
    }
    const double qnorm = sqrt((dq[1] * dq[1] + dq[2] * dq[2]) + dq[3] * dq[3]);
    unsigned refused = 0;
    if (!(pnorm < a.gate_p)) refused |= 1u;
    if (!(qnorm < a.gate_q)) refused |= 2u;
    if (!(vnorm < a.gate_v)) refused |= 4u;
    for (int i = 0; i < 3; i++) {
        if (!(fabs(in[10 + i] - x[10 + i]) < a.gate_ba)) refused |= 8u << i;
        if (!(fabs(in[13 + i] - x[13 + i]) < a.gate_bg)) refused |= 64u << i;
    }
    double ab[16], nx[16];
    for (int i = 0; i < 3; i++) ab[i] = (refused & 1u) ? in[i] : x[i];
    for (int i = 3; i < 7; i++) ab[i] = (refused & 2u) ? in[i] : x[i];
    for (int i = 7; i < 10; i++) ab[i] = (refused & 4u) ? in[i] : x[i];
    for (int i = 0; i < 3; i++) {
        ab[10 + i] = (refused & (8u << i)) ? in[10 + i] : x[10 + i];
        ab[13 + i] = (refused & (64u << i)) ? in[13 + i] : x[13 + i];
    }
    for (int i = 0; i < 16; i++) nx[i] = ab[i];
    if (!(refused & 2u)) wb_round_trip(qn, nx + 3);
    for (int i = 0; i < 16; i++) { out->solved[16 * lane + i] = x[i]; out->abs_state[16 * lane + i] = ab[i]; out->next_state[16 * lane + i] = nx[i]; }
    out->refused[lane] = refused;
}

// k_window_marg in cycle mode (a second entry point: k_window_marg stays the code it was — its callees too: win_build<true, 1>, marg_schur<1> are this kernel's own copies,
// because a second caller of one copy ends the compiler's specialisation to the single call site and changes the instructions k_window_marg runs): the state is the one k_window_writeback left in `state`, a solve that stalled
// marginalises nothing, and after marg_schur the workgroup writes the resident prior — J0, r0, x0 = the kept blocks' values of that state, and A0 = J0^T J0 with the row
// index ascending per entry (window_pack's order on the host), computed from a copy of J0 in sh.A, which the Schur step no longer needs.  A sweep cap that is reached
// leaves the resident prior as it was (out->status tells the host).
__global__ __launch_bounds__(kMargThreads) void k_window_marg_cycle(const WinDev* __restrict__ pb, const double* __restrict__ rec, const double* __restrict__ state,
                                                                    const lili_lm_summary* __restrict__ summary, WinCycleMargArgs c, MargOut* out, WinPriorDev* __restrict__ res,
                                                                    lili_window_cycle_result* __restrict__ cyc) {
    __shared__ MargShared sh;
    const int tid = threadIdx.x;
    const int pos = c.a.pos, m = c.a.m, n = pos - m;
    if (summary->termination == LILI_LM_STALLED) { if (tid == 0) out->status = 0; return; }
    {
        const int n_kf = pb->n_kf, N = 15 * n_kf;
        if (tid < 64) {
            for (int e = tid; e < 16 * n_kf; e += 64) sh.sys.x[e / 16][e % 16] = state[e];
            for (int e = tid; e < 72 * n_kf; e += 64) sh.sys.lid[e / 72][e % 72] = rec ? rec[e] : 0.0;
            LILI_WAVE_SYNC();
            win_build<true, 1>(pb, sh.sys);
        }
        __syncthreads();
        for (int e = tid; e < pos * pos; e += kMargThreads) { const int i = e / pos, j = e - i * pos; sh.A[e] = sh.sys.H[c.a.sel[i] * N + c.a.sel[j]]; }
        if (tid < pos) sh.b[tid] = sh.sys.g[c.a.sel[tid]];
    }
    __syncthreads();
    marg_schur<1>(sh, sh.sys.H, pos, m, out);
    __threadfence();
    __syncthreads();
    if (*reinterpret_cast<volatile int*>(&out->status) != 0) return;      // uniform: written by thread 0 before the barrier
    for (int e = tid; e < n * n; e += kMargThreads) { const double v = out->J0[e]; sh.A[e] = v; res->J0[e] = v; }
    if (tid < n) res->r0[tid] = out->r0[tid];
    if (tid < c.n_blocks) {
        int off = 0;
        for (int b = 0; b < tid; b++) off += c.kind[b] == 0 ? 3 : c.kind[b] == 1 ? 4 : 9;
        const int kind = c.kind[tid], gs = kind == 0 ? 3 : kind == 1 ? 4 : 9, first = kind == 0 ? 0 : kind == 1 ? 3 : 7;
        for (int i = 0; i < gs; i++) res->x0[off + i] = sh.sys.x[c.kf[tid]][first + i];
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += kMargThreads) {
        const int a = e / n, b = e - a * n;
        double v = 0.0;
        for (int r = 0; r < n; r++) v += sh.A[r * n + a] * sh.A[r * n + b];
        res->A0[e] = v;
    }
    if (tid == 0) { cyc->prior_updated = 1; cyc->rank = out->rank; cyc->sweeps_mm = out->sweeps[0]; cyc->sweeps_s = out->sweeps[1]; }
}

}  // namespace lili

// ------------------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------------------
// sqrt_info = LLT(cov^-1).matrixL()^T in plain C++ (long double accumulation): cov = C C^T, cov^-1 = C^-T C^-1, Cholesky of that.  false: not positive definite
static bool window_sqrt_info(const double* cov, double* out) {
    constexpr int n = 15;
    long double C[n][n] = {}, Ci[n][n] = {}, A[n][n] = {}, L[n][n] = {};
    auto chol = [&](long double (*M)[n], long double (*R)[n]) {
        for (int j = 0; j < n; j++) {
            long double d = M[j][j];
            for (int k = 0; k < j; k++) d -= R[j][k] * R[j][k];
            if (!(d > 0.0L) || !std::isfinite((double)d)) return false;
            R[j][j] = sqrtl(d);
            for (int i = j + 1; i < n; i++) {
                long double v = M[i][j];
                for (int k = 0; k < j; k++) v -= R[i][k] * R[j][k];
                R[i][j] = v / R[j][j];
            }
        }
        return true;
    };
    long double M[n][n];
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
        if (!std::isfinite(cov[n * i + j])) return false;
        M[i][j] = 0.5L * ((long double)cov[n * i + j] + (long double)cov[n * j + i]);
    }
    if (!chol(M, C)) return false;
    for (int j = 0; j < n; j++) {          // C^-1, lower triangular
        Ci[j][j] = 1.0L / C[j][j];
        for (int i = j + 1; i < n; i++) {
            long double v = 0.0L;
            for (int k = j; k < i; k++) v -= C[i][k] * Ci[k][j];
            Ci[i][j] = v / C[i][i];
        }
    }
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
        long double v = 0.0L;
        for (int k = std::max(i, j); k < n; k++) v += Ci[k][i] * Ci[k][j];
        A[i][j] = v;
    }
    if (!chol(A, L)) return false;
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) out[n * i + j] = (double)L[j][i];
    return true;
}

// A0 = J0^T J0 (n_cols x n_cols, tight), the row index ascending per entry: the order k_window_marg_cycle uses on the device
static void window_prior_gram(const double* J0, int n_rows, int n_cols, double* A0) {
    for (int a = 0; a < n_cols; a++) for (int b = 0; b < n_cols; b++) {
        double v = 0.0;
        for (int r = 0; r < n_rows; r++) v += J0[r * n_cols + a] * J0[r * n_cols + b];
        A0[a * n_cols + b] = v;
    }
}

// the block table of a prior, checked (sizes, kinds, keyframes below kf_bound, no block twice, n_cols = the blocks' local sizes) and, with D, written into the packed
// problem's blk_* / col_blk tables; *x0_doubles = the length of x0.  One definition for window_pack and lili_window_prior_set.
static int window_prior_table(lili_ctx* ctx, const lili_window_prior& p, int kf_bound, const std::string& w, WinDev* D, int* x0_doubles) {
    ARGCHK(p.n_blocks >= 1 && p.n_blocks <= kWinMaxBlocks && p.block_kind && p.block_keyframe, w + ": bad prior");
    ARGCHK(p.n_rows >= 1 && p.n_rows <= kWinMaxN && p.n_cols >= 1 && p.n_cols <= kWinMaxN, w + ": prior size out of range");
    int col = 0, off = 0;
    for (int b = 0; b < p.n_blocks; b++) {
        const int kind = p.block_kind[b], kf = p.block_keyframe[b];
        ARGCHK(kind >= 0 && kind <= 2 && kf >= 0 && kf < kf_bound, w + ": bad prior block");
        for (int k = 0; k < b; k++) ARGCHK(!(p.block_kind[k] == kind && p.block_keyframe[k] == kf), w + ": duplicate prior block");
        const int ls = kind == 2 ? 9 : 3, gs = kind == 0 ? 3 : kind == 1 ? 4 : 9;
        if (D) {
            D->blk_kind[b] = kind; D->blk_kf[b] = kf; D->blk_col[b] = col; D->blk_x0[b] = off;
            for (int i = 0; i < ls && col + i < kWinMaxN; i++) D->col_blk[col + i] = b;
        }
        col += ls; off += gs;
    }
    ARGCHK(col == p.n_cols, w + ": n_cols of the prior does not match its blocks");
    *x0_doubles = off;
    return LILI_OK;
}

// validates the problem and packs it (with `state`) into ctx->win_host; nothing is enqueued
// resident: the problem's prior is the context's resident one — has_prior, the sizes and the blk_* / col_blk tables come from the host's kept-block table, and x0, r0, J0, A0
// stay zero here (the caller copies them over the uploaded block on the device)
static int window_pack(lili_ctx* ctx, const lili_window_problem* pr, const double* state, bool solve, const char* who, bool resident = false) {
    const std::string w(who);
    ARGCHK(pr && state, w + ": null argument");
    ARGCHK(pr->n_kf >= 2 && pr->n_kf <= LILI_WINDOW_MAX_KF, w + ": n_kf must be in 2..LILI_WINDOW_MAX_KF");
    ARGCHK((pr->kind_mask & ~3) == 0 && (pr->kind_mask != 0 || !solve), w + ": bad kind mask");
    const int n_kf = pr->n_kf;
    if (pr->kind_mask) {
        ARGCHK(pr->slots, w + ": null slots");
        for (int i = 0; i < n_kf; i++) {
            ARGCHK(pr->slots[i] >= 0 && pr->slots[i] < LILI_MAX_SLOTS, w + ": bad slot");
            for (int k = 0; k < i; k++) ARGCHK(pr->slots[k] != pr->slots[i], w + ": duplicate slot");
            for (int kind = 0; kind < 2; kind++) if (pr->kind_mask & (1 << kind))
                if (!ctx->slots[pr->slots[i]].k[kind].has_records) return ctx->fail(LILI_E_STATE, w + ": a slot has no records (associate first)");
        }
    }
    for (int i = 0; i < 16 * n_kf; i++) ARGCHK(std::isfinite(state[i]), w + ": state is not finite");
    ctx->win_host.assign(sizeof(WinDev), 0);
    WinDev& D = *reinterpret_cast<WinDev*>(ctx->win_host.data());
    D.n_kf = n_kf;
    std::memcpy(D.state, state, sizeof(double) * 16 * n_kf);
    if (pr->imu) {
        D.n_imu = n_kf - 1;
        for (int f = 0; f < D.n_imu; f++) {
            const lili_window_imu& s = pr->imu[f];
            WinImuDev& d = D.imu[f];
            d.sum_dt = s.sum_dt;
            std::memcpy(d.g, s.g, sizeof d.g); std::memcpy(d.dp, s.delta_p, sizeof d.dp); std::memcpy(d.dq, s.delta_q, sizeof d.dq); std::memcpy(d.dv, s.delta_v, sizeof d.dv);
            std::memcpy(d.ba, s.lin_ba, sizeof d.ba); std::memcpy(d.bg, s.lin_bg, sizeof d.bg);
            auto blk = [&](double* o, int r0, int c0) { for (int i = 0; i < 3; i++) for (int c = 0; c < 3; c++) o[3 * i + c] = s.jacobian[15 * (r0 + i) + c0 + c]; };
            blk(d.dp_dba, 0, 9); blk(d.dp_dbg, 0, 12); blk(d.dq_dbg, 3, 12); blk(d.dv_dba, 6, 9); blk(d.dv_dbg, 6, 12);
            if (!window_sqrt_info(s.covariance, d.sqrt_info)) return ctx->fail(LILI_E_ARG, w + ": an IMU covariance is not positive definite");
        }
    }
    if (pr->sb_prior) for (int k = 0; k < n_kf; k++) {
        D.sb_has[k] = std::isnan(pr->sb_prior[9 * k]) ? 0 : 1;
        if (D.sb_has[k]) for (int i = 0; i < 9; i++) { ARGCHK(std::isfinite(pr->sb_prior[9 * k + i]), w + ": speed-bias prior is not finite"); D.sb_mean[9 * k + i] = pr->sb_prior[9 * k + i]; }
    }
    if (pr->prior || resident) {
        int rc_tab;
        lili_window_prior p{};
        if (resident) {
            const lili_ctx::WinResidentTable& rt = ctx->win_res_tab;
            p.n_rows = rt.n_rows; p.n_cols = rt.n_cols; p.n_blocks = rt.n_blocks; p.block_kind = rt.kind; p.block_keyframe = rt.kf;
        } else {
            p = *pr->prior;
            ARGCHK(p.x0 && p.J0 && p.r0, w + ": bad prior");
        }
        int off = 0;
        if ((rc_tab = window_prior_table(ctx, p, n_kf, w, &D, &off)) != LILI_OK) return rc_tab;
        D.has_prior = 1; D.n_rows = p.n_rows; D.n_cols = p.n_cols; D.n_blocks = p.n_blocks;
        if (!resident) {
            std::memcpy(D.x0, p.x0, sizeof(double) * off);
            std::memcpy(D.r0, p.r0, sizeof(double) * p.n_rows);
            std::memcpy(D.J0, p.J0, sizeof(double) * p.n_rows * p.n_cols);
            window_prior_gram(p.J0, p.n_rows, p.n_cols, D.A0);
        }
    }
    return LILI_OK;
}
static lili_s2m_params window_params(const lili_window_problem* pr, const lili_s2m_params* params) {
    lili_s2m_params p = *params;
    if (pr->q_lb[0] != 0 || pr->q_lb[1] != 0 || pr->q_lb[2] != 0 || pr->q_lb[3] != 0) { std::memcpy(p.q_lb, pr->q_lb, sizeof p.q_lb); std::memcpy(p.t_lb, pr->t_lb, sizeof p.t_lb); }
    return p;
}

// launches k_window_marg on what the caller put into ctx->win_prob (window mode) or ctx->win_marg_in (a host system) and fetches its MargOut: ONE synchronisation
static int marg_run(lili_ctx* ctx, const WinDev* d_prob, const double* d_rec, const double* d_sys, const MargArgs& a, MargOut* h_out, const char* who) {
    HIPCHK(ctx->win_marg.ensure(sizeof(MargOut)));
    hipLaunchKernelGGL(k_window_marg, dim3(1), dim3(kMargThreads), 0, ctx->stream, d_prob, d_rec, d_sys, a, ctx->win_marg.as<MargOut>());
    HIPCHK(hipGetLastError());
    const int n = a.pos - a.m;
    const MargOut* d = ctx->win_marg.as<MargOut>();
    int rc = lili_readback_add(ctx, h_out, d, offsetof(MargOut, J0) + sizeof(double) * n * n);
    if (rc != LILI_OK) { (void)lili_readback_finish(ctx); return rc; }
    if ((rc = lili_readback_finish(ctx)) != LILI_OK) return rc;
    if (h_out->status != 0) return ctx->fail(LILI_E_NUMERIC, std::string(who) + ": the Jacobi eigen-solver reached its sweep cap without converging");
    return LILI_OK;
}

// the blocks the reference's factor set touches (L/src/BackendFusion.cpp:1009-1165), in (keyframe, kind) order: keyframe 0's go, the others stay
// read from the PACKED problem, the words win_build<true> itself branches on (has_prior, sb_has, n_imu) — so the columns picked here are the ones it fills
static int window_marg_table(lili_ctx* ctx, const lili_window_problem* problem, const char* who, WinCycleMargArgs& c) {
    const int n_kf = problem->n_kf;
    const WinDev& D = *reinterpret_cast<const WinDev*>(ctx->win_host.data());
    bool touched[kWinMaxKf][3] = {};
    if (D.has_prior) for (int b = 0; b < D.n_blocks; b++) touched[D.blk_kf[b]][D.blk_kind[b]] = true;
    for (int k = 0; k < n_kf; k++) if (D.sb_has[k]) touched[k][2] = true;
    if (D.n_imu >= 1) for (int k = 0; k < 2; k++) for (int kind = 0; kind < 3; kind++) touched[k][kind] = true;      // the factor between keyframes 0 and 1 only
    if (problem->kind_mask) for (int k = 0; k < n_kf; k++) touched[k][0] = touched[k][1] = true;                      // rec != nullptr below
    c = WinCycleMargArgs{};
    MargArgs& a = c.a;
    for (int k = 0; k < n_kf; k++) for (int kind = 0; kind < 3; kind++) {
        if (!touched[k][kind]) continue;
        const int first = 15 * k + (kind == 0 ? 0 : kind == 1 ? 3 : 6), size = kind == 2 ? 9 : 3;
        for (int i = 0; i < size; i++) a.sel[a.pos++] = first + i;
        if (k == 0) a.m = a.pos;
        else { c.kind[c.n_blocks] = kind; c.kf[c.n_blocks] = k; c.n_blocks++; }
    }
    ARGCHK(a.m >= 1, std::string(who) + ": no factor touches keyframe 0");
    ARGCHK(a.pos > a.m, std::string(who) + ": no factor touches a keyframe that stays");
    return LILI_OK;
}

extern "C" {

int lili_window_sqrt_info(const double covariance[225], double sqrt_info[225]) {
    if (!covariance || !sqrt_info) return LILI_E_ARG;
    return window_sqrt_info(covariance, sqrt_info) ? LILI_OK : LILI_E_ARG;
}

int lili_window_evaluate(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const double* state,
                         double* cost, double* gradient, double* JtJ) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(params && cost && gradient, "window_evaluate: null argument");
    int rc = window_pack(ctx, problem, state, false, "window_evaluate");
    if (rc != LILI_OK) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const int n_kf = problem->n_kf, N = 15 * n_kf;
    const size_t n_out = (size_t)1 + N + (size_t)N * N;
    HIPCHK(ctx->win_prob.ensure(sizeof(WinDev)));
    HIPCHK(ctx->win_out.ensure(sizeof(double) * (1 + kWinMaxN + kWinMaxN * kWinMaxN) + sizeof(lili_lm_summary)));
    const double* rec = nullptr;
    if (problem->kind_mask) {
        double t[3 * kWinMaxKf], q[4 * kWinMaxKf];
        for (int k = 0; k < n_kf; k++) { std::memcpy(t + 3 * k, state + 16 * k, 3 * sizeof(double)); std::memcpy(q + 4 * k, state + 16 * k + 3, 4 * sizeof(double)); }
        const lili_s2m_params p = window_params(problem, params);
        HIPCHK(ctx->win_rec.ensure(sizeof(double) * LILI_GRAM_DOUBLES * LILI_MAX_SLOTS));
        if ((rc = lili_match_window_records(ctx, problem->slots, n_kf, problem->kind_mask, &p, t, q, ctx->win_rec.as<double>())) != LILI_OK) return rc;
        rec = ctx->win_rec.as<double>();
    }
    HIPCHK(hipMemcpyAsync(ctx->win_prob.p, ctx->win_host.data(), sizeof(WinDev), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_window_evaluate, dim3(1), dim3(64), 0, ctx->stream, ctx->win_prob.as<WinDev>(), rec, ctx->win_out.as<double>(), JtJ ? 1 : 0);
    HIPCHK(hipGetLastError());
    const double* d = ctx->win_out.as<double>();
    rc = lili_readback_add(ctx, cost, d, sizeof(double));
    if (rc == LILI_OK) rc = lili_readback_add(ctx, gradient, d + 1, sizeof(double) * N);
    if (rc == LILI_OK && JtJ) rc = lili_readback_add(ctx, JtJ, d + 1 + N, sizeof(double) * N * N);
    (void)n_out;
    if (rc != LILI_OK) { (void)lili_readback_finish(ctx); return rc; }
    return lili_readback_finish(ctx);
}

// the packed problem (ctx->win_host) uploaded and k_window_solve enqueued behind it; resident: the resident prior copied over the uploaded block's x0 .. A0 in between,
// device to device.  Every refusal comes before the first enqueue.  state_bak (the cycle): the slots' states are copied there first, and *enqueued tells the caller that from here
// on a failure has poses to put back.
static int window_solve_enqueue(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params& p, const lili_lm_options* options, bool resident, WinSolveArgs& W,
                                void* state_bak = nullptr, bool* enqueued = nullptr) {
    const int n_kf = problem->n_kf;
    // every workgroup has to be resident: the share of the CUs lili_s2m_solve_lm_window gives a slot, and at most kWinGroup per slot (one exchange hop)
    const int max_blocks = std::max(1, std::min(std::min(ctx->n_simd / 4 - 16, 240) / n_kf, kWinGroup));
    HIPCHK(ctx->win_prob.ensure(sizeof(WinDev)));
    HIPCHK(ctx->win_out.ensure(sizeof(double) * (1 + kWinMaxN + kWinMaxN * kWinMaxN) + sizeof(lili_lm_summary)));
    W = WinSolveArgs{};
    W.n = n_kf;
    int nb = 0, rc;
    for (int i = 0; i < n_kf; i++) {
        if ((rc = lili_match_lm_args(ctx, problem->slots[i], problem->kind_mask, &p, options, max_blocks, &W.a[i])) != LILI_OK) return rc;
        if (W.a[i].nb > kWinGroup) return ctx->fail(LILI_E_STATE, "window_solve: internal: too many workgroups for one exchange hop");
        W.first_block[i] = nb;
        nb += W.a[i].nb;
    }
    W.prob = ctx->win_prob.as<WinDev>();
    W.state_out = ctx->win_out.as<double>();
    W.summary = reinterpret_cast<lili_lm_summary*>(ctx->win_out.as<double>() + 1 + kWinMaxN + kWinMaxN * kWinMaxN);
    MatchParams P = lili_match_device_params(&p);
    P.no_cost = 0;                              // the robust cost drives the accept / reject decisions
    if (state_bak) {
        HIPCHK(hipMemcpyAsync(state_bak, ctx->states.p, sizeof(SlotState) * LILI_MAX_SLOTS, hipMemcpyDeviceToDevice, ctx->stream));
        *enqueued = true;
    }
    HIPCHK(hipMemcpyAsync(ctx->win_prob.p, ctx->win_host.data(), sizeof(WinDev), hipMemcpyHostToDevice, ctx->stream));
    if (resident) HIPCHK(hipMemcpyAsync(reinterpret_cast<unsigned char*>(ctx->win_prob.p) + offsetof(WinDev, x0), ctx->win_res.p, sizeof(WinPriorDev), hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_window_solve, dim3(nb), dim3(kWinThreads), lds_linearize(kWinThreads), ctx->stream, W, P);
    HIPCHK(hipGetLastError());
    return LILI_OK;
}

int lili_window_solve(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const lili_lm_options* options,
                      double* state, lili_lm_summary* summary) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(params, "window_solve: null params");
    int rc = window_pack(ctx, problem, state, true, "window_solve");
    if (rc != LILI_OK) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const int n_kf = problem->n_kf;
    const lili_s2m_params p = window_params(problem, params);
    WinSolveArgs W;
    if ((rc = window_solve_enqueue(ctx, problem, p, options, false, W)) != LILI_OK) return rc;
    if (summary) {
        rc = lili_readback_add(ctx, summary, W.summary, sizeof(lili_lm_summary));
        if (rc == LILI_OK) rc = lili_readback_add(ctx, state, W.state_out, sizeof(double) * 16 * n_kf);
        if (rc != LILI_OK) { (void)lili_readback_finish(ctx); return rc; }
        return lili_readback_finish(ctx);
    }
    return LILI_OK;
}

int lili_window_state_get(lili_ctx* ctx, int n_kf, double* state) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(state && n_kf >= 2 && n_kf <= LILI_WINDOW_MAX_KF, "window_state_get: bad argument");
    if (!ctx->win_out.p) return ctx->fail(LILI_E_STATE, "window_state_get: no lili_window_solve yet");
    HIPCHK(hipSetDevice(ctx->device));
    const int rc = lili_readback_add(ctx, state, ctx->win_out.p, sizeof(double) * 16 * n_kf);
    if (rc != LILI_OK) { (void)lili_readback_finish(ctx); return rc; }
    return lili_readback_finish(ctx);
}

int lili_marg_schur(lili_ctx* ctx, const double* A, size_t ld, const double* b, int pos, int m, double* J0, double* r0, int* rank) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(A && b && J0 && r0 && rank, "marg_schur: null argument");
    ARGCHK(pos >= 2 && pos <= kWinMaxN && m >= 1 && m < pos && ld >= (size_t)pos, "marg_schur: need 2 <= pos <= 60, 1 <= m < pos, ld >= pos");
    std::vector<double> sys((size_t)pos * pos + pos);
    for (int i = 0; i < pos; i++) {
        for (int j = 0; j < pos; j++) { const double v = A[(size_t)i * ld + j]; ARGCHK(std::isfinite(v), "marg_schur: A is not finite"); sys[(size_t)i * pos + j] = v; }
        ARGCHK(std::isfinite(b[i]), "marg_schur: b is not finite");
        sys[(size_t)pos * pos + i] = b[i];
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->win_marg_in.ensure(sizeof(double) * sys.size()));
    HIPCHK(hipMemcpyAsync(ctx->win_marg_in.p, sys.data(), sizeof(double) * sys.size(), hipMemcpyHostToDevice, ctx->stream));
    MargArgs a{};
    a.pos = pos; a.m = m;
    std::vector<unsigned char> buf(sizeof(MargOut));
    MargOut* o = reinterpret_cast<MargOut*>(buf.data());
    const int rc = marg_run(ctx, nullptr, nullptr, ctx->win_marg_in.as<double>(), a, o, "marg_schur");
    if (rc != LILI_OK) return rc;
    const int n = pos - m;
    std::memcpy(J0, o->J0, sizeof(double) * n * n);
    std::memcpy(r0, o->r0, sizeof(double) * n);
    *rank = o->rank;
    return LILI_OK;
}

int lili_window_marginalize(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const double* state, lili_window_prior_storage* out) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(params && out, "window_marginalize: null argument");
    int rc = window_pack(ctx, problem, state, false, "window_marginalize");
    if (rc != LILI_OK) return rc;
    const int n_kf = problem->n_kf;
    WinCycleMargArgs c{};
    if ((rc = window_marg_table(ctx, problem, "window_marginalize", c)) != LILI_OK) return rc;
    const MargArgs& a = c.a;
    const int n_blocks = c.n_blocks;
    const int* kind_of = c.kind;
    const int* kf_of = c.kf;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->win_prob.ensure(sizeof(WinDev)));
    const double* rec = nullptr;
    if (problem->kind_mask) {      // the launches of lili_window_evaluate: every slot linearised at `state`
        double t[3 * kWinMaxKf], q[4 * kWinMaxKf];
        for (int k = 0; k < n_kf; k++) { std::memcpy(t + 3 * k, state + 16 * k, 3 * sizeof(double)); std::memcpy(q + 4 * k, state + 16 * k + 3, 4 * sizeof(double)); }
        const lili_s2m_params p = window_params(problem, params);
        HIPCHK(ctx->win_rec.ensure(sizeof(double) * LILI_GRAM_DOUBLES * LILI_MAX_SLOTS));
        if ((rc = lili_match_window_records(ctx, problem->slots, n_kf, problem->kind_mask, &p, t, q, ctx->win_rec.as<double>())) != LILI_OK) return rc;
        rec = ctx->win_rec.as<double>();
    }
    HIPCHK(hipMemcpyAsync(ctx->win_prob.p, ctx->win_host.data(), sizeof(WinDev), hipMemcpyHostToDevice, ctx->stream));
    std::vector<unsigned char> buf(sizeof(MargOut));
    MargOut* o = reinterpret_cast<MargOut*>(buf.data());
    if ((rc = marg_run(ctx, ctx->win_prob.as<WinDev>(), rec, nullptr, a, o, "window_marginalize")) != LILI_OK) return rc;
    // ---- the prior as the NEXT window sees it: keyframe k is its keyframe k - 1 (addr_shift, L:1170-1177), x0 = the block's value in `state`
    const int n = a.pos - a.m;
    std::memset(out, 0, sizeof *out);
    int off = 0;
    for (int b = 0; b < n_blocks; b++) {
        const int kind = kind_of[b], gs = kind == 0 ? 3 : kind == 1 ? 4 : 9;
        out->block_kind[b] = kind; out->block_keyframe[b] = kf_of[b] - 1;
        std::memcpy(out->x0 + off, state + 16 * kf_of[b] + (kind == 0 ? 0 : kind == 1 ? 3 : 7), sizeof(double) * gs);
        off += gs;
    }
    std::memcpy(out->J0, o->J0, sizeof(double) * n * n);
    std::memcpy(out->r0, o->r0, sizeof(double) * n);
    out->rank = o->rank; out->sweeps_mm = o->sweeps[0]; out->sweeps_s = o->sweeps[1];
    out->prior.n_rows = n; out->prior.n_cols = n; out->prior.n_blocks = n_blocks;
    out->prior.block_kind = out->block_kind; out->prior.block_keyframe = out->block_keyframe;
    out->prior.x0 = out->x0; out->prior.J0 = out->J0; out->prior.r0 = out->r0;
    return LILI_OK;
}

// lili_window_cycle without its clean-up: *enqueued is set once the solve's launches are on the stream (the slots' states saved in win_state_bak just before).  The next prior
// is written into win_res_nxt and becomes the resident one (a swap of the two buffers) only when everything, the read-back included, has succeeded.
static int window_cycle_body(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const lili_lm_options* options,
                             const lili_window_cycle_options* cycle_options, const double* state_in, lili_window_cycle_result* out, bool* enqueued) {
    ARGCHK(params && out, "window_cycle: null argument");
    lili_window_cycle_options co{10.0, 10.0, 10.0, 22.0, 22.0, 0, 0};
    if (cycle_options) co = *cycle_options;
    const bool resident = co.use_resident_prior != 0;
    ARGCHK(!(resident && problem && problem->prior), "window_cycle: use_resident_prior together with a prior of the problem");
    // ---- every refusal of the chain, before anything of the cycle is enqueued (a context's first cycle clears its two new prior buffers on the way): the solve's, then the marginalisation's (its factor set is the packed problem's)
    int rc = window_pack(ctx, problem, state_in, true, "window_cycle", resident && ctx->win_res_tab.valid);
    if (rc != LILI_OK) return rc;
    if (resident && !ctx->win_res_tab.valid) return ctx->fail(LILI_E_STATE, "window_cycle: no resident prior (no cycle has left one, or lili_window_cycle_reset dropped it)");
    const int n_kf = problem->n_kf;
    WinCycleMargArgs c{};
    if ((rc = window_marg_table(ctx, problem, "window_cycle", c)) != LILI_OK) return rc;
    const lili_lm_options opt = lm_options_or_default(options);
    HIPCHK(hipSetDevice(ctx->device));
    for (DevBuf* b : {&ctx->win_res, &ctx->win_res_nxt})
        if (!b->p) { HIPCHK(b->ensure(sizeof(WinPriorDev))); HIPCHK(hipMemsetAsync(b->p, 0, sizeof(WinPriorDev), ctx->stream)); }
    HIPCHK(ctx->win_cyc.ensure(sizeof(lili_window_cycle_result)));
    HIPCHK(ctx->win_state_bak.ensure(sizeof(SlotState) * LILI_MAX_SLOTS));
    HIPCHK(ctx->win_marg.ensure(sizeof(MargOut)));
    HIPCHK(ctx->win_rec.ensure(sizeof(double) * LILI_GRAM_DOUBLES * LILI_MAX_SLOTS));
    const lili_s2m_params p = window_params(problem, params);
    // ---- the solve (its own refusals still come before its first enqueue)
    WinSolveArgs W;
    if ((rc = window_solve_enqueue(ctx, problem, p, options, resident, W, ctx->win_state_bak.p, enqueued)) != LILI_OK) return rc;
    // ---- unification and gates, one wave
    const int rows = std::min(std::max(opt.max_iterations, 0), LILI_LM_MAX_LOG);      // the log has a row per judged candidate: at most max_iterations of them
    const size_t summary_bytes = offsetof(lili_lm_summary, it) + sizeof(lili_lm_iteration) * rows;
    WinWbArgs wb{};
    wb.n = n_kf; wb.summary_words = (int)(summary_bytes / sizeof(double));
    for (int k = 0; k < n_kf; k++) wb.st[k] = ctx->state(problem->slots[k]);
    wb.gate_p = co.gate_p; wb.gate_q = co.gate_q; wb.gate_v = co.gate_v; wb.gate_ba = co.gate_ba; wb.gate_bg = co.gate_bg;
    lili_window_cycle_result* d_cyc = ctx->win_cyc.as<lili_window_cycle_result>();
    hipLaunchKernelGGL(k_window_writeback, dim3(1), dim3(64), 0, ctx->stream, ctx->win_prob.as<WinDev>(), W.state_out, (const lili_lm_summary*)W.summary, wb, d_cyc);
    HIPCHK(hipGetLastError());
    // ---- the lidar records at the slots' device poses (the unified state), then the next prior into the resident buffer
    if ((rc = lili_match_window_records(ctx, problem->slots, n_kf, problem->kind_mask, &p, nullptr, nullptr, ctx->win_rec.as<double>())) != LILI_OK) return rc;
    MargOut* d_marg = ctx->win_marg.as<MargOut>();
    hipLaunchKernelGGL(k_window_marg_cycle, dim3(1), dim3(kMargThreads), 0, ctx->stream, (const WinDev*)W.prob, (const double*)ctx->win_rec.as<double>(), (const double*)W.state_out,
                       (const lili_lm_summary*)W.summary, c, d_marg, ctx->win_res_nxt.as<WinPriorDev>(), d_cyc);
    HIPCHK(hipGetLastError());
    // ---- one synchronisation, one read-back: the summary's rows that can be written, n_kf rows of the three states, the gates' and the prior's words
    std::vector<unsigned char> buf(sizeof(lili_window_cycle_result), 0);
    lili_window_cycle_result* h = reinterpret_cast<lili_window_cycle_result*>(buf.data());
    int marg_status[4] = {0, 0, 0, 0};
    const size_t row_bytes = sizeof(double) * 16 * n_kf, tail = offsetof(lili_window_cycle_result, refused);
    rc = lili_readback_add(ctx, &h->summary, &d_cyc->summary, summary_bytes);
    if (rc == LILI_OK) rc = lili_readback_add(ctx, h->solved, d_cyc->solved, row_bytes);
    if (rc == LILI_OK) rc = lili_readback_add(ctx, h->abs_state, d_cyc->abs_state, row_bytes);
    if (rc == LILI_OK) rc = lili_readback_add(ctx, h->next_state, d_cyc->next_state, row_bytes);
    if (rc == LILI_OK) rc = lili_readback_add(ctx, buf.data() + tail, reinterpret_cast<const unsigned char*>(d_cyc) + tail, sizeof(lili_window_cycle_result) - tail);
    if (rc == LILI_OK) rc = lili_readback_add(ctx, marg_status, d_marg, sizeof marg_status);
    if (rc != LILI_OK) { (void)lili_readback_finish(ctx); return rc; }
    if ((rc = lili_readback_finish(ctx)) != LILI_OK) return rc;
    if (marg_status[0] != 0)      // the sweep cap: nothing was written into win_res_nxt; the caller puts the slots' states back
        return ctx->fail(LILI_E_NUMERIC, "window_cycle: the Jacobi eigen-solver reached its sweep cap without converging");
    for (int k = n_kf; k < kWinMaxKf; k++) h->refused[k] = 0;
    for (int r = std::max(h->summary.n_logged, 0); r < LILI_LM_MAX_LOG; r++) std::memset(&h->summary.it[r], 0, sizeof(lili_lm_iteration));
    if (h->prior_updated) {
        ctx->win_res.swap(ctx->win_res_nxt);
        lili_ctx::WinResidentTable& rt = ctx->win_res_tab;
        rt.valid = true; rt.n_rows = rt.n_cols = c.a.pos - c.a.m; rt.n_blocks = c.n_blocks;
        rt.rank = h->rank; rt.sweeps[0] = h->sweeps_mm; rt.sweeps[1] = h->sweeps_s;
        for (int b = 0; b < c.n_blocks; b++) { rt.kind[b] = c.kind[b]; rt.kf[b] = c.kf[b] - 1; }      // the next window's numbering (addr_shift, L:1170-1177)
        h->prior_n = rt.n_cols; h->prior_blocks = rt.n_blocks;
    }
    std::memcpy(out, h, sizeof *out);
    return LILI_OK;
}

int lili_window_cycle(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const lili_lm_options* options,
                      const lili_window_cycle_options* cycle_options, const double* state_in, lili_window_cycle_result* out) {
    if (!ctx) return LILI_E_ARG;
    bool enqueued = false;
    const int rc = window_cycle_body(ctx, problem, params, options, cycle_options, state_in, out, &enqueued);
    if (rc != LILI_OK && enqueued) {
        // a failure behind the solve's launches — the sweep cap, a launch, the read-back: the slots get the states they had before the solve, and the stream is drained so
        // that nothing of the failed cycle is still running when the call returns.  The message of the failure stays; an error of this clean-up is not reported on top of it.
        const std::string msg = ctx->err;
        (void)lili_readback_finish(ctx);
        (void)hipMemcpyAsync(ctx->states.p, ctx->win_state_bak.p, sizeof(SlotState) * LILI_MAX_SLOTS, hipMemcpyDeviceToDevice, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        ctx->err = msg;
    }
    return rc;
}

int lili_window_cycle_reset(lili_ctx* ctx) {
    if (!ctx) return LILI_E_ARG;
    ctx->win_res_tab = lili_ctx::WinResidentTable{};
    return LILI_OK;
}

int lili_window_prior_get(lili_ctx* ctx, lili_window_prior_storage* out) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(out, "window_prior_get: null argument");
    const lili_ctx::WinResidentTable& rt = ctx->win_res_tab;
    if (!rt.valid) return ctx->fail(LILI_E_STATE, "window_prior_get: no resident prior");
    HIPCHK(hipSetDevice(ctx->device));
    int off = 0;
    for (int b = 0; b < rt.n_blocks; b++) off += rt.kind[b] == 0 ? 3 : rt.kind[b] == 1 ? 4 : 9;
    std::vector<double> x0(off), r0(rt.n_rows), J0((size_t)rt.n_rows * rt.n_cols);
    const WinPriorDev* d = ctx->win_res.as<WinPriorDev>();
    // three plain copies, then the synchronisation (36 KB at most: more than the page-locked scratch's lazy items take)
    HIPCHK(hipMemcpyAsync(x0.data(), d->x0, sizeof(double) * x0.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(r0.data(), d->r0, sizeof(double) * r0.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(J0.data(), d->J0, sizeof(double) * J0.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memset(out, 0, sizeof *out);
    for (int b = 0; b < rt.n_blocks; b++) { out->block_kind[b] = rt.kind[b]; out->block_keyframe[b] = rt.kf[b]; }
    std::memcpy(out->x0, x0.data(), sizeof(double) * x0.size());
    std::memcpy(out->r0, r0.data(), sizeof(double) * r0.size());
    std::memcpy(out->J0, J0.data(), sizeof(double) * J0.size());
    out->rank = rt.rank; out->sweeps_mm = rt.sweeps[0]; out->sweeps_s = rt.sweeps[1];
    out->prior.n_rows = rt.n_rows; out->prior.n_cols = rt.n_cols; out->prior.n_blocks = rt.n_blocks;
    out->prior.block_kind = out->block_kind; out->prior.block_keyframe = out->block_keyframe;
    out->prior.x0 = out->x0; out->prior.J0 = out->J0; out->prior.r0 = out->r0;
    return LILI_OK;
}

int lili_window_prior_set(lili_ctx* ctx, const lili_window_prior* prior) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(prior, "window_prior_set: null argument");
    const lili_window_prior& p = *prior;
    ARGCHK(p.x0 && p.J0 && p.r0, "window_prior_set: bad prior");
    int off = 0;
    const int rc_tab = window_prior_table(ctx, p, kWinMaxKf, "window_prior_set", nullptr, &off);
    if (rc_tab != LILI_OK) return rc_tab;
    for (int i = 0; i < off; i++) ARGCHK(std::isfinite(p.x0[i]), "window_prior_set: x0 is not finite");
    for (int i = 0; i < p.n_rows; i++) ARGCHK(std::isfinite(p.r0[i]), "window_prior_set: r0 is not finite");
    for (int i = 0; i < p.n_rows * p.n_cols; i++) ARGCHK(std::isfinite(p.J0[i]), "window_prior_set: J0 is not finite");
    std::vector<unsigned char> buf(sizeof(WinPriorDev), 0);
    WinPriorDev& h = *reinterpret_cast<WinPriorDev*>(buf.data());
    std::memcpy(h.x0, p.x0, sizeof(double) * off);
    std::memcpy(h.r0, p.r0, sizeof(double) * p.n_rows);
    std::memcpy(h.J0, p.J0, sizeof(double) * p.n_rows * p.n_cols);
    window_prior_gram(p.J0, p.n_rows, p.n_cols, h.A0);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->win_res.ensure(sizeof(WinPriorDev)));
    HIPCHK(hipMemcpyAsync(ctx->win_res.p, buf.data(), sizeof(WinPriorDev), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // `buf` is pageable and goes out of scope
    lili_ctx::WinResidentTable& rt = ctx->win_res_tab;
    rt = lili_ctx::WinResidentTable{};
    rt.valid = true; rt.n_rows = p.n_rows; rt.n_cols = p.n_cols; rt.n_blocks = p.n_blocks;
    for (int b = 0; b < p.n_blocks; b++) { rt.kind[b] = p.block_kind[b]; rt.kf[b] = p.block_keyframe[b]; }
    for (int r = 0; r < p.n_rows; r++) {
        bool nz = false;
        for (int cc = 0; cc < p.n_cols; cc++) nz = nz || p.J0[r * p.n_cols + cc] != 0.0;
        rt.rank += nz ? 1 : 0;
    }
    return LILI_OK;
}

}  // extern "C"
