// Global pose graph over every frame (include/lili_hip.h: lili_pose_graph*): what saveKeyFramesAndFactors, performLoopClosure and correctPoses
// (L/src/BackendFusion.cpp:1820-1889, 2587-2633, 2177-2311) hand to GTSAM, as a batch Gauss-Newton solve on the device, f64, no contraction.
//
// One iteration is nine launches (more with the blocked reduced solve), every one enqueued up front; none waits for another workgroup, every loop is bounded by the graph's size:
//   k_pg_linearize         two lanes per factor: the even one the weighted residual and the Jacobian block of the factor's first node, the odd one the second node's;
//                          a loop with a robust loss (lili_pose_graph_add_loop_robust) is scaled by sqrt(w), w from its unweighted d^2 = |r|^2, which both lanes
//                          compute on the same bits and the even one keeps in lw for the cost;
//   k_pg_assemble          one lane per entry of H and g, by gather: a node sums its <= 2 chain contributions, then its loop contributions in loop order;
//   k_pg_gate              one workgroup: |g|inf (and, before the first step, the cost) in a fixed order; sets the termination word at the gradient tolerance;
//   k_pg_eliminate         one wave per segment: 6 x 6-block Cholesky along the chain between two separators, lane c carrying column c of
//                          [L block^T | g | columns of the left separator | columns of the right separator] through the forward substitution, and the 13 x 13
//                          Gram of the carried columns — the segment's Schur contribution;
//   k_pg_zero              the reduced system's storage cleared;
//   k_pg_reduced_assemble  one workgroup per block of the reduced system over the separators that can be non-zero (diagonal, adjacent separators, pairs joined
//                          by a loop): diagonal, Schur terms, loop blocks in loop order;
//   k_pg_reduced_solve     up to kPgMaxReduced unknowns.  One workgroup: dense left-looking Cholesky (one row per thread, fixed-order sums) and the two substitutions;
//   k_pg_chol_*            beyond.  A right-looking blocked Cholesky in tiles of kPgTile unknowns, per tile column k three launches: _diag (one workgroup factors
//                          the diagonal tile in LDS, checks the pivots, solves its piece of L y = b), _panel (one workgroup per row tile below: L_ik = A_ik L_kk^-T,
//                          and b_i -= L_ik y_k), _update (one workgroup per lower-triangle tile: A_ij -= L_ik L_jk^T on v_mfma_f64_16x16x4_f64, operands staged in
//                          LDS); then per tile row i, last first, _back: every workgroup solves x_i = L_ii^-T y_i on the same bits, workgroup k < i takes
//                          L_ik^T x_i off y_k, workgroup i writes the step.  Every tile and every piece of b has one owner per launch and sums over k ascending;
//   k_pg_backsub           one wave per segment, every lane the same arithmetic: the interior nodes' step from the separators';
//   k_pg_retract_cost      one workgroup: the candidate, its cost in a fixed order (a robust loop adds rho, not half its squared residual), the accept / stop
//                          decision, the termination word.
// lili_pose_graph_solve_lm is the same chain with PgTables::damping set: k_pg_eliminate (its kDamped instance) and k_pg_reduced_assemble add PgState::lambda to H's diagonal as they read it
// (D itself stays undamped), a non-positive pivot raises PgState::fail instead of ending the solve and the launches up to the tail return at once, and the tail is
//   k_pg_lm_decide         accept (X <- candidate, lambda down) or reject (X stays, lambda up; past its bound the solve ends), the log of the attempt.
// A rejected attempt linearises again at the unchanged X.  lili_pose_graph_loop_status is one launch, k_pg_loop_status: d^2 and w of a range of loops.
// lili_pose_graph_marginals runs the launches up to the reduced factorisation (the gate in its evaluate mode: it decides nothing), then three of its own:
//   k_pg_marg_inverse      one workgroup per separator: its six columns of the reduced inverse through L and L^T, tile by tile;
//   k_pg_marg_segments     one wave per segment, last node first: W = -L_II^-T Y_E, the segment's own inverse blocks, Sigma(i, i) of every node;
//   k_pg_marg_pairs        one wave per requested pair: Sigma(i, j).
// No atomics anywhere: H, g, the cost and the step are pure functions of the graph.  The tables (separators, segments, loops, the loops of each node and of each
// reduced block) and the work arrays follow the graph's size: the reduced system takes 8 (6 K)^2 bytes, 1.3 GB at 1024 loops (K = 2112).
#include "lili_launch.h"
#include "lili_device_math.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace lili {

__device__ __forceinline__ dq pg_conj(const dq q) { return dq{q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ dq pg_quat(const double* p) { return dq{p[3], p[4], p[5], p[6]}; }
__device__ __forceinline__ void pg_mat(const dq q, double R[9]) { const double a[4] = {q.w, q.x, q.y, q.z}; quat_to_mat(a, R); }
__device__ __forceinline__ void pg_mm3(const double* A, const double* B, double* O) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
// Log of a unit quaternion as a rotation vector, the angle in [0, pi]
__device__ __forceinline__ void pg_log(dq q, double phi[3]) {
    if (q.w < 0.0) q = dq{-q.w, -q.x, -q.y, -q.z};
    const double n2 = (q.x * q.x + q.y * q.y) + q.z * q.z;
    double k = 2.0;
    if (n2 > 0.0) { const double n = sqrt(n2); k = 2.0 * atan2(n, q.w) / n; }
    phi[0] = k * q.x; phi[1] = k * q.y; phi[2] = k * q.z;
}
// S = [v]x, row-major (host too: lili_pose_relative_covariance)
__host__ __device__ __forceinline__ void pg_skew(const double x, const double y, const double z, double S[9]) {
    S[0] = 0.0; S[1] = -z; S[2] = y; S[3] = z; S[4] = 0.0; S[5] = -x; S[6] = -y; S[7] = x; S[8] = 0.0;
}
// the inverse of SO(3)'s right Jacobian: I + [phi]x / 2 + c [phi]x^2, c by its series below LILI_PG_SMALL_ANGLE
__device__ __forceinline__ void pg_jr_inv(const double phi[3], double M[9]) {
    const double t2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
    double c;
    if (t2 < LILI_PG_SMALL_ANGLE * LILI_PG_SMALL_ANGLE) c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0)));
    else { const double t = sqrt(t2); c = 1.0 / t2 - (1.0 + cos(t)) / (2.0 * t * sin(t)); }
    double S[9];
    pg_skew(phi[0], phi[1], phi[2], S);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = ((i == j ? 1.0 : 0.0) + 0.5 * S[3 * i + j]) + c * (phi[i] * phi[j] - (i == j ? t2 : 0.0));
}
// e = (Log(R_Z^T R_A^T R_B), R_Z^T (R_A^T (p_B - p_A) - t_Z)); also qab = q_A^-1 q_B, d = R_A^T (p_B - p_A), qe = q_Z^-1 qab
__device__ __forceinline__ void pg_error(const d3 pa, const dq qa, const d3 pb, const dq qb, const double* Z, double e[6], dq& qab, d3& d, dq& qe) {
    const dq ia = pg_conj(qa), iz = pg_conj(pg_quat(Z));
    d = qrot(ia, pb - pa);
    const d3 ev = qrot(iz, d - d3{Z[0], Z[1], Z[2]});
    qab = qmul(ia, qb);
    qe = qmul(iz, qab);
    pg_log(qe, e);
    e[3] = ev.x; e[4] = ev.y; e[5] = ev.z;
}
__device__ __forceinline__ double pg_sq6(const double* r) { return ((((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]) + r[4] * r[4]) + r[5] * r[5]; }
// Robust loss on a loop (GTSAM's mEstimator::Huber / Cauchy / GemanMcClure), d2 = |r|^2 of the whitened residual, k the scale: the weight w = rho'(d) / d ...
__device__ __forceinline__ double pg_loss_weight(const int loss, const double k, const double d2) {
    if (loss == LILI_PG_LOSS_HUBER) { const double d = sqrt(d2); return d <= k ? 1.0 : k / d; }
    const double k2 = k * k, u = k2 / (k2 + d2);
    return loss == LILI_PG_LOSS_CAUCHY ? u : u * u;
}
// ... and 2 rho(d), what the factor adds to twice the cost (a factor without a loss adds d2)
__device__ __forceinline__ double pg_loss_rho2(const int loss, const double k, const double d2) {
    if (loss == LILI_PG_LOSS_HUBER) { const double d = sqrt(d2); return d <= k ? d2 : 2.0 * (k * (d - 0.5 * k)); }
    const double k2 = k * k;
    return loss == LILI_PG_LOSS_CAUCHY ? k2 * log1p(d2 / k2) : k2 * (d2 / (k2 + d2));
}
// the loss of factor f: LILI_PG_LOSS_NONE for the prior and the chain
__device__ __forceinline__ int pg_loss_of(const PgTables& T, const int f, double& scale) {
    if (f < T.n) { scale = 0.0; return LILI_PG_LOSS_NONE; }
    const PgLoop& l = T.loop[f - T.n];
    scale = l.scale;
    return l.loss;
}
// the two poses, the measurement and the weights of factor f at the estimates x
struct PgFactorIn { d3 pa, pb; dq qa, qb; const double* Z; const double* w; };
__device__ __forceinline__ PgFactorIn pg_factor(const PgTables& T, const double* x, const double* meas, const int f) {
    PgFactorIn F;
    int a = -1, b = 0;
    if (f == 0) { F.Z = meas; F.w = T.w_prior; }
    else if (f < T.n) { a = f - 1; b = f; F.Z = meas + 7 * (size_t)f; F.w = T.w_odom; }
    else { const PgLoop& l = T.loop[f - T.n]; a = l.from; b = l.to; F.Z = l.meas; F.w = l.w; }
    if (a < 0) { F.pa = d3{0.0, 0.0, 0.0}; F.qa = dq{1.0, 0.0, 0.0, 0.0}; }
    else { const double* A = x + 7 * (size_t)a; F.pa = d3{A[0], A[1], A[2]}; F.qa = pg_quat(A); }
    const double* B = x + 7 * (size_t)b;
    F.pb = d3{B[0], B[1], B[2]}; F.qb = pg_quat(B);
    return F;
}
// d^2 = |r|^2 of a factor's whitened error: one text for the cost, the linearisation's weight and lili_pose_graph_loop_status
__device__ __forceinline__ double pg_whitened_d2(const PgFactorIn& F, const double e[6]) {
    double r[6];
#pragma unroll
    for (int k = 0; k < 6; k++) r[k] = e[k] * F.w[k];
    return pg_sq6(r);
}
__device__ __forceinline__ double pg_factor_cost(const PgTables& T, const double* x, const double* meas, const int f) {
    const PgFactorIn F = pg_factor(T, x, meas, f);
    double e[6];
    dq qab, qe; d3 d;
    pg_error(F.pa, F.qa, F.pb, F.qb, F.Z, e, qab, d, qe);
    const double d2 = pg_whitened_d2(F, e);
    double scale;
    const int loss = pg_loss_of(T, f, scale);
    return loss == LILI_PG_LOSS_NONE ? d2 : pg_loss_rho2(loss, scale, d2);
}
// Op (PgSum / PgMax) over the kPgWide threads of the single-workgroup stages, in a fixed order; every thread gets the result
struct PgSum { __device__ double operator()(const double a, const double b) const { return a + b; } };
struct PgMax { __device__ double operator()(const double a, const double b) const { return fmax(a, b); } };
template <class Op>
__device__ __forceinline__ double pg_block_reduce(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = kPgWide / 2; s > 0; s >>= 1) { if (t < s) sh[t] = Op()(sh[t], sh[t + s]); __syncthreads(); }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// x <- L^-1 x and x <- L^-T x, L a row-major lower-triangular 6 x 6 block
__device__ __forceinline__ void pg_fwd6(const double* L, double x[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double v = x[k];
#pragma unroll
        for (int m = 0; m < k; m++) v -= L[6 * k + m] * x[m];
        x[k] = v / L[6 * k + k];
    }
}
__device__ __forceinline__ void pg_back6(const double* L, double x[6]) {
#pragma unroll
    for (int k = 5; k >= 0; k--) {
        double v = x[k];
#pragma unroll
        for (int m = k + 1; m < 6; m++) v -= L[6 * m + k] * x[m];
        x[k] = v / L[6 * k + k];
    }
}

// new nodes first .. first + n - 1 from the staged rows (row 0 = prev, rows 1 .. n = the poses): estimates and frozen measurements
__global__ void k_pg_append(const double* __restrict__ rows, const int first, const int n, double* __restrict__ X, double* __restrict__ meas) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = first + i;
    const double* B = rows + 7 * (size_t)(i + 1);
    const double* A = rows + 7 * (size_t)i;
    double* x = X + 7 * (size_t)id;
    double* m = meas + 7 * (size_t)id;
#pragma unroll
    for (int k = 0; k < 7; k++) x[k] = B[k];
    if (id == 0) {
#pragma unroll
        for (int k = 0; k < 7; k++) m[k] = B[k];
        return;
    }
    const dq ia = pg_conj(pg_quat(A));
    const d3 t = qrot(ia, d3{B[0] - A[0], B[1] - A[1], B[2] - A[2]});
    const dq q = qmul(ia, pg_quat(B));
    m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = q.w; m[4] = q.x; m[5] = q.y; m[6] = q.z;
}

__global__ __launch_bounds__(256) void k_pg_linearize(const PgDev G) {
    if (G.st->done) return;
    const PgTables& T = *G.tab;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = tid >> 1, side = tid & 1;
    if (f >= T.n + T.n_loops) return;
    const PgFactorIn F = pg_factor(T, G.X, G.meas, f);
    double e[6], Jri[9];
    dq qab, qe; d3 d;
    pg_error(F.pa, F.qa, F.pb, F.qb, F.Z, e, qab, d, qe);
    pg_jr_inv(e, Jri);
    // a loop: its unweighted d^2 and the weight of its loss, by both lanes of the factor on the same bits; a robust loop's rows are scaled by sqrt(w)
    bool robust = false;
    double sw = 1.0;
    if (f >= T.n) {
        double scale;
        const double d2 = pg_whitened_d2(F, e);
        const int loss = pg_loss_of(T, f, scale);
        robust = loss != LILI_PG_LOSS_NONE;
        const double wl = robust ? pg_loss_weight(loss, scale, d2) : 1.0;
        sw = sqrt(wl);
        if (side == 0) { G.lw[2 * (size_t)(f - T.n)] = d2; G.lw[2 * (size_t)(f - T.n) + 1] = wl; }
    }
    auto rw = [&](const double v) { return robust ? v * sw : v; };
    double* J = G.fJ + (size_t)f * 72 + 36 * side;
    if (side == 0) {
        double* r = G.fr + (size_t)f * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) r[k] = rw(e[k] * F.w[k]);
        // first node: [-Jr^-1 Rab^T, 0; R_Z^T [d]x, -R_Z^T]
        double Rab[9], RabT[9], Rz[9], A[9], Bm[9];
        pg_mat(qab, Rab);
        pg_mat(pg_conj(pg_quat(F.Z)), Rz);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) RabT[3 * i + j] = Rab[3 * j + i];
        pg_mm3(Jri, RabT, A);
        double Sd[9];
        pg_skew(d.x, d.y, d.z, Sd);
        pg_mm3(Rz, Sd, Bm);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                J[6 * i + j] = rw(-A[3 * i + j] * F.w[i]); J[6 * i + 3 + j] = 0.0;
                J[6 * (3 + i) + j] = rw(Bm[3 * i + j] * F.w[3 + i]); J[6 * (3 + i) + 3 + j] = rw(-Rz[3 * i + j] * F.w[3 + i]);
            }
    } else {
        // second node: [Jr^-1, 0; 0, R_Z^T R_A^T R_B]
        double Re[9];
        pg_mat(qe, Re);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                J[6 * i + j] = rw(Jri[3 * i + j] * F.w[i]); J[6 * i + 3 + j] = 0.0;
                J[6 * (3 + i) + j] = 0.0; J[6 * (3 + i) + 3 + j] = rw(Re[3 * i + j] * F.w[3 + i]);
            }
    }
}

// (A^T B)[r][c] of two row-major 6 x 6 blocks, and (A^T v)[c]
__device__ __forceinline__ double pg_atb(const double* A, const double* B, const int r, const int c) {
    double s = A[r] * B[c];
#pragma unroll
    for (int k = 1; k < 6; k++) s += A[6 * k + r] * B[6 * k + c];
    return s;
}
__device__ __forceinline__ double pg_atv(const double* A, const double* v, const int c) {
    double s = A[c] * v[0];
#pragma unroll
    for (int k = 1; k < 6; k++) s += A[6 * k + c] * v[k];
    return s;
}
__global__ __launch_bounds__(256) void k_pg_assemble(const PgDev G) {
    if (G.st->done) return;
    const PgTables& T = *G.tab;
    const int n = T.n, L = T.n_loops;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long long)n * 78) {
        const int t = (int)(tid - (long long)n * 78);
        if (t >= 36 * L) return;
        const int l = t / 36, e = t - 36 * l;
        const double* J = G.fJ + (size_t)(n + l) * 72;
        G.LB[t] = pg_atb(J, J + 36, e / 6, e % 6);
        return;
    }
    const int i = (int)(tid / 78), e = (int)(tid - (long long)i * 78);
    const double* Jb = G.fJ + (size_t)i * 72 + 36;                  // factor i: node i is its second node
    const double* Ja = G.fJ + (size_t)(i + 1) * 72;                 // factor i + 1: node i is its first node
    const bool next = i + 1 < n;
    if (e < 36) {
        const int r = e / 6, c = e - 6 * r;
        double v = pg_atb(Jb, Jb, r, c);
        if (next) v += pg_atb(Ja, Ja, r, c);
        for (int u = T.node_ptr[i]; u < T.node_ptr[i + 1]; u++) {      // in loop order
            const int en = T.node_ent[u];
            const double* Jl = G.fJ + (size_t)(n + (en >> 1)) * 72 + 36 * (en & 1);
            v += pg_atb(Jl, Jl, r, c);
        }
        G.D[(size_t)i * 36 + e] = v;
    } else if (e < 72) {
        const int r = (e - 36) / 6, c = (e - 36) - 6 * r;
        G.S[(size_t)i * 36 + (e - 36)] = next ? pg_atb(Ja + 36, Ja, r, c) : 0.0;      // block (i + 1, i): second node's rows, first node's columns
    } else {
        const int c = e - 72;
        double v = pg_atv(Jb, G.fr + (size_t)i * 6, c);
        if (next) v += pg_atv(Ja, G.fr + (size_t)(i + 1) * 6, c);
        for (int u = T.node_ptr[i]; u < T.node_ptr[i + 1]; u++) {
            const int en = T.node_ent[u], l = en >> 1;
            v += pg_atv(G.fJ + (size_t)(n + l) * 72 + 36 * (en & 1), G.fr + (size_t)(n + l) * 6, c);
        }
        G.g[(size_t)i * 6 + c] = v;
    }
}

// evaluate == 0: the head of an iteration; != 0: lili_pose_graph_evaluate (cost and |g|inf into the state, nothing decided)
__global__ __launch_bounds__(kPgWide) void k_pg_gate(const PgDev G, const int evaluate) {
    if (G.st->done) return;
    __shared__ double sh[kPgWide];
    const PgTables& T = *G.tab;
    const int t = threadIdx.x, it = G.st->s.iterations;
    double m = 0.0;
    for (int i = t; i < 6 * T.n; i += kPgWide) m = fmax(m, fabs(G.g[i]));
    m = pg_block_reduce<PgMax>(m, sh);
    double cost = G.st->cost;
    if (it == 0 || evaluate) {
        double c = 0.0;
        for (int f = t; f < T.n + T.n_loops; f += kPgWide) {      // a robust loop adds 2 rho of its unweighted d^2, not the square of its weighted residual
            double scale;
            const int loss = pg_loss_of(T, f, scale);
            c += loss == LILI_PG_LOSS_NONE ? pg_sq6(G.fr + (size_t)f * 6) : pg_loss_rho2(loss, scale, G.lw[2 * (size_t)(f - T.n)]);
        }
        cost = 0.5 * pg_block_reduce<PgSum>(c, sh);
    }
    if (t == 0) {
        PgState& st = *G.st;
        st.gmax = m; st.fail = 0;
        if (it == 0 || evaluate) { st.cost = cost; st.s.initial_cost = cost; st.s.final_cost = cost; }
        if (!evaluate) {
            if (it < LILI_PG_MAX_LOG) st.s.grad_inf[it] = m;
            if (m <= T.gradient_tolerance) { st.s.termination = LILI_LM_GRADIENT_TOLERANCE; st.done = 1; }
        }
    }
}

// a diagonal entry of H under lili_pose_graph_solve_lm's damping (PgTables::damping != 0 in that call only): + lambda, or + lambda h
__device__ __forceinline__ double pg_damped(const double h, const int damping, const double lambda) { return damping == 1 ? h + lambda : h + lambda * h; }
// kDamped: lili_pose_graph_solve_lm's instance.  The pivot block sits on the serial path of the segment (one node after the other on one wave), so the calls
// that never damp run the instance that has no trace of it
template <bool kDamped>
__global__ __launch_bounds__(64) void k_pg_eliminate(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sLs[36];      // L block (i, i - 1), row by row
    __shared__ double sY[6 * kPgCols];      // the carried columns of node i, column by column
    const PgTables& T = *G.tab;
    const PgSeg sg = T.seg[blockIdx.x];
    const int c = threadIdx.x, n = T.n, damping = kDamped ? T.damping : 0;
    const double lambda = kDamped ? G.st->lambda : 0.0;
    double yprev[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, acc[3] = {0.0, 0.0, 0.0};
    bool ok = true;
    for (int i = sg.first; i <= sg.last; i++) {
        const bool first = i == sg.first;
        // the pivot block D_i - Ls Ls^T and its Cholesky factor, by every lane on the same bits
        double A[36];
        const double* Di = G.D + (size_t)i * 36;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int q = 0; q <= r; q++) {
                double v = Di[6 * r + q];
                if (kDamped && r == q) v = pg_damped(v, damping, lambda);
                if (!first) {
                    double s = sLs[6 * r] * sLs[6 * q];
#pragma unroll
                    for (int k = 1; k < 6; k++) s += sLs[6 * r + k] * sLs[6 * q + k];
                    v -= s;
                }
                A[6 * r + q] = v;
            }
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double s = A[6 * j + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= A[6 * j + k] * A[6 * j + k];
            ok = ok && (s > 0.0);
            const double l = sqrt(s);
            A[6 * j + j] = l;
#pragma unroll
            for (int r = j + 1; r < 6; r++) {
                double v = A[6 * r + j];
#pragma unroll
                for (int k = 0; k < j; k++) v -= A[6 * r + k] * A[6 * j + k];
                A[6 * r + j] = v / l;
            }
        }
        // this lane's column of [S_i^T | g_i | E_left | E_right] - Ls [0 | Y_(i-1)], then the forward substitution
        double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (c < 6) {
            if (i + 1 < n) {
#pragma unroll
                for (int k = 0; k < 6; k++) z[k] = G.S[(size_t)i * 36 + 6 * c + k];
            }
        } else if (c == 6) {
#pragma unroll
            for (int k = 0; k < 6; k++) z[k] = G.g[(size_t)i * 6 + k];
        } else if (c < 13) {
            if (first) {
#pragma unroll
                for (int k = 0; k < 6; k++) z[k] = G.S[(size_t)sg.left * 36 + 6 * k + (c - 7)];      // block (left + 1, left), its column c - 7
            }
        } else if (c < 19) {
            if (i == sg.last && sg.right >= 0) {
#pragma unroll
                for (int k = 0; k < 6; k++) z[k] = G.S[(size_t)i * 36 + 6 * (c - 13) + k];           // block (last, right) = block (right, last)^T, its column c - 13
            }
        }
        if (!first && c >= 6) {
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double s = sLs[6 * k] * yprev[0];
#pragma unroll
                for (int m = 1; m < 6; m++) s += sLs[6 * k + m] * yprev[m];
                z[k] -= s;
            }
        }
        pg_fwd6(A, z);
        __syncthreads();      // every lane has read sLs and sY of the previous node
        if (c < 6) {
#pragma unroll
            for (int k = 0; k < 6; k++) { sLs[6 * c + k] = z[k]; G.Ls[(size_t)i * 36 + 6 * c + k] = z[k]; }
        } else if (c < 6 + kPgCols) {
#pragma unroll
            for (int k = 0; k < 6; k++) { sY[6 * (c - 6) + k] = z[k]; G.Y[(size_t)i * (6 * kPgCols) + 6 * (c - 6) + k] = z[k]; yprev[k] = z[k]; }
        }
        if (c == 63) {
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int q = 0; q < 6; q++) G.Ld[(size_t)i * 36 + 6 * r + q] = q <= r ? A[6 * r + q] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const int e = c + 64 * u;
            if (e < kPgGram) {
                const int a = e / kPgCols, b = e - kPgCols * a;
                double s = sY[6 * a] * sY[6 * b];
#pragma unroll
                for (int k = 1; k < 6; k++) s += sY[6 * a + k] * sY[6 * b + k];
                acc[u] += s;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 3; u++) { const int e = c + 64 * u; if (e < kPgGram) G.gram[(size_t)blockIdx.x * kPgGram + e] = acc[u]; }
    if (!ok && c == 0) G.st->fail = 1;
}

__global__ __launch_bounds__(256) void k_pg_zero(const PgDev G) {
    if (G.st->done) return;
    const size_t nr = 6 * (size_t)G.tab->n_sep, n2 = nr * nr / 2;      // nr is even
    double2* R = reinterpret_cast<double2*>(G.red);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n2; e += (size_t)gridDim.x * blockDim.x) R[e] = double2{0.0, 0.0};
}

// block (p, q), p >= q, of the reduced system over the separators, and (block (p, p)) its right-hand side g_p minus the Schur terms, kept in delta's rows of the
// separators (and, for the blocked solve, in rhs).  One workgroup per entry of T.blk; every other block stays at k_pg_zero's zeros.
__global__ __launch_bounds__(64) void k_pg_reduced_assemble(const PgDev G) {
    if (G.st->done) return;
    const PgTables& T = *G.tab;
    const int nr = 6 * T.n_sep;
    const PgBlock B = T.blk[blockIdx.x];
    const int p = B.p, q = B.q;
    const int t = threadIdx.x;
    const int sp = T.sep[p], sq = T.sep[q];
    const bool seg_p = T.seg[p].first <= T.seg[p].last;                       // the segment to the right of separator p has nodes
    const bool seg_l = p > 0 && T.seg[p - 1].first <= T.seg[p - 1].last;      // ... to its left
    if (t < 36) {
        const int r = t / 6, c = t - 6 * r;
        double v = 0.0;
        if (p == q) {
            v = G.D[(size_t)sp * 36 + t];
            if (T.damping && r == c) v = pg_damped(v, T.damping, G.st->lambda);
            if (seg_p) v -= G.gram[(size_t)p * kPgGram + (1 + r) * kPgCols + (1 + c)];
            if (seg_l) v -= G.gram[(size_t)(p - 1) * kPgGram + (7 + r) * kPgCols + (7 + c)];
        } else if (p == q + 1) {
            if (T.seg[q].first <= T.seg[q].last) v = -G.gram[(size_t)q * kPgGram + (7 + r) * kPgCols + (1 + c)];
            else v = G.S[(size_t)sq * 36 + t];
        }
        for (int u = B.begin; u < B.end; u++) {      // in loop order
            const int en = T.blk_ent[u], l = en >> 1;
            v += (en & 1) ? G.LB[36 * l + 6 * c + r] : G.LB[36 * l + 6 * r + c];
        }
        G.red[(size_t)(6 * q + c) * nr + (6 * p + r)] = v;
    } else if (t < 42 && p == q) {
        const int r = t - 36;
        double v = G.g[(size_t)sp * 6 + r];
        if (seg_p) v -= G.gram[(size_t)p * kPgGram + (1 + r) * kPgCols];
        if (seg_l) v -= G.gram[(size_t)(p - 1) * kPgGram + (7 + r) * kPgCols];
        G.delta[(size_t)sp * 6 + r] = v;
        if (G.rhs) G.rhs[6 * p + r] = v;
    }
}

// a non-positive pivot ends the solve; the damped solve counts it as a rejected attempt: fail stays up until the next gate, the launches in between return at once
__device__ __forceinline__ void pg_pivot_failed(const PgTables& T, PgState& st) {
    if (T.damping) st.fail = 1; else { st.s.termination = LILI_LM_NUMERICAL_FAILURE; st.done = 1; }
}

__global__ __launch_bounds__(kPgWide) void k_pg_reduced_solve(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sy[kPgMaxReduced], srow[kPgMaxReduced];
    __shared__ double spiv;
    const PgTables& T = *G.tab;
    const int nr = 6 * T.n_sep, i = threadIdx.x;
    double* R = G.red;
    bool ok = G.st->fail == 0;
    if (i < nr) sy[i] = G.delta[(size_t)T.sep[i / 6] * 6 + i % 6];
    for (int j = 0; j < nr; j++) {
        if (i < j) srow[i] = R[(size_t)i * nr + j];      // row j of L
        __syncthreads();
        double s = 0.0;
        if (i >= j && i < nr) {
            s = R[(size_t)j * nr + i];
            for (int k = 0; k < j; k++) s -= R[(size_t)k * nr + i] * srow[k];
            if (i == j) spiv = s;
        }
        __syncthreads();
        const double piv = spiv;
        ok = ok && (piv > 0.0);
        const double l = sqrt(piv);
        if (i >= j && i < nr) R[(size_t)j * nr + i] = i == j ? l : s / l;
        __syncthreads();      // column j is in front of the next column's reads of it
    }
    __syncthreads();
    if (!ok) {
        if (i == 0) pg_pivot_failed(T, *G.st);
        return;
    }
    for (int j = 0; j < nr; j++) {      // L y = b
        const double yj = sy[j] / R[(size_t)j * nr + j];
        __syncthreads();
        if (i == j) sy[j] = yj;
        else if (i > j && i < nr) sy[i] -= R[(size_t)j * nr + i] * yj;
        __syncthreads();
    }
    for (int j = nr - 1; j >= 0; j--) {      // L^T x = y
        const double xj = sy[j] / R[(size_t)j * nr + j];
        __syncthreads();
        if (i == j) sy[j] = xj;
        else if (i < j) sy[i] -= R[(size_t)i * nr + j] * xj;
        __syncthreads();
    }
    if (i < nr) G.delta[(size_t)T.sep[i / 6] * 6 + i % 6] = -sy[i];
}

// ---- the blocked reduced solve (6 n_sep > kPgMaxReduced).  red holds the lower triangle column by column: element (r, c), r >= c, at red[c * nr + r].  Tile (i, j)
// covers rows i T .. and columns j T ..; the last tile row / column may overhang the matrix: its loads read zeros, its stores are masked.
__device__ __forceinline__ int pg_tri(const int r, const int c) { return r * (r + 1) / 2 + c; }      // the packed lower triangle of a tile in LDS, r >= c
// the lower triangle of the diagonal tile at o (m of its rows inside the matrix) into LDS and back, by the kThreads threads of the workgroup
template <int kThreads>
__device__ __forceinline__ void pg_load_tile(double* sL, const double* R, const int nr, const int o, const int m) {
    for (int e = threadIdx.x; e < m * m; e += kThreads) {
        const int c = e / m, r = e - c * m;
        if (r >= c) sL[pg_tri(r, c)] = R[(size_t)(o + c) * nr + (o + r)];
    }
}
template <int kThreads>
__device__ __forceinline__ void pg_store_tile(const double* sL, double* R, const int nr, const int o, const int m) {
    for (int e = threadIdx.x; e < m * m; e += kThreads) {
        const int c = e / m, r = e - c * m;
        if (r >= c) R[(size_t)(o + c) * nr + (o + r)] = sL[pg_tri(r, c)];
    }
}
constexpr int kPgPanelCols = 32;     // columns of its row a panel thread holds in registers at a time
static_assert(kPgTile % kPgPanelCols == 0, "panel columns");

// Tile column k: L_kk = chol(A_kk) in LDS (right-looking, element (r, c) takes its updates over j ascending), then y_k = L_kk^-1 b_k.  A non-positive pivot, or a
// segment's (PgState::fail), ends the solve.
__global__ __launch_bounds__(256) void k_pg_chol_diag(const PgDev G, const int k) {
    if (G.st->done) return;
    __shared__ double sL[kPgTile * (kPgTile + 1) / 2], sb[kPgTile];
    const int nr = 6 * G.tab->n_sep, o = k * kPgTile, m = min(kPgTile, nr - o), t = threadIdx.x;
    double* R = G.red;
    pg_load_tile<256>(sL, R, nr, o, m);
    if (t < m) sb[t] = G.rhs[o + t];
    bool ok = G.st->fail == 0;
    __syncthreads();
    // 16 x 16 threads over the triangle: thread (ty, tx) owns the elements (r, c) = (tx + 16 b, ty + 16 a) with c <= r < m, at fixed places of the packed triangle
    constexpr int kSpan = kPgTile / 16;
    int trr[kSpan], cc[kSpan];
#pragma unroll
    for (int u = 0; u < kSpan; u++) { const int r = (t & 15) + 16 * u; trr[u] = r < m ? r * (r + 1) / 2 : -1; cc[u] = (t >> 4) + 16 * u; }
    for (int j = 0; j < m && ok; j++) {
        const double piv = sL[pg_tri(j, j)];
        ok = piv > 0.0;      // (the same value in every thread)
        const double l = sqrt(piv);
        for (int r = j + 1 + t; r < m; r += 256) sL[pg_tri(r, j)] = sL[pg_tri(r, j)] / l;
        __syncthreads();
        if (t == 0) sL[pg_tri(j, j)] = l;      // (nobody reads it before the factor is complete)
        // the trailing update of column j: a thread's reads first, then its writes
        double lc[kSpan], lr[kSpan], cur[kSpan][kSpan];
#pragma unroll
        for (int u = 0; u < kSpan; u++) {
            lc[u] = cc[u] > j && cc[u] < m ? sL[pg_tri(cc[u], j)] : 0.0;
            lr[u] = trr[u] >= 0 && (t & 15) + 16 * u > j ? sL[trr[u] + j] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < kSpan; a++)
#pragma unroll
            for (int b = 0; b < kSpan; b++) cur[a][b] = cc[a] > j && trr[b] >= 0 && (t & 15) + 16 * b >= cc[a] ? sL[trr[b] + cc[a]] : 0.0;
#pragma unroll
        for (int a = 0; a < kSpan; a++)
#pragma unroll
            for (int b = 0; b < kSpan; b++)
                if (cc[a] > j && trr[b] >= 0 && (t & 15) + 16 * b >= cc[a]) sL[trr[b] + cc[a]] = cur[a][b] - lr[b] * lc[a];
        __syncthreads();
    }
    if (!ok) {
        if (t == 0) pg_pivot_failed(*G.tab, *G.st);
        return;
    }
    pg_store_tile<256>(sL, R, nr, o, m);
    for (int j = 0; j < m; j++) {      // L y = b
        const double yj = sb[j] / sL[pg_tri(j, j)];
        __syncthreads();
        if (t == j) sb[j] = yj;
        else if (t > j && t < m) sb[t] -= sL[pg_tri(t, j)] * yj;
        __syncthreads();
    }
    if (t < m) G.rhs[o + t] = sb[t];
}

// Row tile i = k + 1 + blockIdx.x of tile column k, one thread per row: x L_kk^T = a by forward substitution over the columns (the row stays in memory, in place), then
// b_i -= L_ik y_k
__global__ __launch_bounds__(128) void k_pg_chol_panel(const PgDev G, const int k) {
    if (G.st->done || G.st->fail) return;      // (fail without done: a rejected attempt of the damped solve)
    __shared__ double sL[kPgTile * (kPgTile + 1) / 2], sy[kPgTile];
    const int nr = 6 * G.tab->n_sep, o = k * kPgTile, i = k + 1 + blockIdx.x, t = threadIdx.x;
    double* R = G.red;
    pg_load_tile<128>(sL, R, nr, o, kPgTile);      // tile column k is not the last one: it is whole
    if (t < kPgTile) sy[t] = G.rhs[o + t];
    __syncthreads();
    const int row = i * kPgTile + t;
    if (t >= kPgTile || row >= nr) return;
    double* X = R + (size_t)o * nr + row;      // element c of the row at X[c * nr]
    double b = G.rhs[row];
    for (int c0 = 0; c0 < kPgTile; c0 += kPgPanelCols) {      // kPgPanelCols columns at a time in registers; every element sums over q ascending
        double v[kPgPanelCols];
#pragma unroll
        for (int c = 0; c < kPgPanelCols; c++) v[c] = X[(size_t)(c0 + c) * nr];
#pragma unroll 4
        for (int q = 0; q < c0; q++) {
            const double xq = X[(size_t)q * nr];
#pragma unroll
            for (int c = 0; c < kPgPanelCols; c++) v[c] -= xq * sL[pg_tri(c0 + c, q)];
        }
#pragma unroll
        for (int c = 0; c < kPgPanelCols; c++) {
#pragma unroll
            for (int q = 0; q < c; q++) v[c] -= v[q] * sL[pg_tri(c0 + c, c0 + q)];
            v[c] = v[c] / sL[pg_tri(c0 + c, c0 + c)];
        }
#pragma unroll
        for (int c = 0; c < kPgPanelCols; c++) { X[(size_t)(c0 + c) * nr] = v[c]; b -= v[c] * sy[c0 + c]; }
    }
    G.rhs[row] = b;
}

// Lower-triangle tile (i, j), k < j <= i, of the trailing matrix: A_ij -= L_ik L_jk^T.  The matrix instruction's rows are the tile's COLUMNS (operand A = L_jk), its
// columns the tile's rows (operand B = L_ik^T), so that a lane's 16 neighbours store 16 consecutive doubles.  Four waves, each a 48 x 48 quarter as 3 x 3
// instruction tiles; the f64 result map: column = lane & 15, row = (lane >> 4) + 4 reg.  The sum over the kPgTile columns of tile column k runs in ascending order.
typedef double pg_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_pg_chol_update(const PgDev G, const int k) {
    if (G.st->done || G.st->fail) return;      // (fail without done: a rejected attempt of the damped solve)
    __shared__ double sA[kPgTileK * kPgTileLd], sB[kPgTileK * kPgTileLd];
    const int nr = 6 * G.tab->n_sep, t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int b = blockIdx.x;
    int ii = (int)((sqrtf(8.f * (float)b + 1.f) - 1.f) * 0.5f);
    while (ii * (ii + 1) / 2 > b) ii--;
    while ((ii + 1) * (ii + 2) / 2 <= b) ii++;
    const int i = k + 1 + ii, j = k + 1 + (b - ii * (ii + 1) / 2);
    const bool live = !(i == j && wm > wn);      // a quarter above the diagonal of a diagonal tile
    double* R = G.red;
    pg_d4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[a][c] = pg_d4{0.0, 0.0, 0.0, 0.0};
    // the operands of a chunk travel memory -> registers -> LDS; the next chunk's loads are in flight while this one is multiplied
    constexpr int kPer = kPgTileK * kPgTile / 256;
    static_assert(kPgTileK * kPgTile % 256 == 0, "whole rounds of the 256 threads");
    double pa[kPer], pb[kPer];
    auto fetch = [&](const int kc) {
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int e = t + 256 * u, kk = e / kPgTile, r = e - kk * kPgTile;
            const size_t col = (size_t)(k * kPgTile + kc + kk) * nr;
            const int rj = j * kPgTile + r, ri = i * kPgTile + r;
            pa[u] = rj < nr ? R[col + rj] : 0.0;
            pb[u] = ri < nr ? R[col + ri] : 0.0;
        }
    };
    fetch(0);
    for (int kc = 0; kc < kPgTile; kc += kPgTileK) {
        __syncthreads();      // the previous chunk has been read
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int e = t + 256 * u, kk = e / kPgTile, r = e - kk * kPgTile;
            sA[kk * kPgTileLd + r] = pa[u];
            sB[kk * kPgTileLd + r] = pb[u];
        }
        __syncthreads();
        if (kc + kPgTileK < kPgTile) fetch(kc + kPgTileK);
        if (live) {
#pragma unroll
            for (int k4 = 0; k4 < kPgTileK; k4 += 4) {
                const int kq = (k4 + (lane >> 4)) * kPgTileLd + (lane & 15);
                double a[3], c[3];
#pragma unroll
                for (int u = 0; u < 3; u++) { a[u] = sA[kq + wm * 48 + 16 * u]; c[u] = sB[kq + wn * 48 + 16 * u]; }
#pragma unroll
                for (int u = 0; u < 3; u++)
#pragma unroll
                    for (int v = 0; v < 3; v++) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], c[v], acc[u][v], 0, 0, 0);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = 0; v < 3; v++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int c = j * kPgTile + wm * 48 + 16 * u + (lane >> 4) + 4 * reg, r = i * kPgTile + wn * 48 + 16 * v + (lane & 15);
                if (r < nr && c < nr && r >= c) { double* e = R + (size_t)c * nr + r; *e = *e - acc[u][v][reg]; }
            }
}

// Tile row i (launched last row first), workgroup kb = blockIdx.x <= i: every workgroup solves L_ii^T x_i = y_i in LDS on the same bits; workgroup kb < i takes
// L_(i, kb)^T x_i off y_kb (its own piece of rhs), workgroup i writes the separators' step -x_i
__global__ __launch_bounds__(128) void k_pg_chol_back(const PgDev G, const int i) {
    if (G.st->done || G.st->fail) return;      // (fail without done: a rejected attempt of the damped solve)
    __shared__ double sL[kPgTile * (kPgTile + 1) / 2], sx[kPgTile];
    const PgTables& T = *G.tab;
    const int nr = 6 * T.n_sep, o = i * kPgTile, m = min(kPgTile, nr - o), t = threadIdx.x, kb = blockIdx.x;
    const double* R = G.red;
    pg_load_tile<128>(sL, R, nr, o, m);
    if (t < m) sx[t] = G.rhs[o + t];
    __syncthreads();
    for (int c = m - 1; c >= 0; c--) {
        const double xc = sx[c] / sL[pg_tri(c, c)];
        __syncthreads();
        if (t == c) sx[c] = xc;
        else if (t < c) sx[t] -= sL[pg_tri(c, t)] * xc;
        __syncthreads();
    }
    if (kb == i) {
        if (t < m) G.delta[(size_t)T.sep[(o + t) / 6] * 6 + (o + t) % 6] = -sx[t];
        return;
    }
    if (t >= kPgTile) return;
    const int col = kb * kPgTile + t;      // tile column kb < i is whole
    const double* Lc = R + (size_t)col * nr + o;
    double y = G.rhs[col];
    for (int r = 0; r < m; r++) y -= Lc[r] * sx[r];
    G.rhs[col] = y;
}

__global__ __launch_bounds__(64) void k_pg_backsub(const PgDev G) {
    if (G.st->done || G.st->fail) return;      // (fail without done: a rejected attempt of the damped solve)
    const PgTables& T = *G.tab;
    const PgSeg sg = T.seg[blockIdx.x];
    double xl[6], xr[6], xn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; k++) { xl[k] = G.delta[(size_t)sg.left * 6 + k]; xr[k] = sg.right >= 0 ? G.delta[(size_t)sg.right * 6 + k] : 0.0; }
    for (int i = sg.last; i >= sg.first; i--) {
        const double* Y = G.Y + (size_t)i * (6 * kPgCols);
        const double* Ls = G.Ls + (size_t)i * 36;
        const double* Ld = G.Ld + (size_t)i * 36;
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            double s = Y[k];
#pragma unroll
            for (int m = 0; m < 6; m++) s += Y[6 * (1 + m) + k] * xl[m];
#pragma unroll
            for (int m = 0; m < 6; m++) s += Y[6 * (7 + m) + k] * xr[m];
            s = -s;
            if (i < sg.last) {
#pragma unroll
                for (int m = 0; m < 6; m++) s -= Ls[6 * m + k] * xn[m];
            }
            x[k] = s;
        }
        pg_back6(Ld, x);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 6; k++) G.delta[(size_t)i * 6 + k] = x[k];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) xn[k] = x[k];
    }
}

// the candidate X (+) delta into Xn, |delta|inf and the candidate's cost, in a fixed order; every thread gets both
__device__ __forceinline__ void pg_candidate(const PgDev& G, double* sh, double& smax_out, double& cost_out) {
    const PgTables& T = *G.tab;
    const int t = threadIdx.x, n = T.n;
    double smax = 0.0;
    for (int i = t; i < n; i += kPgWide) {
        const double* x = G.X + 7 * (size_t)i;
        const double* dl = G.delta + 6 * (size_t)i;
        double* o = G.Xn + 7 * (size_t)i;
        const dq q = pg_quat(x);
        const d3 p = d3{x[0], x[1], x[2]} + qrot(q, d3{dl[3], dl[4], dl[5]});
        const double t2 = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2];
        double sc = 0.5, cw = 1.0;
        if (t2 > 0.0) { const double th = sqrt(t2); sc = sin(0.5 * th) / th; cw = cos(0.5 * th); }
        const dq qn = qmul(q, dq{cw, sc * dl[0], sc * dl[1], sc * dl[2]});
        const double nq = sqrt(((qn.w * qn.w + qn.x * qn.x) + qn.y * qn.y) + qn.z * qn.z);
        o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = qn.w / nq; o[4] = qn.x / nq; o[5] = qn.y / nq; o[6] = qn.z / nq;
#pragma unroll
        for (int k = 0; k < 6; k++) smax = fmax(smax, fabs(dl[k]));
    }
    smax_out = pg_block_reduce<PgMax>(smax, sh);      // (its barriers also put the candidate in front of the reads below)
    double c = 0.0;
    for (int f = t; f < n + T.n_loops; f += kPgWide) c += pg_factor_cost(T, G.Xn, G.meas, f);
    cost_out = 0.5 * pg_block_reduce<PgSum>(c, sh);
}
// thread 0, an accepted step: the new cost, then the stop tests (parameter tolerance, function tolerance, the iteration cap)
__device__ __forceinline__ void pg_accept_step(PgState& st, const PgTables& T, const int it, const double cost, const double new_cost, const double smax) {
    st.cost = new_cost; st.s.final_cost = new_cost;
    if (smax <= T.parameter_tolerance) { st.s.termination = LILI_LM_PARAMETER_TOLERANCE; st.done = 1; }
    else if (fabs(cost - new_cost) <= T.function_tolerance * cost) { st.s.termination = LILI_LM_FUNCTION_TOLERANCE; st.done = 1; }
    else if (it + 1 >= T.max_iter) { st.s.termination = LILI_LM_MAX_ITERATIONS; st.done = 1; }
}
// X <- the candidate, by the whole workgroup
__device__ __forceinline__ void pg_commit(const PgDev& G, const int n) {
    for (int e = threadIdx.x; e < 7 * n; e += kPgWide) G.X[e] = G.Xn[e];
}

__global__ __launch_bounds__(kPgWide) void k_pg_retract_cost(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sh[kPgWide];
    __shared__ int s_accept;
    const int n = G.tab->n;
    double smax, new_cost;
    pg_candidate(G, sh, smax, new_cost);
    if (threadIdx.x == 0) {
        PgState& st = *G.st;
        const int it = st.s.iterations;
        const double cost = st.cost;
        if (it < LILI_PG_MAX_LOG) { st.s.cost[it] = new_cost; st.s.step_inf[it] = smax; }
        st.s.iterations = it + 1;
        int accept = 0;
        if (!(new_cost <= cost)) { st.s.termination = LILI_PG_COST_INCREASED; st.done = 1; }
        else { accept = 1; pg_accept_step(st, *G.tab, it, cost, new_cost, smax); }
        s_accept = accept;
    }
    __syncthreads();
    if (s_accept) pg_commit(G, n);
}

// The tail of an attempt of lili_pose_graph_solve_lm: the candidate and its cost, then the decision.  Accepted (new cost <= cost): X <- candidate, lambda falls by
// the factor down to its lower bound, the stop tests of k_pg_retract_cost.  Rejected (a higher cost, or a non-positive pivot on the way: PgState::fail, no
// candidate is formed): X stays, lambda rises by the factor, past its upper bound the solve ends.
__global__ __launch_bounds__(kPgWide) void k_pg_lm_decide(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sh[kPgWide];
    __shared__ int s_accept;
    const PgTables& T = *G.tab;
    const int n = T.n;
    const bool failed = G.st->fail != 0;
    double smax = 0.0, new_cost = G.st->cost;
    if (!failed) pg_candidate(G, sh, smax, new_cost);
    __syncthreads();      // every thread has read the state
    if (threadIdx.x == 0) {
        PgState& st = *G.st;
        const int it = st.s.iterations;
        const double cost = st.cost, lambda = st.lambda;
        const int accept = !failed && new_cost <= cost;
        if (it < LILI_PG_MAX_LOG) { st.s.cost[it] = new_cost; st.s.step_inf[it] = smax; st.lambda_log[it] = lambda; st.accepted[it] = accept; }
        st.s.iterations = it + 1;
        if (accept) {
            st.steps_accepted++;
            st.lambda = fmax(lambda / st.lambda_factor, st.lambda_lower);
            pg_accept_step(st, T, it, cost, new_cost, smax);
        } else {
            st.steps_rejected++;
            st.lambda = lambda * st.lambda_factor;
            if (st.lambda > st.lambda_upper) { st.s.termination = LILI_PG_LAMBDA_LIMIT; st.done = 1; }
            else if (it + 1 >= T.max_iter) { st.s.termination = LILI_LM_MAX_ITERATIONS; st.done = 1; }
        }
        s_accept = accept;
    }
    __syncthreads();
    if (s_accept) pg_commit(G, n);
}

// lili_pose_graph_loop_status: d^2 and the weight of loops first .. first + n - 1 at the estimates, the linearisation's arithmetic
__global__ __launch_bounds__(256) void k_pg_loop_status(const PgDev G, const int first, const int n, double* __restrict__ out) {
    const PgTables& T = *G.tab;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = T.n + first + i;
    const PgFactorIn F = pg_factor(T, G.X, G.meas, f);
    double e[6], scale;
    dq qab, qe; d3 d;
    pg_error(F.pa, F.qa, F.pb, F.qb, F.Z, e, qab, d, qe);
    const double d2 = pg_whitened_d2(F, e);
    const int loss = pg_loss_of(T, f, scale);
    out[i] = d2;
    out[n + i] = loss == LILI_PG_LOSS_NONE ? 1.0 : pg_loss_weight(loss, scale, d2);
}

// ---- marginal covariances (lili_pose_graph_marginals): the inverse-side passes behind one iteration's factorisation.  With the interior nodes I in front of the
// separators s, H = [A_II E; E^T A_ss], A_II = L_II L_II^T (Ld, Ls), Y_E = L_II^-1 E (Y), S = A_ss - Y_E^T Y_E = L L^T (red):
//   Sigma_ss = S^-1,   W = -L_II^-T Y_E,   Sigma_Is = W Sigma_ss,   Sigma_II = A_II^-1 + W Sigma_ss W^T.
// A node's rows of W are non-zero only in the columns of the (at most two) separators that bound its segment, and A_II^-1 is block diagonal by segment.
//
// k_pg_marg_inverse: workgroup p = the six columns of S^-1 that belong to separator p, thread (q, r) = column q, the rows r mod kPgTile.  L x = e from the tile that
// holds row 6 p (x is zero above it), then L^T x = y back down to that tile: only the rows >= 6 p are wanted, the others follow by symmetry.  Tile by tile: the diagonal
// tile in LDS, its triangular solve there, then every row below (forward) / above (backward) takes its 96 products, summed over the tile in ascending order.  Every
// element of x has one owner for the whole launch, which reads back only what it wrote itself.
constexpr int kPgInvThreads = 6 * kPgTile;
static_assert(kPgInvThreads % 64 == 0 && kPgInvThreads <= 1024, "whole waves, one workgroup");
__global__ __launch_bounds__(kPgInvThreads) void k_pg_marg_inverse(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sL[kPgTile * (kPgTile + 1) / 2], sx[6 * kPgTile];
    const int nr = 6 * G.tab->n_sep, p = blockIdx.x, t = threadIdx.x, q = t / kPgTile, r = t - q * kPgTile;
    const int nt = (nr + kPgTile - 1) / kPgTile, k0 = 6 * p / kPgTile;
    const double* R = G.red;
    double* X = G.sinv + (size_t)(6 * p + q) * nr;      // this thread's column
    const double* xq = sx + q * kPgTile;
    for (int kt = k0; kt < nt; kt++) {      // L y = e
        const int o = kt * kPgTile, m = min(kPgTile, nr - o);
        __syncthreads();      // the previous tile's reads of sL and sx
        pg_load_tile<kPgInvThreads>(sL, R, nr, o, m);
        if (r < m) sx[t] = kt == k0 ? (o + r == 6 * p + q ? 1.0 : 0.0) : X[o + r];
        __syncthreads();
        for (int c = 0; c < m; c++) {
            const double xc = xq[c] / sL[pg_tri(c, c)];
            __syncthreads();
            if (r == c) sx[t] = xc;
            else if (r > c && r < m) sx[t] -= sL[pg_tri(r, c)] * xc;
            __syncthreads();
        }
        if (r < m) X[o + r] = sx[t];
        for (int row = o + kPgTile + r; row < nr; row += kPgTile) {      // (rows below: this tile column is whole)
            const double* Lr = R + (size_t)o * nr + row;
            double s = kt == k0 ? 0.0 : X[row];
#pragma unroll 8
            for (int c = 0; c < kPgTile; c++) s -= Lr[(size_t)c * nr] * xq[c];
            X[row] = s;
        }
    }
    for (int kt = nt - 1; kt >= k0; kt--) {      // L^T x = y
        const int o = kt * kPgTile, m = min(kPgTile, nr - o);
        __syncthreads();
        pg_load_tile<kPgInvThreads>(sL, R, nr, o, m);
        if (r < m) sx[t] = X[o + r];
        __syncthreads();
        for (int c = m - 1; c >= 0; c--) {
            const double xc = xq[c] / sL[pg_tri(c, c)];
            __syncthreads();
            if (r == c) sx[t] = xc;
            else if (r < c) sx[t] -= sL[pg_tri(c, r)] * xc;
            __syncthreads();
        }
        if (r < m) X[o + r] = sx[t];
        for (int row = k0 * kPgTile + r; row < o; row += kPgTile) {      // y_row -= L(o .., row)^T x_tile
            const double* Lc = R + (size_t)row * nr + o;
            double s = X[row];
#pragma unroll 8
            for (int rr = 0; rr < m; rr++) s -= Lc[rr] * xq[rr];
            X[row] = s;
        }
    }
}

// element (a, b) of the reduced inverse, from its lower triangle: the same bits for (a, b) and (b, a)
__device__ __forceinline__ double pg_sinv(const double* X, const int nr, const int a, const int b) { return a >= b ? X[(size_t)b * nr + a] : X[(size_t)a * nr + b]; }

// One wave per segment, last node first.  Lanes 0 .. 11: a column of W_i = Ld_i^-T (-Y_E,i - Ls_i^T W_(i+1)).  Lanes 12 .. 17: a column of the segment's own inverse
// block P_i = Ld_i^-T (I + Ls_i^T P_(i+1) Ls_i) Ld_i^-1, made symmetric by averaging.  Lanes 0 .. 35: entry (r, c) of Sigma_ii = P_i + W_i Sigma_sep W_i^T, Sigma_sep
// the 12 x 12 joint block of the segment's two separators (neighbours in the reduced order; the chain's last segment has one, the other half is zero); entries (r, c)
// and (c, r) evaluate the same expression.  Lanes 0 .. 35 also write the left separator's own block.
__global__ __launch_bounds__(64) void k_pg_marg_segments(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sS[144], sW[72], sP[36], sPn[36];
    const PgTables& T = *G.tab;
    const int k = blockIdx.x, c = threadIdx.x, nr = 6 * T.n_sep;
    const PgSeg sg = T.seg[k];
    for (int e = c; e < 144; e += 64) {
        const int a = e / 12, b = e - 12 * a;
        sS[e] = (sg.right >= 0 || (a < 6 && b < 6)) ? pg_sinv(G.sinv, nr, 6 * k + a, 6 * k + b) : 0.0;
    }
    if (c < 36) sP[c] = 0.0;
    __syncthreads();
    if (c < 36) G.cov[(size_t)sg.left * 36 + c] = sS[12 * (c / 6) + c % 6];
    double wn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = sg.last; i >= sg.first; i--) {
        const double* Ld = G.Ld + (size_t)i * 36;
        const double* Ls = G.Ls + (size_t)i * 36;      // L block (i + 1, i), row by row
        const bool tail = i < sg.last;
        if (c < 12) {
            const double* Y = G.Y + (size_t)i * (6 * kPgCols) + 6 * (1 + c);
            double x[6];
#pragma unroll
            for (int kk = 0; kk < 6; kk++) {
                double s = -Y[kk];
                if (tail) {
#pragma unroll
                    for (int m = 0; m < 6; m++) s -= Ls[6 * m + kk] * wn[m];
                }
                x[kk] = s;
            }
            pg_back6(Ld, x);
#pragma unroll
            for (int kk = 0; kk < 6; kk++) { sW[6 * c + kk] = x[kk]; G.W[(size_t)i * 72 + 6 * c + kk] = x[kk]; wn[kk] = x[kk]; }
        } else if (c < 18) {
            const int cc = c - 12;
            double u[6], x[6];
#pragma unroll
            for (int kk = 0; kk < 6; kk++) u[kk] = kk == cc ? 1.0 : 0.0;
            pg_fwd6(Ld, u);      // u = Ld^-1 e_cc
            if (tail) {
                double v[6], pv[6];
#pragma unroll
                for (int rr = 0; rr < 6; rr++) {
                    double s = Ls[6 * rr] * u[0];
#pragma unroll
                    for (int m = 1; m < 6; m++) s += Ls[6 * rr + m] * u[m];
                    v[rr] = s;
                }
#pragma unroll
                for (int rr = 0; rr < 6; rr++) {
                    double s = sP[6 * rr] * v[0];
#pragma unroll
                    for (int m = 1; m < 6; m++) s += sP[6 * rr + m] * v[m];
                    pv[rr] = s;
                }
#pragma unroll
                for (int kk = 0; kk < 6; kk++) {
                    double s = u[kk];
#pragma unroll
                    for (int rr = 0; rr < 6; rr++) s += Ls[6 * rr + kk] * pv[rr];
                    x[kk] = s;
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < 6; kk++) x[kk] = u[kk];
            }
            pg_back6(Ld, x);
#pragma unroll
            for (int kk = 0; kk < 6; kk++) sPn[6 * kk + cc] = x[kk];
        }
        __syncthreads();      // P_(i+1) has been read, the raw columns of P_i are in place
        if (c < 36) { const int rr = c / 6, qq = c - 6 * rr; sP[c] = 0.5 * (sPn[6 * rr + qq] + sPn[6 * qq + rr]); }
        __syncthreads();
        if (c < 36) {
            const int rr = c / 6, qq = c - 6 * rr, hi = max(rr, qq), lo = min(rr, qq);
            double s = sP[6 * hi + lo];
            for (int a = 0; a < 12; a++) {
                double ta = sS[12 * a] * sW[lo];
#pragma unroll
                for (int b = 1; b < 12; b++) ta += sS[12 * a + b] * sW[6 * b + lo];
                s += sW[6 * a + hi] * ta;
            }
            G.cov[(size_t)i * 36 + c] = s;
            G.P[(size_t)i * 36 + c] = sP[c];
        }
        __syncthreads();      // sW and sP have been read
    }
}

// the separator at or in front of node i: the largest p with sep[p] <= i (sep[0] = 0)
__device__ __forceinline__ int pg_sep_at(const PgTables& T, const int i) {
    int lo = 0, hi = T.n_sep - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (T.sep[mid] <= i) lo = mid; else hi = mid - 1; }
    return lo;
}

// One wave per pair (i, j): Sigma(lo, hi) of the smaller and the larger id, written as it is or transposed, so that the two orders of a pair are transposes bit for
// bit; i == j copies the node's diagonal block.  Sigma(lo, hi) = Z + W_lo M W_hi^T: W of a separator = the identity on its own six columns, M = the blocks of the
// reduced inverse between the nodes' separators, Z = the segment's own inverse block (lo, hi) when both are interior nodes of one segment, from the larger node's P
// by Z_(k, hi) = -Ld_k^-T Ls_k^T Z_(k+1, hi) (lanes 0 .. 5, a column each; at most LILI_PG_SEGMENT - 2 steps).
__global__ __launch_bounds__(64) void k_pg_marg_pairs(const PgDev G) {
    if (G.st->done) return;
    __shared__ double sM[144], sWl[72], sWh[72], sZ[36];
    const PgTables& T = *G.tab;
    const int c = threadIdx.x, nr = 6 * T.n_sep;
    const int i = G.pairs[2 * blockIdx.x], j = G.pairs[2 * blockIdx.x + 1];
    double* out = G.cross + (size_t)blockIdx.x * 36;
    if (i == j) {
        if (c < 36) out[c] = G.cov[(size_t)i * 36 + c];
        return;
    }
    const int lo = min(i, j), hi = max(i, j), pl = pg_sep_at(T, lo), ph = pg_sep_at(T, hi);
    const bool il = T.sep[pl] != lo, ih = T.sep[ph] != hi;      // interior nodes of segments pl / ph
    for (int e = c; e < 72; e += 64) {
        const int a = e / 6, rr = e - 6 * a;
        sWl[e] = il ? G.W[(size_t)lo * 72 + e] : (a == rr ? 1.0 : 0.0);
        sWh[e] = ih ? G.W[(size_t)hi * 72 + e] : (a == rr ? 1.0 : 0.0);
    }
    for (int e = c; e < 144; e += 64) {
        const int a = e / 12, b = e - 12 * a;
        const bool va = a < 6 || (il && pl + 1 < T.n_sep), vb = b < 6 || (ih && ph + 1 < T.n_sep);
        sM[e] = va && vb ? pg_sinv(G.sinv, nr, 6 * pl + a, 6 * ph + b) : 0.0;
    }
    if (c < 36) sZ[c] = 0.0;
    __syncthreads();
    if (il && ih && pl == ph && c < 6) {
        double v[6];
#pragma unroll
        for (int rr = 0; rr < 6; rr++) v[rr] = G.P[(size_t)hi * 36 + 6 * rr + c];
        for (int kn = hi - 1; kn >= lo; kn--) {
            const double* Ls = G.Ls + (size_t)kn * 36;
            double x[6];
#pragma unroll
            for (int kk = 0; kk < 6; kk++) {
                double s = Ls[kk] * v[0];
#pragma unroll
                for (int rr = 1; rr < 6; rr++) s += Ls[6 * rr + kk] * v[rr];
                x[kk] = -s;
            }
            pg_back6(G.Ld + (size_t)kn * 36, x);
#pragma unroll
            for (int kk = 0; kk < 6; kk++) v[kk] = x[kk];
        }
#pragma unroll
        for (int rr = 0; rr < 6; rr++) sZ[6 * rr + c] = v[rr];
    }
    __syncthreads();
    if (c < 36) {
        const int rr = c / 6, qq = c - 6 * rr;
        double s = sZ[c];
        for (int a = 0; a < 12; a++) {
            double ta = sM[12 * a] * sWh[qq];
#pragma unroll
            for (int b = 1; b < 12; b++) ta += sM[12 * a + b] * sWh[6 * b + qq];
            s += sWl[6 * a + rr] * ta;
        }
        out[i < j ? c : 6 * qq + rr] = s;
    }
}

}  // namespace lili

namespace {

struct PoseGraphState : ExtState {
    int n = 0, n_loops = 0;
    std::vector<PgLoop> loops;
    DevBuf X, Xn, meas, tab, tabv, st, stage, fr, fJ, lw, g, D, S, LB, Ld, Ls, Y, gram, red, delta, rhs;
    DevBuf sinv, W, Pm, cov, cross, pairs;      // lili_pose_graph_marginals only
    PinBuf h_tab, h_io, h_pairs;
    Event ev0, ev1;
    float last_ms = -1.f;
    // the host copy of the state, behind the fixed tables in the page-locked block: a call's read-back lands there
    PgState* host_state() const { return reinterpret_cast<PgState*>(h_tab.as<PgTables>() + 1); }
    // the graph itself is allocated once at the caps (3.7 MB): it has to outlive every call
    int persist(lili_ctx* ctx) {
        HIPCHK(X.ensure(sizeof(double) * 7 * kPgMaxNodes));
        HIPCHK(meas.ensure(sizeof(double) * 7 * kPgMaxNodes));
        HIPCHK(tab.ensure(sizeof(PgTables)));
        HIPCHK(st.ensure(sizeof(PgState)));
        return LILI_OK;
    }
    // the work arrays of an evaluation (solve: and of the elimination) for the current sizes.  The reduced system is dense: 8 (6 n_sep)^2 bytes, 4.7 MB at the
    // default caps (128 separators), 1.3 GB at LILI_PG_MAX_LOOPS_EXT loops (2112 separators, 12 672 unknowns)
    int work(lili_ctx* ctx, int n_sep, bool solve) {
        const size_t N = (size_t)n, F = (size_t)n + (size_t)n_loops, d = sizeof(double);
        HIPCHK(fr.ensure(F * 6 * d)); HIPCHK(fJ.ensure(F * 72 * d)); HIPCHK(lw.ensure((size_t)std::max(n_loops, 1) * 2 * d));
        HIPCHK(g.ensure(N * 6 * d)); HIPCHK(D.ensure(N * 36 * d)); HIPCHK(S.ensure(N * 36 * d)); HIPCHK(LB.ensure((size_t)std::max(n_loops, 1) * 36 * d));
        if (solve) {
            HIPCHK(Xn.ensure(N * 7 * d));
            HIPCHK(Ld.ensure(N * 36 * d)); HIPCHK(Ls.ensure(N * 36 * d)); HIPCHK(Y.ensure(N * 6 * kPgCols * d));
            HIPCHK(gram.ensure((size_t)n_sep * kPgGram * d));
            HIPCHK(red.ensure((size_t)36 * n_sep * n_sep * d));
            HIPCHK(delta.ensure(N * 6 * d));
            if (6 * n_sep > kPgMaxReduced) HIPCHK(rhs.ensure((size_t)6 * n_sep * d));
        }
        return LILI_OK;
    }
    // what the inverse-side passes add, allocated by the first lili_pose_graph_marginals: a second dense array of the reduced system's size, W and P per node, the outputs
    int work_marginals(lili_ctx* ctx, int n_sep, int n_pairs) {
        const size_t N = (size_t)n, d = sizeof(double);
        HIPCHK(sinv.ensure((size_t)36 * n_sep * n_sep * d));
        HIPCHK(W.ensure(N * 72 * d)); HIPCHK(Pm.ensure(N * 36 * d)); HIPCHK(cov.ensure(N * 36 * d));
        HIPCHK(cross.ensure((size_t)std::max(n_pairs, 1) * 36 * d)); HIPCHK(pairs.ensure((size_t)std::max(n_pairs, 1) * 2 * sizeof(int32_t)));
        return LILI_OK;
    }
    PgDev dev(int n_sep) const {
        PgDev G{};
        G.tab = tab.as<PgTables>(); G.st = st.as<PgState>();
        G.X = X.as<double>(); G.Xn = Xn.as<double>(); G.meas = meas.as<double>();
        G.fr = fr.as<double>(); G.fJ = fJ.as<double>(); G.lw = lw.as<double>(); G.g = g.as<double>(); G.D = D.as<double>(); G.S = S.as<double>(); G.LB = LB.as<double>();
        G.Ld = Ld.as<double>(); G.Ls = Ls.as<double>(); G.Y = Y.as<double>(); G.gram = gram.as<double>(); G.red = red.as<double>(); G.delta = delta.as<double>();
        G.rhs = 6 * n_sep > kPgMaxReduced ? rhs.as<double>() : nullptr;
        G.sinv = sinv.as<double>(); G.W = W.as<double>(); G.P = Pm.as<double>(); G.cov = cov.as<double>(); G.cross = cross.as<double>(); G.pairs = pairs.as<int>();
        return G;
    }
};
PoseGraphState* pg_of(lili_ctx* ctx) { return ext_of<PoseGraphState>(ctx, lili_ctx::kExtPoseGraph); }

// the norm of a pose's quaternion; false where it is more than 1e-6 from 1 (or not a number)
bool unit_quaternion(const double* pose, double* nq) {
    const double* q = pose + 3;
    *nq = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    return std::fabs(*nq - 1.0) <= 1e-6;
}
// n poses: finite, quaternions within 1e-6 of unit norm; out (scratch) = the poses with the quaternions normalised
int check_poses(lili_ctx* ctx, const char* who, const double* poses, size_t n, double* out) {
    ARGCHK(finite_n(poses, 7 * n), std::string(who) + ": an input is not finite");
    for (size_t i = 0; i < n; i++) {
        const double* p = poses + 7 * i;
        double nq;
        ARGCHK(unit_quaternion(p, &nq), std::string(who) + ": a quaternion is more than 1e-6 from unit norm");
        for (int k = 0; k < 3; k++) out[7 * i + k] = p[k];
        for (int k = 3; k < 7; k++) out[7 * i + k] = p[k] / nq;
    }
    return LILI_OK;
}
int check_options(lili_ctx* ctx, const lili_pg_options* options, lili_pg_options* opt) {
    if (options) *opt = *options; else lili_pg_default_options(opt);
    ARGCHK(opt->max_iterations >= 1 && opt->max_iterations <= 1000, "pose_graph: max_iterations must be in 1..1000");
    ARGCHK(std::isfinite(opt->function_tolerance) && std::isfinite(opt->gradient_tolerance) && std::isfinite(opt->parameter_tolerance) && opt->function_tolerance >= 0 &&
           opt->gradient_tolerance >= 0 && opt->parameter_tolerance >= 0, "pose_graph: a tolerance is negative or not finite");
    for (int k = 0; k < 6; k++)
        ARGCHK(std::isfinite(opt->prior_var[k]) && std::isfinite(opt->odom_var[k]) && opt->prior_var[k] > 0 && opt->odom_var[k] > 0, "pose_graph: a variance is not positive and finite");
    return LILI_OK;
}
// the tables of a solve / an evaluation in the page-locked block: the fixed part, the state, then the arrays that follow the graph (PgTables' pointers are their
// addresses in tabv); *n_sep, *n_blk = the number of separators and of reduced blocks
struct PgLayout { size_t loop, seg, blk, sep, node_ptr, node_ent, blk_ent, bytes; };
int fill_tables(lili_ctx* ctx, PoseGraphState* P, const lili_pg_options& opt, PgLayout* lay, int* n_sep, int* n_blk) {
    const int n = P->n, L = P->n_loops;
    std::vector<int> sep;
    sep.reserve((size_t)n / kPgSegment + 1 + 2 * (size_t)L);
    for (int s = 0; s < n; s += kPgSegment) sep.push_back(s);
    for (const PgLoop& l : P->loops) { sep.push_back(l.from); sep.push_back(l.to); }
    std::sort(sep.begin(), sep.end());
    sep.erase(std::unique(sep.begin(), sep.end()), sep.end());
    const int K = (int)sep.size();
    // the loops of every pair of separators (p > q), in loop order
    struct Ent { int p, q, en; };
    std::vector<Ent> ents((size_t)L);
    std::vector<int> sf((size_t)L), stt((size_t)L);
    for (int l = 0; l < L; l++) {
        sf[l] = (int)(std::lower_bound(sep.begin(), sep.end(), P->loops[l].from) - sep.begin());
        stt[l] = (int)(std::lower_bound(sep.begin(), sep.end(), P->loops[l].to) - sep.begin());
        ents[l] = sf[l] > stt[l] ? Ent{sf[l], stt[l], 2 * l} : Ent{stt[l], sf[l], 2 * l + 1};
    }
    std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.p != b.p ? a.p < b.p : a.q != b.q ? a.q < b.q : a.en < b.en; });
    std::vector<PgBlock> blk;
    blk.reserve((size_t)2 * K + L);
    for (int p = 0; p < K; p++) blk.push_back(PgBlock{p, p, 0, 0});
    for (int q = 0; q + 1 < K; q++) blk.push_back(PgBlock{q + 1, q, 0, 0});
    for (int u = 0; u < L;) {
        int e = u;
        while (e < L && ents[e].p == ents[u].p && ents[e].q == ents[u].q) e++;
        if (ents[u].p == ents[u].q + 1) { blk[(size_t)K + ents[u].q].begin = u; blk[(size_t)K + ents[u].q].end = e; }
        else blk.push_back(PgBlock{ents[u].p, ents[u].q, u, e});
        u = e;
    }
    const int NB = (int)blk.size();
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    PgLayout& o = *lay;
    o.loop = 0;
    o.seg = o.loop + up8(sizeof(PgLoop) * (size_t)L);
    o.blk = o.seg + up8(sizeof(PgSeg) * (size_t)K);
    o.sep = o.blk + up8(sizeof(PgBlock) * (size_t)NB);
    o.node_ptr = o.sep + up8(sizeof(int) * (size_t)K);
    o.node_ent = o.node_ptr + up8(sizeof(int) * ((size_t)n + 1));
    o.blk_ent = o.node_ent + up8(sizeof(int) * 2 * (size_t)L);
    o.bytes = o.blk_ent + up8(sizeof(int) * (size_t)L) + 8;
    HIPCHK(P->h_tab.ensure(sizeof(PgTables) + sizeof(PgState) + o.bytes));
    HIPCHK(P->tabv.ensure(o.bytes));
    PgTables* T = P->h_tab.as<PgTables>();
    std::memset(T, 0, sizeof *T);
    T->n = n; T->n_loops = L; T->n_sep = K; T->n_blk = NB; T->max_iter = opt.max_iterations;
    T->function_tolerance = opt.function_tolerance; T->gradient_tolerance = opt.gradient_tolerance; T->parameter_tolerance = opt.parameter_tolerance;
    for (int k = 0; k < 6; k++) { T->w_prior[k] = 1.0 / std::sqrt(opt.prior_var[k]); T->w_odom[k] = 1.0 / std::sqrt(opt.odom_var[k]); }
    PgState* S = P->host_state();
    std::memset(S, 0, sizeof *S);
    S->s.n_nodes = n; S->s.n_loops = L;
    char* hv = reinterpret_cast<char*>(S + 1);
    const char* dv = P->tabv.as<char>();
    std::memset(hv, 0, o.bytes);
    PgLoop* h_loop = reinterpret_cast<PgLoop*>(hv + o.loop);
    PgSeg* h_seg = reinterpret_cast<PgSeg*>(hv + o.seg);
    int* h_sep = reinterpret_cast<int*>(hv + o.sep);
    int* h_np = reinterpret_cast<int*>(hv + o.node_ptr);
    int* h_ne = reinterpret_cast<int*>(hv + o.node_ent);
    int* h_be = reinterpret_cast<int*>(hv + o.blk_ent);
    for (int k = 0; k < K; k++) {
        const bool more = k + 1 < K;
        h_sep[k] = sep[k];
        h_seg[k] = PgSeg{sep[k], sep[k] + 1, more ? sep[k + 1] - 1 : n - 1, more ? sep[k + 1] : -1};
    }
    for (int l = 0; l < L; l++) { h_loop[l] = P->loops[l]; h_loop[l].sep_from = sf[l]; h_loop[l].sep_to = stt[l]; }
    if (NB) std::memcpy(hv + o.blk, blk.data(), sizeof(PgBlock) * (size_t)NB);
    for (int l = 0; l < L; l++) h_be[l] = ents[l].en;
    // the loops of every node, in loop order: counts, offsets, entries
    for (int l = 0; l < L; l++) { h_np[P->loops[l].from + 1]++; h_np[P->loops[l].to + 1]++; }
    for (int i = 0; i < n; i++) h_np[i + 1] += h_np[i];
    {
        std::vector<int> fill(sep.size(), 0);      // only separators have loops
        for (int l = 0; l < L; l++) {
            h_ne[h_np[P->loops[l].from] + fill[sf[l]]++] = 2 * l;
            h_ne[h_np[P->loops[l].to] + fill[stt[l]]++] = 2 * l + 1;
        }
    }
    T->loop = reinterpret_cast<const PgLoop*>(dv + o.loop); T->seg = reinterpret_cast<const PgSeg*>(dv + o.seg); T->blk = reinterpret_cast<const PgBlock*>(dv + o.blk);
    T->sep = reinterpret_cast<const int*>(dv + o.sep); T->node_ptr = reinterpret_cast<const int*>(dv + o.node_ptr);
    T->node_ent = reinterpret_cast<const int*>(dv + o.node_ent); T->blk_ent = reinterpret_cast<const int*>(dv + o.blk_ent);
    *n_sep = K; *n_blk = NB;
    return LILI_OK;
}
int upload_tables(lili_ctx* ctx, PoseGraphState* P, const PgLayout& lay) {
    const PgTables* T = P->h_tab.as<PgTables>();
    const PgState* S = P->host_state();
    HIPCHK(hipMemcpyAsync(P->tab.p, T, sizeof(PgTables), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(P->st.p, S, sizeof(PgState), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(P->tabv.p, S + 1, lay.bytes, hipMemcpyHostToDevice, ctx->stream));
    return LILI_OK;
}
// the reduced system's solve of one iteration: one workgroup up to kPgMaxReduced unknowns, the blocked Cholesky and its substitutions beyond
void launch_reduced_solve(lili_ctx* ctx, const PgDev& G, const int n_sep) {
    const int nr = 6 * n_sep;
    if (nr <= kPgMaxReduced) { hipLaunchKernelGGL(k_pg_reduced_solve, dim3(1), dim3(kPgWide), 0, ctx->stream, G); return; }
    const int nt = (nr + kPgTile - 1) / kPgTile;
    for (int k = 0; k < nt; k++) {
        hipLaunchKernelGGL(k_pg_chol_diag, dim3(1), dim3(256), 0, ctx->stream, G, k);
        const int w = nt - k - 1;
        if (w == 0) break;
        hipLaunchKernelGGL(k_pg_chol_panel, dim3(w), dim3(128), 0, ctx->stream, G, k);
        hipLaunchKernelGGL(k_pg_chol_update, dim3(w * (w + 1) / 2), dim3(256), 0, ctx->stream, G, k);
    }
    for (int i = nt - 1; i >= 0; i--) hipLaunchKernelGGL(k_pg_chol_back, dim3(i + 1), dim3(128), 0, ctx->stream, G, i);
}
void launch_linearize(lili_ctx* ctx, const PoseGraphState* P, const PgDev& G) {
    const int F = P->n + P->n_loops;
    hipLaunchKernelGGL(k_pg_linearize, dim3(nblocks(2 * (int64_t)F, 256)), dim3(256), 0, ctx->stream, G);
    hipLaunchKernelGGL(k_pg_assemble, dim3(nblocks((int64_t)P->n * 78 + 36 * P->n_loops, 256)), dim3(256), 0, ctx->stream, G);
}

// ---- what the calls that run kernels on the graph share.  PgNeeds: the work arrays of nothing (loop_status), of an evaluation, of the elimination too
enum PgNeeds { kPgTablesOnly, kPgEvaluation, kPgElimination };
struct PgCall { PoseGraphState* P; lili_pg_options opt{}; PgLayout lay{}; int K = 0, NB = 0; PgDev G{}; };
using PgStep = std::function<int()>;
// The prologue, in the order of its refusals: the options, own_checks (the caller's argument checks behind the options' and in front of the empty graph's refusal),
// the empty graph.  before_upload edits the host tables and state, or allocates what the device view needs.  Without the elimination the view is that of K = 0 (no rhs)
int prepare_call(lili_ctx* ctx, const char* who, const lili_pg_options* options, const PgNeeds needs, PgCall* c, const PgStep& own_checks = nullptr,
                 const PgStep& before_upload = nullptr) {
    PoseGraphState* P = c->P;
    TRY(check_options(ctx, options, &c->opt));
    if (own_checks) TRY(own_checks());
    if (P->n == 0) return ctx->fail(LILI_E_STATE, std::string(who) + ": the graph is empty");
    HIPCHK(hipSetDevice(ctx->device));
    TRY(P->persist(ctx));
    TRY(fill_tables(ctx, P, c->opt, &c->lay, &c->K, &c->NB));
    if (before_upload) TRY(before_upload());
    const int K = needs == kPgElimination ? c->K : 0;
    if (needs != kPgTablesOnly) TRY(P->work(ctx, K, needs == kPgElimination));
    TRY(upload_tables(ctx, P, c->lay));
    c->G = P->dev(K);
    return LILI_OK;
}
int zero_blocks(const int K) { return (int)std::min<size_t>(2048, ((size_t)18 * K * K + 255) / 256); }
// The front of an iteration, up to the separators' step.  damped: k_pg_eliminate's kDamped instance; gate_mode 1 (marginals): a converged graph is factored like any other
void enqueue_factorisation(lili_ctx* ctx, const PgCall& c, const bool damped, const int gate_mode) {
    const PgDev& G = c.G;
    launch_linearize(ctx, c.P, G);
    hipLaunchKernelGGL(k_pg_gate, dim3(1), dim3(kPgWide), 0, ctx->stream, G, gate_mode);
    if (damped) hipLaunchKernelGGL((k_pg_eliminate<true>), dim3(c.K), dim3(64), 0, ctx->stream, G);
    else hipLaunchKernelGGL((k_pg_eliminate<false>), dim3(c.K), dim3(64), 0, ctx->stream, G);
    hipLaunchKernelGGL(k_pg_zero, dim3(zero_blocks(c.K)), dim3(256), 0, ctx->stream, G);
    hipLaunchKernelGGL(k_pg_reduced_assemble, dim3(c.NB), dim3(64), 0, ctx->stream, G);
    launch_reduced_solve(ctx, G, c.K);
}
// the events around a call's kernels; close: the launches' status, the closing event, the state's read-back enqueued
int open_bracket(lili_ctx* ctx, PoseGraphState* P) {
    HIPCHK(P->ev0.get(hipEventDefault)); HIPCHK(P->ev1.get(hipEventDefault));
    HIPCHK(hipEventRecord(P->ev0, ctx->stream));
    return LILI_OK;
}
int close_bracket(lili_ctx* ctx, PoseGraphState* P) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(P->ev1, ctx->stream));
    HIPCHK(hipMemcpyAsync(P->host_state(), P->st.p, sizeof(PgState), hipMemcpyDeviceToHost, ctx->stream));
    return LILI_OK;
}
// every iteration enqueued up front (damped: a rejected attempt linearises again at the unchanged X: the same bytes); the state lands in P->host_state()
int run_solve(lili_ctx* ctx, const PgCall& c, const bool damped) {
    PoseGraphState* P = c.P;
    TRY(open_bracket(ctx, P));
    for (int it = 0; it < c.opt.max_iterations; it++) {
        enqueue_factorisation(ctx, c, damped, 0);
        hipLaunchKernelGGL(k_pg_backsub, dim3(c.K), dim3(64), 0, ctx->stream, c.G);
        if (damped) hipLaunchKernelGGL(k_pg_lm_decide, dim3(1), dim3(kPgWide), 0, ctx->stream, c.G);
        else hipLaunchKernelGGL(k_pg_retract_cost, dim3(1), dim3(kPgWide), 0, ctx->stream, c.G);
    }
    TRY(close_bracket(ctx, P));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipEventElapsedTime(&P->last_ms, P->ev0, P->ev1));
    return LILI_OK;
}

// ---- host-side quaternion algebra as Eigen 3.3 evaluates it (q = w, x, y, z)
struct hq { double w, x, y, z; };
struct hv { double x, y, z; };
hq h_mul(const hq a, const hq b) {
    return hq{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
              a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
hq h_inv(const hq q) {
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    return hq{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
}
hv h_cross(const hv a, const hv b) { return hv{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
hv h_rot(const hq q, const hv v) {
    const hv u{q.x, q.y, q.z};
    hv uv = h_cross(u, v);
    uv = hv{uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
    const hv c = h_cross(u, uv);
    return hv{(v.x + q.w * uv.x) + c.x, (v.y + q.w * uv.y) + c.y, (v.z + q.w * uv.z) + c.z};
}
hq h_normalized(const hq q) {
    const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return hq{q.w / n, q.x / n, q.y / n, q.z / n};
}
// Eigen::Quaterniond(const Matrix3d&), m row-major
hq h_from_matrix(const double* m) {
    double t = m[0] + m[4] + m[8];
    double q[4];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t; q[2] = (m[2] - m[6]) * t; q[3] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
    return hq{q[0], q[1], q[2], q[3]};
}

}  // namespace

extern "C" {

void lili_pg_default_options(lili_pg_options* o) {
    if (!o) return;
    o->max_iterations = 10; o->reserved_ = 0;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    for (int k = 0; k < 3; k++) { o->prior_var[k] = 1e-6; o->prior_var[3 + k] = 1e-8; o->odom_var[k] = 1e-6; o->odom_var[3 + k] = 1e-4; }
}

int lili_pose_graph_reset(lili_ctx* ctx) {
    if (!ctx) return LILI_E_ARG;
    PoseGraphState* P = pg_of(ctx);
    P->n = 0; P->n_loops = 0;
    P->loops.clear();
    ctx->pose_graph_loops = 0;
    return LILI_OK;
}

int lili_pose_graph_info(lili_ctx* ctx, int* n_nodes, int* n_loops) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(n_nodes && n_loops, "pose_graph_info: null argument");
    const PoseGraphState* P = pg_of(ctx);
    *n_nodes = P->n; *n_loops = P->n_loops;
    return LILI_OK;
}

int lili_pose_graph_append(lili_ctx* ctx, const double* prev, const double* poses, int n, int* first_id) {
    if (!ctx) return LILI_E_ARG;
    PoseGraphState* P = pg_of(ctx);
    ARGCHK(poses, "pose_graph_append: null poses");
    ARGCHK(n >= 1 && n <= kPgMaxNodes - P->n, "pose_graph_append: n < 1, or more than LILI_PG_MAX_NODES nodes");
    ARGCHK((prev != nullptr) == (P->n > 0), "pose_graph_append: prev must be NULL on an empty graph and the last node's pose on any other");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 7 * ((size_t)n + 1);
    HIPCHK(P->h_io.ensure(bytes));
    double* rows = P->h_io.as<double>();
    if (prev) TRY(check_poses(ctx, "pose_graph_append", prev, 1, rows));
    else std::memset(rows, 0, sizeof(double) * 7);
    TRY(check_poses(ctx, "pose_graph_append", poses, (size_t)n, rows + 7));
    TRY(P->persist(ctx));
    HIPCHK(P->stage.ensure(bytes));
    HIPCHK(hipMemcpyAsync(P->stage.p, rows, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pg_append, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, P->stage.as<double>(), P->n, n, P->X.as<double>(), P->meas.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (first_id) *first_id = P->n;
    P->n += n;
    return LILI_OK;
}

int lili_pose_graph_add_loop(lili_ctx* ctx, int from, int to, const double meas[7], const double var[6]) {
    return lili_pose_graph_add_loop_robust(ctx, from, to, meas, var, LILI_PG_LOSS_NONE, 0.0);
}

int lili_pose_graph_add_loop_robust(lili_ctx* ctx, int from, int to, const double meas[7], const double var[6], int loss, double scale) {
    if (!ctx) return LILI_E_ARG;
    PoseGraphState* P = pg_of(ctx);
    ARGCHK(meas && var, "pose_graph_add_loop: null argument");
    ARGCHK(from >= 0 && from < P->n && to >= 0 && to < P->n && from != to, "pose_graph_add_loop: from / to must be two different nodes of the graph");
    ARGCHK(P->n_loops < ctx->pose_graph_max_loops, "pose_graph_add_loop: more than LILI_PG_MAX_LOOPS loops");      // (option "pose_graph_max_loops")
    ARGCHK(finite_n(var, 6), "pose_graph_add_loop: an input is not finite");
    for (int k = 0; k < 6; k++) ARGCHK(var[k] > 0, "pose_graph_add_loop: a variance is not positive");
    ARGCHK(loss == LILI_PG_LOSS_NONE || loss == LILI_PG_LOSS_HUBER || loss == LILI_PG_LOSS_CAUCHY || loss == LILI_PG_LOSS_GEMAN_MCCLURE, "pose_graph_add_loop_robust: unknown loss");
    ARGCHK(loss == LILI_PG_LOSS_NONE || (std::isfinite(scale) && scale > 0), "pose_graph_add_loop_robust: the scale of a loss must be positive and finite");
    PgLoop l{};
    TRY(check_poses(ctx, "pose_graph_add_loop", meas, 1, l.meas));
    l.from = from; l.to = to;
    for (int k = 0; k < 6; k++) l.w[k] = 1.0 / std::sqrt(var[k]);
    l.loss = loss; l.scale = loss == LILI_PG_LOSS_NONE ? 0.0 : scale;
    P->loops.push_back(l);
    ctx->pose_graph_loops = P->n_loops = (int)P->loops.size();
    return LILI_OK;
}

int lili_pose_graph_get(lili_ctx* ctx, int first, int n, double* poses) {
    if (!ctx) return LILI_E_ARG;
    PoseGraphState* P = pg_of(ctx);
    ARGCHK(poses, "pose_graph_get: null poses");
    ARGCHK(first >= 0 && n >= 1 && first <= P->n && n <= P->n - first, "pose_graph_get: range outside the graph");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 7 * (size_t)n;
    HIPCHK(P->h_io.ensure(bytes));
    HIPCHK(hipMemcpyAsync(P->h_io.p, P->X.as<double>() + 7 * (size_t)first, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memcpy(poses, P->h_io.p, bytes);
    return LILI_OK;
}

int lili_pose_graph_set(lili_ctx* ctx, int first, int n, const double* poses) {
    if (!ctx) return LILI_E_ARG;
    PoseGraphState* P = pg_of(ctx);
    ARGCHK(poses, "pose_graph_set: null poses");
    ARGCHK(first >= 0 && n >= 1 && first <= P->n && n <= P->n - first, "pose_graph_set: range outside the graph");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 7 * (size_t)n;
    HIPCHK(P->h_io.ensure(bytes));
    TRY(check_poses(ctx, "pose_graph_set", poses, (size_t)n, P->h_io.as<double>()));
    HIPCHK(hipMemcpyAsync(P->X.as<double>() + 7 * (size_t)first, P->h_io.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LILI_OK;
}

int lili_pose_graph_evaluate(lili_ctx* ctx, const lili_pg_options* options, double* cost, double* gradient, double* diag, double* sub, double* loop_blocks) {
    if (!ctx) return LILI_E_ARG;
    PgCall c{pg_of(ctx)};
    PoseGraphState* P = c.P;
    ARGCHK(cost && gradient && diag && (sub || P->n <= 1) && (loop_blocks || P->n_loops == 0), "pose_graph_evaluate: null argument");
    TRY(prepare_call(ctx, "pose_graph_evaluate", options, kPgEvaluation, &c));
    const size_t N = (size_t)P->n, L = (size_t)P->n_loops, d = sizeof(double);
    const size_t o_g = 0, o_D = o_g + 6 * N, o_S = o_D + 36 * N, o_L = o_S + 36 * N, total = o_L + 36 * L;
    HIPCHK(P->h_io.ensure(total * d));
    launch_linearize(ctx, P, c.G);
    hipLaunchKernelGGL(k_pg_gate, dim3(1), dim3(kPgWide), 0, ctx->stream, c.G, 1);
    HIPCHK(hipGetLastError());
    double* h = P->h_io.as<double>();
    PgState* hs = P->host_state();
    HIPCHK(hipMemcpyAsync(hs, P->st.p, sizeof(PgState), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h + o_g, P->g.p, 6 * N * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h + o_D, P->D.p, 36 * N * d, hipMemcpyDeviceToHost, ctx->stream));
    if (N > 1) HIPCHK(hipMemcpyAsync(h + o_S, P->S.p, 36 * (N - 1) * d, hipMemcpyDeviceToHost, ctx->stream));
    if (L) HIPCHK(hipMemcpyAsync(h + o_L, P->LB.p, 36 * L * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *cost = hs->cost;
    std::memcpy(gradient, h + o_g, 6 * N * d);
    std::memcpy(diag, h + o_D, 36 * N * d);
    if (N > 1) std::memcpy(sub, h + o_S, 36 * (N - 1) * d);
    if (L) std::memcpy(loop_blocks, h + o_L, 36 * L * d);
    return LILI_OK;
}

int lili_pose_graph_solve(lili_ctx* ctx, const lili_pg_options* options, lili_pg_summary* summary) {
    if (!ctx) return LILI_E_ARG;
    PgCall c{pg_of(ctx)};
    ARGCHK(summary, "pose_graph_solve: null summary");
    TRY(prepare_call(ctx, "pose_graph_solve", options, kPgElimination, &c));
    TRY(run_solve(ctx, c, false));
    *summary = c.P->host_state()->s;
    return LILI_OK;
}

void lili_pg_lm_default_options(lili_pg_lm_options* o) {
    if (!o) return;
    o->initial_lambda = 1e-5; o->lambda_factor = 10.0; o->lambda_lower = 1e-10; o->lambda_upper = 1e8;
    o->diagonal_damping = 0; o->reserved_ = 0;
}

int lili_pose_graph_solve_lm(lili_ctx* ctx, const lili_pg_options* options, const lili_pg_lm_options* lm_options, lili_pg_lm_summary* summary) {
    if (!ctx) return LILI_E_ARG;
    PgCall c{pg_of(ctx)};
    PoseGraphState* P = c.P;
    ARGCHK(summary, "pose_graph_solve_lm: null summary");
    lili_pg_lm_options lm;
    if (lm_options) lm = *lm_options; else lili_pg_lm_default_options(&lm);
    const auto check_lm = [&]() -> int {
        ARGCHK(std::isfinite(lm.initial_lambda) && std::isfinite(lm.lambda_factor) && std::isfinite(lm.lambda_lower) && std::isfinite(lm.lambda_upper),
               "pose_graph_solve_lm: an option is not finite");
        ARGCHK(lm.initial_lambda > 0 && lm.lambda_factor > 1 && lm.lambda_lower > 0 && lm.lambda_upper >= lm.lambda_lower,
               "pose_graph_solve_lm: initial_lambda and lambda_lower must be positive, lambda_factor above 1, lambda_upper not below lambda_lower");
        ARGCHK(lm.diagonal_damping == 0 || lm.diagonal_damping == 1, "pose_graph_solve_lm: diagonal_damping must be 0 or 1");
        return LILI_OK;
    };
    const auto set_damping = [&]() -> int {
        PgState* hs = P->host_state();
        P->h_tab.as<PgTables>()->damping = lm.diagonal_damping ? 2 : 1;
        hs->lambda = lm.initial_lambda; hs->lambda_factor = lm.lambda_factor; hs->lambda_lower = lm.lambda_lower; hs->lambda_upper = lm.lambda_upper;
        return LILI_OK;
    };
    TRY(prepare_call(ctx, "pose_graph_solve_lm", options, kPgElimination, &c, check_lm, set_damping));
    TRY(run_solve(ctx, c, true));
    const PgState* hs = P->host_state();
    std::memset(summary, 0, sizeof *summary);
    summary->base = hs->s;
    std::memcpy(summary->lambda, hs->lambda_log, sizeof summary->lambda);
    for (int k = 0; k < LILI_PG_MAX_LOG; k++) summary->accepted[k] = hs->accepted[k];
    summary->steps_accepted = hs->steps_accepted; summary->steps_rejected = hs->steps_rejected;
    summary->final_lambda = hs->lambda;
    return LILI_OK;
}

int lili_pose_graph_loop_status(lili_ctx* ctx, const lili_pg_options* options, int first, int n, double* chi2, double* weight) {
    if (!ctx) return LILI_E_ARG;
    PgCall c{pg_of(ctx)};
    PoseGraphState* P = c.P;
    ARGCHK(chi2 && weight, "pose_graph_loop_status: null argument");
    ARGCHK(first >= 0 && n >= 1 && first <= P->n_loops && n <= P->n_loops - first, "pose_graph_loop_status: range outside the graph's loops");      // (a loop: not empty)
    TRY(prepare_call(ctx, "pose_graph_loop_status", options, kPgTablesOnly, &c));
    const size_t bytes = sizeof(double) * 2 * (size_t)n;
    HIPCHK(P->h_io.ensure(bytes));
    HIPCHK(P->stage.ensure(bytes));
    hipLaunchKernelGGL(k_pg_loop_status, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, c.G, first, n, P->stage.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(P->h_io.p, P->stage.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memcpy(chi2, P->h_io.p, sizeof(double) * (size_t)n);
    std::memcpy(weight, P->h_io.as<double>() + n, sizeof(double) * (size_t)n);
    return LILI_OK;
}

int lili_pose_graph_kernel_ms(lili_ctx* ctx, float* ms) {
    if (!ctx) return LILI_E_ARG;
    ARGCHK(ms, "pose_graph_kernel_ms: null argument");
    const PoseGraphState* P = static_cast<const PoseGraphState*>(ctx->ext[lili_ctx::kExtPoseGraph].get());
    if (!P || P->last_ms < 0.f) return ctx->fail(LILI_E_STATE, "pose_graph_kernel_ms: no lili_pose_graph_solve or lili_pose_graph_solve_lm yet");
    *ms = P->last_ms;
    return LILI_OK;
}

int lili_pose_graph_marginals(lili_ctx* ctx, const lili_pg_options* options, int first, int n, double* cov, const int32_t* pairs, int n_pairs, double* cross,
                              lili_pg_marginals_info* info) {
    if (!ctx) return LILI_E_ARG;
    PgCall c{pg_of(ctx)};
    PoseGraphState* P = c.P;
    ARGCHK(n >= 0 && n_pairs >= 0 && n_pairs <= LILI_PG_MAX_PAIRS && (n > 0 || n_pairs > 0), "pose_graph_marginals: n or n_pairs is negative, both are zero, or more than LILI_PG_MAX_PAIRS pairs");
    ARGCHK((cov || n == 0) && ((pairs && cross) || n_pairs == 0), "pose_graph_marginals: null argument");
    const size_t d = sizeof(double), n_cov = 36 * (size_t)n, n_cross = 36 * (size_t)n_pairs;
    const auto check_range = [&]() -> int {      // on an empty graph no range is judged: the prologue's refusal of the empty graph comes first
        if (P->n == 0) return LILI_OK;
        ARGCHK(n == 0 || (first >= 0 && first < P->n && n <= P->n - first), "pose_graph_marginals: range outside the graph");
        for (int k = 0; k < 2 * n_pairs; k++) ARGCHK(pairs[k] >= 0 && pairs[k] < P->n, "pose_graph_marginals: a pair names a node outside the graph");
        return LILI_OK;
    };
    const auto own_arrays = [&]() -> int { return P->work_marginals(ctx, c.K, n_pairs); };      // (in front of the device view)
    TRY(prepare_call(ctx, "pose_graph_marginals", options, kPgElimination, &c, check_range, own_arrays));
    HIPCHK(P->h_io.ensure((n_cov + n_cross) * d));
    const int K = c.K;
    if (n_pairs) {
        HIPCHK(P->h_pairs.ensure(sizeof(int32_t) * 2 * (size_t)n_pairs));
        std::memcpy(P->h_pairs.p, pairs, sizeof(int32_t) * 2 * (size_t)n_pairs);
        HIPCHK(hipMemcpyAsync(P->pairs.p, P->h_pairs.p, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
    }
    TRY(open_bracket(ctx, P));
    enqueue_factorisation(ctx, c, false, 1);
    // the inverse side
    hipLaunchKernelGGL(k_pg_marg_inverse, dim3(K), dim3(kPgInvThreads), 0, ctx->stream, c.G);
    hipLaunchKernelGGL(k_pg_marg_segments, dim3(K), dim3(64), 0, ctx->stream, c.G);
    if (n_pairs) hipLaunchKernelGGL(k_pg_marg_pairs, dim3(n_pairs), dim3(64), 0, ctx->stream, c.G);
    TRY(close_bracket(ctx, P));
    double* h = P->h_io.as<double>();
    const PgState* hs = P->host_state();
    if (n) HIPCHK(hipMemcpyAsync(h, P->cov.as<double>() + 36 * (size_t)first, n_cov * d, hipMemcpyDeviceToHost, ctx->stream));
    if (n_pairs) HIPCHK(hipMemcpyAsync(h + n_cov, P->cross.p, n_cross * d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, P->ev0, P->ev1));
    const bool failed = hs->done != 0;      // only a non-positive pivot sets the termination word here
    if (info) {
        info->status = failed ? LILI_LM_NUMERICAL_FAILURE : 0;
        info->n_nodes = P->n; info->n_loops = P->n_loops; info->reduced_unknowns = 6 * K;
        info->kernel_ms = ms; info->reserved_ = 0;
    }
    if (failed) return ctx->fail(LILI_E_NUMERIC, "pose_graph_marginals: a non-positive pivot: the information matrix is not positive definite in double precision");
    if (n) std::memcpy(cov, h, n_cov * d);
    if (n_pairs) std::memcpy(cross, h + n_cov, n_cross * d);
    return LILI_OK;
}

int lili_pose_relative_covariance(const double pose_i[7], const double pose_j[7], const double cov_ii[36], const double cov_jj[36], const double cov_ij[36],
                                  double cov_rel[36]) {
    if (!pose_i || !pose_j || !cov_ii || !cov_jj || !cov_ij || !cov_rel) return LILI_E_ARG;
    if (!finite_n(pose_i, 7) || !finite_n(pose_j, 7) || !finite_n(cov_ii, 36) || !finite_n(cov_jj, 36) || !finite_n(cov_ij, 36)) return LILI_E_ARG;
    double ni, nj;
    if (!unit_quaternion(pose_i, &ni) || !unit_quaternion(pose_j, &nj)) return LILI_E_ARG;
    // Z = between(X_i, X_j): R_Z = R_i^T R_j, t_Z = d = R_i^T (p_j - p_i)
    const hq qi{pose_i[3] / ni, pose_i[4] / ni, pose_i[5] / ni, pose_i[6] / ni}, qj{pose_j[3] / nj, pose_j[4] / nj, pose_j[5] / nj, pose_j[6] / nj};
    const hq ci{qi.w, -qi.x, -qi.y, -qi.z};
    const hv t = h_rot(ci, hv{pose_j[0] - pose_i[0], pose_j[1] - pose_i[1], pose_j[2] - pose_i[2]});
    const hq z = h_normalized(h_mul(ci, qj));
    const double R[9] = {1 - 2 * (z.y * z.y + z.z * z.z), 2 * (z.x * z.y - z.w * z.z), 2 * (z.x * z.z + z.w * z.y),
                         2 * (z.x * z.y + z.w * z.z), 1 - 2 * (z.x * z.x + z.z * z.z), 2 * (z.y * z.z - z.w * z.x),
                         2 * (z.x * z.z - z.w * z.y), 2 * (z.y * z.z + z.w * z.x), 1 - 2 * (z.x * z.x + z.y * z.y)};
    double Sd[9];
    lili::pg_skew(t.x, t.y, t.z, Sd);
    // J_a = [-R_Z^T, 0; R_Z^T [t_Z]x, -R_Z^T], J_b = I
    double Ja[36] = {0.0};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            Ja[6 * r + c] = -R[3 * c + r];
            Ja[6 * (3 + r) + 3 + c] = -R[3 * c + r];
            Ja[6 * (3 + r) + c] = (R[r] * Sd[c] + R[3 + r] * Sd[3 + c]) + R[6 + r] * Sd[6 + c];
        }
    double A[36], B[36], out[36];      // A = J_a Sigma_ii, B = J_a Sigma_ij
    for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < 6; k++) { a += Ja[6 * r + k] * cov_ii[6 * k + c]; b += Ja[6 * r + k] * cov_ij[6 * k + c]; }
            A[6 * r + c] = a; B[6 * r + c] = b;
        }
    for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++) {
            double a = 0.0;
            for (int k = 0; k < 6; k++) a += A[6 * r + k] * Ja[6 * c + k];
            out[6 * r + c] = ((a + B[6 * r + c]) + B[6 * c + r]) + cov_jj[6 * r + c];
        }
    std::memcpy(cov_rel, out, sizeof out);
    return LILI_OK;
}

int lili_loop_measurement(const double T_icp[16],const double pose_latest[7], const double pose_closest[7], double meas[7]) {
    if (!T_icp || !pose_latest || !pose_closest || !meas) return LILI_E_ARG;
    if (!finite_n(T_icp, 16) || !finite_n(pose_latest, 7) || !finite_n(pose_closest, 7)) return LILI_E_ARG;
    // L:2587-2600: quaternionIncre(R), transitionIncre; corrected = incre * toCorrect
    const double R[9] = {T_icp[0], T_icp[1], T_icp[2], T_icp[4], T_icp[5], T_icp[6], T_icp[8], T_icp[9], T_icp[10]};
    const hq q_inc = h_from_matrix(R);
    const hq q_lat{pose_latest[3], pose_latest[4], pose_latest[5], pose_latest[6]}, q_clo{pose_closest[3], pose_closest[4], pose_closest[5], pose_closest[6]};
    const hq q_cor = h_mul(q_inc, q_lat);
    const hv r = h_rot(q_inc, hv{pose_latest[0], pose_latest[1], pose_latest[2]});
    const hv t_cor{r.x + T_icp[3], r.y + T_icp[7], r.z + T_icp[11]};
    const double n_from = q_cor.x * q_cor.x + q_cor.y * q_cor.y + q_cor.z * q_cor.z + q_cor.w * q_cor.w;
    const double n_to = q_clo.x * q_clo.x + q_clo.y * q_clo.y + q_clo.z * q_clo.z + q_clo.w * q_clo.w;
    if (!(n_from > 0.0) || !(n_to > 0.0) || !std::isfinite(n_from) || !std::isfinite(n_to)) return LILI_E_ARG;
    // L:2602-2622: Rot3::Quaternion of both (unit quaternions), poseFrom.between(poseTo)
    const hq qf = h_normalized(q_cor), qt = h_normalized(q_clo);
    const hq fi{qf.w, -qf.x, -qf.y, -qf.z};
    const hv t = h_rot(fi, hv{pose_closest[0] - t_cor.x, pose_closest[1] - t_cor.y, pose_closest[2] - t_cor.z});
    const hq q = h_normalized(h_mul(fi, qt));
    if (!std::isfinite(t.x) || !std::isfinite(t.y) || !std::isfinite(t.z) || !std::isfinite(q.w)) return LILI_E_ARG;
    meas[0] = t.x; meas[1] = t.y; meas[2] = t.z; meas[3] = q.w; meas[4] = q.x; meas[5] = q.y; meas[6] = q.z;
    return LILI_OK;
}

int lili_correct_poses(const double* solution, int n_frames, const int32_t* keyframe_id_in_frame, int n_keyframes, int slide_window_width, int f32_positions,
                       double* abs_poses, int n_abs, double* frame_poses, double* keyframe_poses, double last_pose[7], double select_pose[3]) {
    if (!solution || !keyframe_id_in_frame || !abs_poses || !frame_poses || !keyframe_poses || !last_pose || !select_pose) return LILI_E_ARG;
    const int w = slide_window_width;
    if (n_frames < 1 || n_keyframes < 1 || n_abs < 1 || w < 2 || w > n_abs || w > n_keyframes || n_abs > n_keyframes + 1 || n_keyframes - w + 2 > n_abs) return LILI_E_ARG;
    for (int i = 0; i <= n_keyframes - w; i++) if (keyframe_id_in_frame[i] < 0 || keyframe_id_in_frame[i] >= n_frames) return LILI_E_ARG;
    if (!finite_n(solution, 7 * (size_t)n_frames) || !finite_n(abs_poses, 7 * (size_t)n_abs)) return LILI_E_ARG;
    auto A = [&](int i) { return abs_poses + 7 * (size_t)i; };
    auto pos = [&](double v) { return f32_positions ? (double)(float)v : v; };
    // L:2186-2209: the relative transforms of the window's tail
    hq qrel[64]; hv trel[64];
    if (w - 1 > 64) return LILI_E_ARG;
    for (int i = n_abs - w; i < n_abs - 1; i++) {
        const hq qf{A(i)[0], A(i)[1], A(i)[2], A(i)[3]}, qt{A(i + 1)[0], A(i + 1)[1], A(i + 1)[2], A(i + 1)[3]};
        const hv tf{A(i)[4], A(i)[5], A(i)[6]}, tt{A(i + 1)[4], A(i + 1)[5], A(i + 1)[6]};
        qrel[i - (n_abs - w)] = h_mul(h_inv(qf), qt);
        trel[i - (n_abs - w)] = h_rot(h_inv(qf), hv{tt.x - tf.x, tt.y - tf.y, tt.z - tf.z});
    }
    // L:2211-2225: every frame from the solution
    for (int i = 0; i < n_frames; i++) {
        const double* s = solution + 7 * (size_t)i;
        double* f = frame_poses + 7 * (size_t)i;
        f[0] = pos(s[0]); f[1] = pos(s[1]); f[2] = pos(s[2]);
        f[3] = s[3]; f[4] = s[4]; f[5] = s[5]; f[6] = s[6];
    }
    // L:2227-2258: the keyframes outside the window's tail, and abs_poses[i + 1]
    for (int i = 0; i <= n_keyframes - w; i++) {
        const double* f = frame_poses + 7 * (size_t)keyframe_id_in_frame[i];
        double* k = keyframe_poses + 7 * (size_t)i;
        for (int c = 0; c < 7; c++) k[c] = f[c];
        A(i + 1)[0] = k[3]; A(i + 1)[1] = k[4]; A(i + 1)[2] = k[5]; A(i + 1)[3] = k[6];
        A(i + 1)[4] = k[0]; A(i + 1)[5] = k[1]; A(i + 1)[6] = k[2];
    }
    // L:2260-2298: the tail re-chained
    for (int i = n_abs - w; i < n_abs - 1; i++) {
        hq iq{A(i)[0], A(i)[1], A(i)[2], A(i)[3]};
        hv it{A(i)[4], A(i)[5], A(i)[6]};
        const hv r = h_rot(iq, trel[i - n_abs + w]);
        it = hv{it.x + r.x, it.y + r.y, it.z + r.z};
        iq = h_mul(iq, qrel[i - n_abs + w]);
        A(i + 1)[0] = iq.w; A(i + 1)[1] = iq.x; A(i + 1)[2] = iq.y; A(i + 1)[3] = iq.z;
        A(i + 1)[4] = it.x; A(i + 1)[5] = it.y; A(i + 1)[6] = it.z;
        double* k = keyframe_poses + 7 * (size_t)i;
        k[0] = pos(A(i + 1)[4]); k[1] = pos(A(i + 1)[5]); k[2] = pos(A(i + 1)[6]);
        k[3] = A(i + 1)[0]; k[4] = A(i + 1)[1]; k[5] = A(i + 1)[2]; k[6] = A(i + 1)[3];
    }
    // L:2300-2308
    for (int i = 0; i < 7; i++) last_pose[i] = A(n_abs - w)[i];
    select_pose[0] = pos(last_pose[4]); select_pose[1] = pos(last_pose[5]); select_pose[2] = pos(last_pose[6]);
    return LILI_OK;
}

}  // extern "C"
