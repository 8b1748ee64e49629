// The pieces that end an evaluation in every device solver — "turn a Gram partial into a step on a pose" — in ONE definition each:
//   gn_update_block (lili_s2m.hip: launch-by-launch Gauss-Newton), solve_lm_body (lili_s2m_lm.hip: per-slot Levenberg-Marquardt),
//   k_iterate_coop (lili_s2m_coop.hip: persistent Gauss-Newton), k_window_solve (lili_window.hip: the joint keyframe window); the trust-region bookkeeping is
//   also k_local_graph's (lili_local_graph.hip: the per-frame chain, dogleg).
// Every workgroup of a persistent launch runs these on the same bits and must arrive at the same bits, and the trust-region decisions follow
// Ceres' order of checks: a change here changes all four solvers at once, which is the point.  Everything is __device__ __forceinline__ or a type;
// the library is built with -ffp-contract=off, so the value of every result is fixed by the expression trees below.
#pragma once
#include "lili_s2m_dev.h"

namespace lili {

// upper-triangle partial (36 doubles, row by row) -> symmetric 8x8 Gram; lanes 0..63 of one wave
__device__ __forceinline__ void gram_tri_to_full(const double* tri, double* full) {
    const int lane = threadIdx.x & 63;
    const int r = lane >> 3, c = lane & 7;
    const int a = r < c ? r : c, b = r < c ? c : r;
    full[lane] = tri[a * 8 - a * (a - 1) / 2 + (b - a)];
}

// Entry (a, b) of the local 6x6 system H = P^T G77 P (a, b in 0..5) or of g = P^T G7r (b == 7) from the symmetric 8x8 Gram (rows J0..J6, r) at the
// quaternion q = (w, x, y, z); P = blockdiag(I3, Jq), Jq the plus-Jacobian (4x3) of ceres::QuaternionParameterization, rows
// [-x1 -x2 -x3; x0 x3 -x2; -x3 x0 x1; x2 -x1 x0].  Evaluated as M = G P (4-term sums, left to right) and P^T M.  One lane per entry: lanes 0..35 take
// (lane / 6, lane % 6), lanes 36..41 take (lane - 36, 7); where the entry goes (and the sign of g) is the caller's.
__device__ __forceinline__ double pose_local_entry(const double* gram, const double* q, const int a, const int b) {
    const double x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
    auto jcol = [&](int c, double o[4]) {
        o[0] = c == 0 ? -x1 : c == 1 ? -x2 : -x3;
        o[1] = c == 0 ? x0 : c == 1 ? x3 : -x2;
        o[2] = c == 0 ? -x3 : c == 1 ? x0 : x1;
        o[3] = c == 0 ? x2 : c == 1 ? -x1 : x0;
    };
    double jb[4] = {0, 0, 0, 0}, ja[4] = {0, 0, 0, 0};
    if (b >= 3 && b < 6) jcol(b - 3, jb);
    if (a >= 3) jcol(a - 3, ja);
    auto Mrow = [&](int i) -> double {      // (G P)[i][b];  for b == 7 the plain column G[i][7]
        if (b < 3 || b == 7) return gram[i * 8 + b];
        return ((gram[i * 8 + 3] * jb[0] + gram[i * 8 + 4] * jb[1]) + gram[i * 8 + 5] * jb[2]) + gram[i * 8 + 6] * jb[3];
    };
    if (a < 3) return Mrow(a);
    return ((ja[0] * Mrow(3) + ja[1] * Mrow(4)) + ja[2] * Mrow(5)) + ja[3] * Mrow(6);
}

// sin(|d|) / |d| and cos(|d|) from nd2 = |d|^2: the series of sinc_cos_small below 0.5 rad, above it halve the angle first and double it back
// (libm's sin / cos bring a Payne-Hanek reduction with a scratch table into a persistent launch; a trust-region step never turns that far anyway)
__device__ __forceinline__ void sinc_cos_halving(double nd2, double& sbd, double& cw) {
    if (nd2 < 0.25) sinc_cos_small(nd2, sbd, cw);
    else {
        double h2 = nd2; int k = 0;
        while (h2 >= 0.25 && k < 60) { h2 *= 0.25; k++; }
        double sc, c;
        sinc_cos_small(h2, sc, c);
        double sn = sc * sqrt(h2);
        for (int i = 0; i < k; i++) { const double s2 = 2.0 * sn * c, c2 = c * c - sn * sn; sn = s2; c = c2; }
        sbd = sn / sqrt(nd2); cw = c;
    }
}
// x (+) delta on the quaternion (ceres::QuaternionParameterization::Plus): out_q = (cos|d|, sin|d| / |d| d) * x_q, or x_q itself for d = 0; out_q may be x_q.
// sinc_cos(nd2, sbd, cw) supplies sin|d| / |d| and cos|d|.  Two variants exist because their bits differ above 0.5 rad: the persistent solvers pass
// sinc_cos_halving, gn_update_block keeps libm's sin / cos there, which is what its recorded results were computed with.
// sinc_cos must inline completely (a __device__ __forceinline__ function or a capture-less lambda): an indirect call would cost a stack frame, i.e. scratch.
template <class SincCos>
__device__ __forceinline__ void quat_plus(const double* x_q, const double* d_rot, double* out_q, SincCos sinc_cos) {
    const double nd2 = d_rot[0] * d_rot[0] + d_rot[1] * d_rot[1] + d_rot[2] * d_rot[2];
    if (nd2 > 0.0) {
        double sbd, cw;
        sinc_cos(nd2, sbd, cw);
        const dq r = qmul(dq{cw, sbd * d_rot[0], sbd * d_rot[1], sbd * d_rot[2]}, dq{x_q[0], x_q[1], x_q[2], x_q[3]});
        out_q[0] = r.w; out_q[1] = r.x; out_q[2] = r.y; out_q[3] = r.z;
    } else { out_q[0] = x_q[0]; out_q[1] = x_q[1]; out_q[2] = x_q[2]; out_q[3] = x_q[3]; }
}

// A d = b for a 6x6 A by ONE WAVE (all 64 lanes call it, control flow uniform): lane 7 i + j (< 42) passes entry j of row i of the augmented matrix
// [A | b] as `a` (lanes >= 42 idle along), every lane returns the whole d.  Elimination without pivoting — the pivot by v_readlane, the pivot row /
// column through ds_bpermute: six elimination and six substitution steps of ~200 cycles instead of ~600 dependent f64 instructions on one lane.
// Returns false if a pivot is not positive or the step is not finite.  Every workgroup runs the same instruction sequence on the same bits.
__device__ __forceinline__ bool solve6_wave(double a, double d[6]) {
    const int lane = threadIdx.x & 63;
    const int ri = lane / 7, cj = lane - 7 * ri;
    const bool in = lane < 42;
    bool okc = true;
    double pinv[6];
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const double piv = __shfl(a, p * 7 + p);
        okc = okc && (piv > 0.0);
        pinv[p] = 1.0 / piv;
        const double rowp = __shfl(a, p * 7 + (in ? cj : 0));      // A[p][my column]
        const double colp = __shfl(a, (in ? ri : 0) * 7 + p);      // A[my row][p]
        if (in && ri > p) a -= (colp * pinv[p]) * rowp;
    }
#pragma unroll
    for (int p = 5; p >= 0; p--) {
        d[p] = __shfl(a, p * 7 + 6) * pinv[p];
        const double up = __shfl(a, (in ? ri : 0) * 7 + p);        // U[my row][p]
        if (in && cj == 6 && ri < p) a -= up * d[p];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) okc = okc && (d[i] == d[i]);
    return okc;
}

// ---- trust-region bookkeeping of the persistent solves (TrustRegionMinimizer + LevenbergMarquardtStrategy of Ceres 2.0): the state every workgroup keeps
// in LDS and the decisions of lane 0, in Ceres' order.  The solver around it owns the system, the step and the "take" work.
struct LmTrust {
    double cost, radius, decrease, model_change, step_norm;
    int it, n_ok, term, go;    // go: 1 = evaluate the candidate next, 0 = finished
    int n_invalid;             // consecutive invalid steps (model cost change <= 0)
    int stalled;               // a bounded wait gave up
    int take;                  // the candidate was accepted
    int max_iter;
    // the solver options, parked here so that they are not live in registers across the whole launch
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
};
template <class Options>      // LmArgs, or any struct with its option members (LocalOptDev)
__device__ __forceinline__ void lm_trust_init(LmTrust& t, const Options& o) {      // ONE lane
    t.max_iter = o.max_iter;
    t.function_tolerance = o.function_tolerance; t.gradient_tolerance = o.gradient_tolerance; t.parameter_tolerance = o.parameter_tolerance;
    t.max_radius = o.max_radius; t.min_radius = o.min_radius; t.min_relative_decrease = o.min_relative_decrease;
    t.min_lm_diagonal = o.min_lm_diagonal; t.max_lm_diagonal = o.max_lm_diagonal;
    t.radius = o.initial_radius; t.decrease = 2.0; t.it = 0; t.n_ok = 0; t.term = LILI_LM_MAX_ITERATIONS; t.go = 1; t.stalled = 0; t.take = 0; t.n_invalid = 0;
    t.cost = 0.0; t.model_change = 0.0; t.step_norm = 0.0;
}
// Head of the propose loop (the whole wave; gmax = max |gradient| at the accepted point): false = the solve ends here, term and go are set.  The order is
// FinalizeIterationAndCheckIfMinimizerCanContinue's: max iterations, gradient tolerance (Ceres counts the iteration it stops in), min radius (after an invalid step).
__device__ __forceinline__ bool lm_trust_gate(LmTrust& t, const double gmax, const int lane) {
    const int it = t.it;
    if (it >= t.max_iter) { if (lane == 0) { t.term = LILI_LM_MAX_ITERATIONS; t.go = 0; } return false; }
    if (gmax <= t.gradient_tolerance) { if (lane == 0) { t.term = LILI_LM_GRADIENT_TOLERANCE; t.it = it + 1; t.go = 0; } return false; }
    if (!(t.radius > t.min_radius)) { if (lane == 0) { t.term = LILI_LM_MIN_RADIUS; t.go = 0; } return false; }      // MinTrustRegionRadiusReached
    return true;
}
// Not a descent step of the model (or no factorisation) = Ceres' INVALID step (TrustRegionMinimizer::HandleInvalidStep): the iteration counts, nothing is
// evaluated, LevenbergMarquardtStrategy::StepIsInvalid halves the radius (the rejection divisor is left alone); max_num_consecutive_invalid_steps (5) of them
// in a row end the solve with FAILURE.  The whole wave; radius, it = what the wave read at the loop head.  false = the solve ends here.
__device__ __forceinline__ bool lm_trust_invalid(LmTrust& t, const double radius, const int it, const int lane) {
    const int n_inv = t.n_invalid + 1;
    LILI_WAVE_SYNC();
    if (lane == 0) { t.n_invalid = n_inv; t.radius = radius * 0.5; t.it = it + 1; }
    if (n_inv >= 5) { if (lane == 0) { t.term = LILI_LM_NUMERICAL_FAILURE; t.go = 0; } return false; }
    LILI_WAVE_SYNC();
    return true;          // (the loop head checks max iterations, then the radius)
}
// The candidate's cost is known: accept or reject, by ONE lane.  xnorm = |x| at the accepted point.  `boss` writes row n_log of summary->it.  Sets cost, radius,
// decrease, n_ok, it, term, go, take and returns `accepted`; what "taking" the candidate means is the caller's.  The log row, the order of the checks and the
// minimum-radius exit are TrustRegionMinimizer's and the same for every strategy; how the radius moves is the strategy's: accepted_radius(t, rho) and
// rejected_radius(t) (lambdas or functors, inlined).
template <class Accepted, class Rejected>
__device__ __forceinline__ int lm_trust_judge_with(LmTrust& t, const double new_cost, const double xnorm, lili_lm_summary* summary, int& n_log, const bool boss,
                                                   Accepted accepted_radius, Rejected rejected_radius) {
    int accepted = 0, stop = 0;
    const double rho = (t.cost - new_cost) / t.model_change;
    if (boss && summary && n_log < LILI_LM_MAX_LOG) {
        lili_lm_iteration& L = summary->it[n_log];
        L.cost = t.cost; L.new_cost = new_cost; L.rho = rho; L.radius = t.radius; L.step_norm = t.step_norm; L.accepted = 0; L.iteration = t.it;
    }
    if (t.stalled) { t.term = LILI_LM_STALLED; stop = 1; }
    // Ceres returns from ParameterToleranceReached / FunctionToleranceReached BEFORE IsStepSuccessful / HandleSuccessfulStep
    // (TrustRegionMinimizer::Minimize): the candidate that triggers a tolerance is never taken, x stays at the last accepted point
    else if (t.step_norm <= t.parameter_tolerance * (xnorm + t.parameter_tolerance)) { t.term = LILI_LM_PARAMETER_TOLERANCE; stop = 1; }
    else if (fabs(t.cost - new_cost) <= t.function_tolerance * t.cost) { t.term = LILI_LM_FUNCTION_TOLERANCE; stop = 1; }
    else if (rho > t.min_relative_decrease) {
        accepted = 1;
        accepted_radius(t, rho);
    } else {
        // StepRejected; MinTrustRegionRadiusReached ends the solve (CONVERGENCE) once the radius is at or below min_trust_region_radius
        rejected_radius(t);
        if (!(t.radius > t.min_radius)) { t.term = t.it + 1 >= t.max_iter ? LILI_LM_MAX_ITERATIONS : LILI_LM_MIN_RADIUS; stop = 1; }      // (max iterations is checked first)
    }
    if (accepted) { t.cost = new_cost; t.n_ok++; }
    if (boss && summary && n_log < LILI_LM_MAX_LOG) summary->it[n_log].accepted = accepted;
    n_log++;
    t.it++;
    t.go = stop ? 0 : 1;
    t.take = accepted;
    return accepted;
}
// LevenbergMarquardtStrategy: StepAccepted's cubic, clamped to max_radius; StepRejected divides by a divisor that doubles with every rejection in a row, no clamp
__device__ __forceinline__ int lm_trust_judge(LmTrust& t, const double new_cost, const double xnorm, lili_lm_summary* summary, int& n_log, const bool boss) {
    return lm_trust_judge_with(t, new_cost, xnorm, summary, n_log, boss,
        [](LmTrust& s, const double rho) {
            const double f = 2.0 * rho - 1.0;
            s.radius = fmin(s.max_radius, s.radius / fmax(1.0 / 3.0, 1.0 - f * f * f));
            s.decrease = 2.0;
        },
        [](LmTrust& s) { s.radius = s.radius / s.decrease; s.decrease *= 2.0; });
}
__device__ __forceinline__ void lm_write_summary(lili_lm_summary* summary, const LmTrust& t, const double cost0, const int n_log, const int* counts) {
    summary->iterations = t.it; summary->successful_steps = t.n_ok; summary->termination = t.term;
    summary->initial_cost = cost0; summary->final_cost = t.cost; summary->final_radius = t.radius;
    summary->n_logged = n_log < LILI_LM_MAX_LOG ? n_log : LILI_LM_MAX_LOG;
    summary->n_surf = counts[0]; summary->n_edge = counts[1];
}

}  // namespace lili
