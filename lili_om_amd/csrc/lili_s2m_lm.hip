// Device Levenberg-Marquardt on fixed correspondences, ONE launch.
//
// What it replaces: the reference hands the residual blocks of a keyframe to ceres::Solve (L/src/BackendFusion.cpp:984-992: DENSE_QR,
// max_num_iterations = max_num_iter (15), everything else Ceres 2.0 defaults) — a trust-region loop that EVALUATES all
// blocks once per iteration and accepts or rejects the step by the robust cost.  lili_s2m_iterate_inner ran plain Gauss-Newton steps,
// one launch per evaluation (14.7 us at 200 k records); a caller that wanted Ceres' accept / reject had to come back to the host
// after every evaluation.  Here the whole loop is one persistent kernel:
//
//   evaluation   every workgroup linearises its share of the records at the candidate pose (lin_surf_body / lin_edge_body of
//                lili_s2m_dev.h: robustified rows, f64-MFMA Gram, block partial incl. the robust cost) and PUBLISHES the 40-double partial
//                as 16-byte granules {value, value ^ key}, key unique per (launch, evaluation): the data is its own flag
//                (cdna_hip_programming.md Guideline 16 form R2: one write-through store per granule, relaxed agent-scope loads, no fence)
//   exchange     by ONE polling wave per workgroup.  Up to 16 workgroups (8 k records): one hop — everybody adds all partials in index order.
//                More: two hops — the first workgroup of every group of 16 adds its members' partials in index order and publishes the
//                group sum; every workgroup then adds the <= 15 group sums in index order.  Fixed order,
//                so every workgroup holds the SAME 40 doubles bit for bit — no broadcast of the decision is needed: each workgroup
//                runs the trust-region step itself (6x6 LDL^T in one lane) and arrives at the same candidate pose.  Partial / group
//                buffers are double-buffered by the parity of the evaluation: a workgroup can start evaluation e + 1 only after it has
//                read every partial of e, so nobody overwrites what somebody still reads.
//   step logic   TrustRegionMinimizer + LevenbergMarquardtStrategy of Ceres 2.0 (the checker's restatement is what tests/test_lm_gpu.py compares with): Jacobi scaling from
//                the first Jacobian, D^2 = clamp(diag) / radius, model cost change, relative decrease rho, parameter / function /
//                gradient tolerances checked in Ceres' order, radius update radius / max(1/3, 1 - (2 rho - 1)^3) or halving with a
//                doubling divisor.  The linear system is solved on the 6x6 normal equations (the Gram is what the evaluation produces);
//                Ceres' DENSE_QR works on the stacked rows — the same minimiser up to rounding, which tests/test_lm_gpu.py bounds by
//                comparing every accept / reject decision and the final pose with the CPU restatement's loop on per-residual rows.
//
// All workgroups must be co-resident (<= one per CU: 512 threads at up to 256 VGPRs, 48 KB LDS); every wait is bounded and ends the launch with
// termination = LILI_LM_STALLED instead of hanging the GPU.
#include "lili_solve_dev.h"

namespace lili {

struct LmShared {
    double vals[kLmGroup][40];
    double tot[40];            // sum of all partials of the current evaluation (upper triangle of the 8x8 Gram, [36] cost, [37] rows)
    double cur[40];            // the same at the accepted point x
    double full[64];           // symmetric 8x8 Gram of `cur`
    double H[6][6], gv[6];     // local-coordinate normal matrix P^T G P and gradient P^T G_7r at x
    double Hs[6][6], gs[6];    // the same in Jacobi-scaled coordinates (S H S, S g): what the trust-region step works on
    double x[7], xn[7];        // accepted point, candidate
    double scale[6];
    LmTrust t;                 // trust-region state and options; t.take: `tot` becomes `cur`
    int counts[2];
};

// H = P^T G77 P, gv = P^T G7r at the quaternion of sh.x (lanes 0..41 of ONE wave)
__device__ __forceinline__ void lm_local_system(LmShared& sh) {
    const int tid = threadIdx.x & 63;
    if (tid < 42) {
        const int a = tid < 36 ? tid / 6 : tid - 36, b = tid < 36 ? tid % 6 : 7;
        const double v = pose_local_entry(sh.full, sh.x + 3, a, b);
        if (tid < 36) sh.H[a][b] = v; else sh.gv[a] = v;
    }
}

// Jacobi-scaled system of the accepted point (lanes 0..41 of one wave, after lm_local_system and with sh.scale set)
__device__ __forceinline__ void lm_scaled_system(LmShared& sh) {
    const int tid = threadIdx.x & 63;
    if (tid < 36) sh.Hs[tid / 6][tid % 6] = sh.H[tid / 6][tid % 6] * sh.scale[tid / 6] * sh.scale[tid % 6];
    else if (tid < 42) sh.gs[tid - 36] = sh.gv[tid - 36] * sh.scale[tid - 36];
}
// The trust-region step from the accepted point, by ONE WAVE (all 64 lanes call it, control flow uniform).  Returns with sh.t.go = 1 and sh.xn =
// candidate, or sh.t.go = 0 (finished).  The 6x6 system (H_s + D^2) d = -g_s goes through solve6_wave.
// Every workgroup runs the same instruction sequence on the same bits, so the candidates agree bit for bit across workgroups.
__device__ __forceinline__ void lm_propose(LmShared& sh) {
    LmTrust& t = sh.t;
    const int lane = threadIdx.x & 63;
    const int ri = lane / 7, cj = lane - 7 * ri;             // row / column of the augmented 6 x 7 matrix (lanes >= 42 idle along)
    const bool in = lane < 42;
    for (;;) {
        const int it = t.it;
        double gmax = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) gmax = fmax(gmax, fabs(sh.gv[i]));
        if (!lm_trust_gate(t, gmax, lane)) return;
        const double radius = t.radius;
        double a = 0.0;
        if (in) {
            if (cj < 6) {
                a = sh.Hs[ri][cj];
                if (cj == ri) a += fmin(fmax(a, t.min_lm_diagonal), t.max_lm_diagonal) / radius;      // D^2 = clamp(diag H_s) / radius
            } else a = -sh.gs[ri];
        }
        double d[6];
        if (!solve6_wave(a, d)) { if (lane == 0) { t.term = LILI_LM_NUMERICAL_FAILURE; t.go = 0; } return; }
        // model_cost_change = -d^T (g_s + H_s d / 2): row sums on six lanes, then a fixed-order sum
        double tr = 0.0;
        if (lane < 6) {
            double hd = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) hd += sh.Hs[lane][j] * d[j];
            double dl = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) dl = lane == j ? d[j] : dl;
            tr = dl * (sh.gs[lane] + 0.5 * hd);
        }
        double mc = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) mc += __shfl(tr, i);
        mc = -mc;
        if (!(mc > 0.0)) {
            if (!lm_trust_invalid(t, radius, it, lane)) return;
            continue;
        }
        if (lane == 0) {
            double n2 = 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) { d[i] = d[i] * sh.scale[i]; n2 += d[i] * d[i]; }      // delta in the unscaled local coordinates
            t.model_change = mc;
            t.n_invalid = 0;
            t.step_norm = sqrt(n2);
            sh.xn[0] = sh.x[0] + d[0]; sh.xn[1] = sh.x[1] + d[1]; sh.xn[2] = sh.x[2] + d[2];
            quat_plus(sh.x + 3, d + 3, sh.xn + 3, sinc_cos_halving);
            t.go = 1;
        }
        return;
    }
}

// one slot's solve, by the workgroups [0, a.nb) of that slot (b = the workgroup's index within the slot)
__device__ __forceinline__ void solve_lm_body(const LmArgs& a, const MatchParams& P, const int b, double* lds, LmShared& sh) {
    const bool surf = b < a.S.nb;
    const bool wave0 = threadIdx.x < 64;
    const bool boss = b == 0 && threadIdx.x == 0;
    // correspondence counts (ROT residual scale num / N): fixed for the whole solve, summed once from the association's block counts
    {
        const int n_s = (a.S.n_q > 0 && a.S.block_counts) ? sum_block_counts(a.S.block_counts, a.S.n_bc) : 0;
        __syncthreads();
        const int n_e = (a.E.n_q > 0 && a.E.block_counts) ? sum_block_counts(a.E.block_counts, a.E.n_bc) : 0;
        if (threadIdx.x == 0) {
            sh.counts[0] = n_s; sh.counts[1] = n_e;
            for (int i = 0; i < 7; i++) { sh.x[i] = a.state->pose[i]; sh.xn[i] = sh.x[i]; }
            lm_trust_init(sh.t, a);
        }
        __syncthreads();
    }
    LinArgs S = a.S, E = a.E;
    S.block_counts = nullptr; E.block_counts = nullptr;         // the bodies then take N from n_global (= sh.counts)
    int n_log = 0;
    double cost0 = 0.0;
    for (int eval = 0;; eval++) {
        const int par = eval & 1;
        const unsigned long long key = xchg_key(a.launch, eval);
        double* part = a.part + (size_t)par * a.nb * kPartialStride;
        double* gsum = a.gsum + (size_t)par * a.ng * kPartialStride;
        PoseArg pa{};
        for (int i = 0; i < 3; i++) pa.t[i] = sh.xn[i];
        for (int i = 0; i < 4; i++) pa.q[i] = sh.xn[3 + i];
        pa.state = nullptr; pa.derive_assoc = 0;
        // ---- evaluation at the candidate: this workgroup's partial, published as granules
        S.partials = part; E.partials = part + (size_t)a.S.nb * kPartialStride;
        if (surf) lin_surf_body(S, b, pa, P, a.state, sh.counts, lds, key);
        else lin_edge_body(E, b - a.S.nb, pa, P, a.state, sh.counts, lds, key);
        // ---- exchange (wave 0): group sums, then the total, both in index order
        if (wave0) {
            const bool ok = xchg_total<40>(part, gsum, b, a.nb, a.ng, key, sh.vals, sh.tot);
            if (!ok && threadIdx.x == 0) sh.t.stalled = 1;
            // ---- step logic, identical in every workgroup
            if (eval == 0) {
                // first evaluation: x0 is the accepted point; Jacobi scaling 1 / (1 + sqrt(diag J^T J)) from this Jacobian, kept for the whole solve
                if (threadIdx.x < 40) sh.cur[threadIdx.x] = sh.tot[threadIdx.x];
                LILI_WAVE_SYNC();
                gram_tri_to_full(sh.cur, sh.full);
                LILI_WAVE_SYNC();
                lm_local_system(sh);
                LILI_WAVE_SYNC();
                if (threadIdx.x < 6) sh.scale[threadIdx.x] = 1.0 / (1.0 + sqrt(sh.H[threadIdx.x][threadIdx.x]));
                if (threadIdx.x == 0) { sh.t.cost = sh.cur[36]; cost0 = sh.t.cost; }
                LILI_WAVE_SYNC();
                lm_scaled_system(sh);
                LILI_WAVE_SYNC();
                if (threadIdx.x == 0 && sh.t.stalled) { sh.t.term = LILI_LM_STALLED; sh.t.go = 0; }
            } else {
                // the candidate's cost is known: accept or reject (Ceres checks both tolerances on the candidate first)
                if (threadIdx.x == 0) {
                    const double xnorm = sqrt(sh.x[0] * sh.x[0] + sh.x[1] * sh.x[1] + sh.x[2] * sh.x[2] + sh.x[3] * sh.x[3] + sh.x[4] * sh.x[4] + sh.x[5] * sh.x[5] + sh.x[6] * sh.x[6]);
                    if (lm_trust_judge(sh.t, sh.tot[36], xnorm, a.summary, n_log, boss)) { for (int i = 0; i < 7; i++) sh.x[i] = sh.xn[i]; }
                }
                LILI_WAVE_SYNC();
                const bool take = sh.t.take != 0;
                if (take && threadIdx.x < 40) sh.cur[threadIdx.x] = sh.tot[threadIdx.x];
                LILI_WAVE_SYNC();
                if (take) {
                    gram_tri_to_full(sh.cur, sh.full);
                    LILI_WAVE_SYNC();
                    lm_local_system(sh);
                    LILI_WAVE_SYNC();
                    lm_scaled_system(sh);
                }
            }
            LILI_WAVE_SYNC();
            if (sh.t.go) lm_propose(sh);      // the next candidate (or the end), from the accepted point — the whole wave, ONE call site
            LILI_WAVE_SYNC();
        }
        __syncthreads();
        if (!sh.t.go) break;
    }
    if (boss) {
        for (int i = 0; i < 7; i++) a.state->pose[i] = sh.x[i];
        a.state->gn_status = (sh.t.term == LILI_LM_STALLED || sh.t.term == LILI_LM_NUMERICAL_FAILURE) ? 1 : 0;
        a.state->iters += sh.t.n_ok;
        if (a.summary) lm_write_summary(a.summary, sh.t, cost0, n_log, sh.counts);
    }
}

// persistent launch: grid = S.nb + E.nb workgroups of kLmThreads threads; dynamic LDS = kLmThreads * kRow doubles (Gram staging rows)
__global__ __launch_bounds__(kLmThreads) void k_solve_lm(LmArgs a, MatchParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ LmShared sh;
    solve_lm_body(a, P, (int)blockIdx.x, lds, sh);
}
// The solves of ALL keyframes of a sliding window in ONE launch (round 6): workgroup bid belongs to the last slot whose first_block <= bid and is that slot's workgroup
// bid - first_block of k_solve_lm — the slots' solves are independent (own records, own partial buffers, own keys) and run side by side, one slot's exchange under another's
// arithmetic.  It was one launch per slot on forked streams: 65 us of fork / join / launch overhead per window solve around 9 us per evaluation of all three keyframes.
__global__ __launch_bounds__(kLmThreads) void k_solve_lm_window(WinLmArgs W, MatchParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ LmShared sh;
    const int bid = (int)blockIdx.x;
    int i = 0;
#pragma unroll
    for (int k = 1; k < kWindowMaxSlots; k++) if (k < W.n && bid >= W.first_block[k]) i = k;
    solve_lm_body(W.a[i], P, bid - W.first_block[i], lds, sh);
}

}  // namespace lili
