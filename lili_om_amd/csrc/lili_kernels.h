// Kernel-side declarations shared by the translation units of liblili_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lili_hip.h"
#include "lili_p2p_dev.h"

namespace lili {

// Uniform-grid index over the local map (replaces the FLANN kd-tree).
// Points are stored cell-sorted as float4 (x, y, z, bitcast(original index)); cell_start has
// n_cells+1 entries; cells are x-fastest so the 3 x-neighbours of a cell are one contiguous run.
// With super-rows, `pts` / `aux` continue behind the n_points base entries with the super-row copy (same float4 layout).
struct GridView {
    const float4* pts;      // cell-sorted map points
    const float* aux;       // cell-sorted auxiliary float (Livox reflectivity) or nullptr
    const int* cell_start;  // [n_cells + 1]
    const int* cell_start9; // super-row index (k_start9 in lili_s2m.hip) or nullptr: [bnx*bny*bnz + 1] positions in the unified array
    int bx0, by0, bz0, bnx, bny, bnz;   // the box of cells that has super-rows (the whole grid, or the cells around lili_map_focus)
    double ox, oy, oz;      // grid origin
    double inv_cell;        // 1 / cell edge
    double cell;            // 1 / inv_cell (the value the pruning bounds use)
    int nx, ny, nz;
    int n_points;
    int reach;              // neighbourhood half-width in cells: reach * cell edge >= 1.01 * gate radius (1 or 2)
};

// A caller's point cloud as the map-index build reads it (round 4: no float4 copy of the map any more): device pointer, byte stride, byte offset of the
// auxiliary float or < 0.  `f4`: stride 16, 16-byte aligned, aux at offset 12 or absent — one 16-byte load per point.
struct SrcCloud {
    const unsigned char* p;
    int stride, aux_off;
    int f4;
};

// Per-slot state that lives in device memory so that outer iterations need no host round trip.
struct SlotState {
    double pose[7];   // body pose: t(3), q(w,x,y,z)
    int n_res[2];     // correspondences of the last associate: [surf, edge]
    int gn_status;    // 0 ok, 1 = normal matrix not positive definite (pose left unchanged)
    int iters;        // GN updates applied since pose_set
    double last_delta[6];
    long long tprof[16];   // profiling aid (LILI_DEBUG bit 256): s_memrealtime stamps (100 MHz) of one block per kernel
    unsigned int reserved_;
    unsigned long long cnt_word;   // k_associate_coop's in-launch count barrier: [0,24) surf correspondences, [24,48) edge, [48,64) workgroups arrived; k_reduce_partials zeroes it
    unsigned long long epoch;   // fused linearisation launches of this slot so far: launch_key(epoch) tags the granules of the next one
    // Round 5, option "overlap_gn": raised (sticky) by an association launch that gave up waiting for the pose the Gauss-Newton kernel in front of it publishes
    // (PosePub below).  Behind `epoch`: lili_s2m_pose_set does not touch it.
    unsigned long long wait_failed;
};
// The pose of the last Gauss-Newton update PUBLISHED for an association launch that is already running (option "overlap_gn"): seven 16-byte granules
// {value, value ^ key}, key unique per update (the data is its own flag, as the partials of the fused tail), in kPubReplicas copies 128 bytes apart — the 3 125 waves
// of the association poll, and all of them on ONE line queue up on one memory channel behind each other (and the publishing store behind them: measured, the overlap
// then gains nothing); workgroup b polls copy b mod kPubReplicas.
constexpr int kPubReplicas = 64;
constexpr int kPubStride = 16;      // doubles per copy: 7 granules + padding to 128 bytes

// Fused tail of a linearisation launch (see fused_tail in lili_s2m.hip)
struct FuseTail {
    int mode;                  // 0 = off, 1 = reduce to `out`, 2 = reduce + GN update, 3 = publish the partials as granules only
    const double* part_surf; int nb_surf;
    const double* part_edge; int nb_edge;
    double* out;
    SlotState* state;
    int debug;                 // LILI_DEBUG bits (256: phase stamps of the reducer block)
    const SlotState* pose_src; // mode 2: the slot whose pose the Gauss-Newton step starts from (the first step after a restart), or nullptr = state
};


// Pose argument of a kernel: either by value (host-provided) or read from SlotState.
struct PoseArg {
    double t[3];
    double q[4];
    const SlotState* state;  // if non-null, the body pose is read from state->pose
    int derive_assoc;        // associate only: derive (Q2,T2) = (Q*q_lb^-1, T - Q2*t_lb) from the body pose
    const double* pub;             // the slot's kPubReplicas x kPubStride published-pose copies (wait_key != 0)
    unsigned long long wait_key;   // associate only, != 0: the launch may have started BEFORE the reduction + GN kernel in front of it has finished (no barrier between the two
                                   // dispatches): the pose is taken from state->pose_pub once all seven granules carry this key
};

struct MatchParams {     // device copy of lili_s2m_params (+ derived values)
    int variant, loss;
    double loss_a, lidar_const, kd_max_radius, edge_gate, surf_dist_thres, reflect_thres, surf_weight_min, edge_dist_max;
    double q_lb[4], t_lb[3];
    double q_lb_inv[4];   // Eigen inverse() of q_lb (conjugate / squared norm), computed once on the host: IEEE divisions, same bits
    double q_lb_inv_jet[4];   // the same inverse as the plane factor sees it on ceres::Jet (LidarKeyframeFactor.h:86): conjugate * (1 / n2)
    double scale_surf_num, scale_edge_num;
    int no_cost;   // 1: the robust cost value (slot 64 of the Gram record) is not computed — the fused iterate loops, whose record never leaves the library
    int debug;   // LILI_DEBUG env, tests and profiling builds only: 256 / 512 = clock stamps of the linearisation / reduction / association prologue into SlotState::tprof,
                 // 2048 = never fall back to the pivoted QR, 16384 = always the pivoted QR, 32768 = exact (d2, index) selector only (the tier tests force both tiers and
                 // compare bit for bit), 4096 = per-workgroup timestamps (only in a -DLILI_PHASE_PROBE build: tools/assoc_blocks.py, tools/assoc_phases.sh)
    int assoc_prio;   // option "assoc_prio" (lili_ctx.h), set by the launchers of the one-lane association kernels and of k_associate_coop<L, false> alone (with_prio, lili_match.hip): the
                      // waves run at issue priority 1 while they search and at 0 from the fit on (phase_prio, lili_s2m_dev.h)
};

// Arguments of one kind (surf or edge) of the combined linearisation launch k_linearize.
struct LinArgs {
    const float4* queries; int n_q;
    const float4* rec0;            // surf: (w*n, w*d); edge: (A, s)
    const void* rec1;              // surf: double score[]; edge: float4 (B, 0)
    const unsigned char* valid;
    const int* block_counts; int n_bc;   // per-block correspondence counts of the association launch (nullptr: use n_global / state)
    double* partials;
    int nb;                        // linearisation blocks of this kind
};
// Arguments of one kind of the combined association launch k_associate_both.
struct AssocArgs {
    const float4* queries; int n_q; GridView g;
    float4* rec0; void* rec1; unsigned char* valid;
    int* dbg_idx; float* dbg_d2; int* block_counts;
    int nb;
};

// The slots of a sliding window handed to ONE reduction / count launch (k_window_reduce, k_window_counts in lili_s2m.hip)
constexpr int kWindowMaxSlots = 8;
static_assert(kWindowMaxSlots == LILI_MAX_SLOTS, "a window launch carries every slot of a context");
struct WindowSlot {
    const double* part_surf; int nb_surf;      // block partials of the slot's last linearisation (k_linearize)
    const double* part_edge; int nb_edge;
    const int* bc_surf; int nbc_surf;          // per-block correspondence counts of the slot's last association
    const int* bc_edge; int nbc_edge;
    SlotState* state;
};
struct WindowArgs { WindowSlot s[kWindowMaxSlots]; int n; };
// The linearisation of EVERY slot of the window in ONE launch (k_linearize_window): slot i owns the blocks [first_block, first_block + S.nb + E.nb)
// of the grid and runs exactly the bodies k_linearize runs for it (same block geometry, same partial buffers) — one launch boundary per
// evaluation of the joint window instead of one per keyframe (the reference evaluates all keyframes per solver evaluation, L/src/BackendFusion.cpp:919-992).
struct WinLinSlot {
    LinArgs S, E;
    PoseArg pa;
    const SlotState* state;
    const int* n_global;           // all-reduced correspondence counts of a multi-GPU caller, else nullptr
    int first_block;
};
struct WinLinArgs { WinLinSlot s[kWindowMaxSlots]; int n; };
// The cooperative association of EVERY slot of the window in ONE launch (k_associate_coop_window in lili_s2m_coop.hip): per slot and kind what
// AssocArgs holds minus the map view, which all slots share.
struct WinAssocKind {
    const float4* queries; int n_q;
    float4* rec0; void* rec1; unsigned char* valid;
    int* dbg_idx; float* dbg_d2; int* block_counts;
    int nb;
};
struct WinAssocSlot { WinAssocKind k[2]; PoseArg pa; int first_block; };
struct WinAssocArgs { GridView g[2]; WinAssocSlot s[kWindowMaxSlots]; int n; };

constexpr int kPartialDoubles = 40;  // per-block partial: 36 upper-triangle Gram entries, cost, count, 2 spare
constexpr int kPartialStride = 80;   // doubles per block slot of the partial buffers: 40 plain doubles, or 40 16-byte granules {value, value ^ key}
constexpr int kBlock = 256;
constexpr int kAssocBlock = 64;   // association (one query per thread): one wave per workgroup, so the dispatcher balances SIMDs wave by wave
constexpr int kLinBlock = 1024;   // linearisation block (16 waves; the launch covers the queries with <= 256 blocks)
constexpr int kLmThreads = 512;   // k_solve_lm*: 8 waves: the launch may use 256 VGPRs per lane (1024-thread workgroups cap it at 128 and the loop spilled ~150 words)
constexpr int kLmGroup = 16;      // k_solve_lm*: workgroups per group sum; up to this many workgroups exchange in ONE hop (32: measured slower, one wave polls 1280 granules)

// Arguments of the Levenberg-Marquardt loop on fixed correspondences, one persistent launch (k_solve_lm, k_solve_lm_window in lili_s2m_lm.hip)
struct LmArgs {
    LinArgs S, E;                 // records of the two kinds; S.nb / E.nb = workgroups of each kind (either may be 0)
    SlotState* state;
    double* part;                 // [2 parities][nb][kPartialStride]   block partials as granules
    double* gsum;                 // [2 parities][ng][kPartialStride]   group sums as granules
    int nb, ng;
    int max_iter;
    unsigned long long launch;    // host counter: makes the granule keys of this launch unique
    lili_lm_summary* summary;     // device copy, written by workgroup 0
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
};
struct WinLmArgs { LmArgs a[kWindowMaxSlots]; int first_block[kWindowMaxSlots]; int n; };
// Arguments of the persistent outer iteration of small scans (k_iterate_coop in lili_s2m_coop.hip)
struct IterArgs {
    SlotState* state;
    double* part;                 // [2 parities][nb][kPartialStride]
    double* gsum;                 // [2 parities][ng][kPartialStride]
    double* cpart;                // [2 parities][nb + ng][4]            correspondence counts (surf, edge) as granules
    int nb, ng, n_iters, derive_assoc;
    unsigned long long launch;
};

// IMU pre-integration (k_imu_preintegrate in lili_imu.hip): one workgroup per segment.  The packed upload is the table of segment headers followed by the sample
// rows of every segment, 7 doubles each (dt, acc[3], gyr[3]); a segment owns n + 1 rows, row 0 = (0, acc0, gyr0), the constructor's pair.
constexpr int kImuThreads = 256;     // 225 of them own one entry of the 15 x 15 matrices
constexpr int kImuChunk = 64;        // samples whose state chain and F / V blocks are prepared at a time
constexpr int kImuRow = 7;
struct ImuSegDev {
    long long first_row;             // of the segment in the sample rows
    int n, predict;
    double ba[3], bg[3], g[3];
    double P0[3], R0[9], V0[3];
};
// Local pose graph (k_local_graph in lili_local_graph.hip): ONE workgroup of one wave.  The packed upload is LocalGraphIn followed by the n_rows sample rows the
// walk reads, 7 doubles each (stamp, acc[3], gyr[3]), rebased so that row 0 is sample ii0.  mode: what the launch does.
constexpr int kLocalThreads = 64;
constexpr int kLocalMaxFrames = LILI_LOCAL_MAX_FRAMES, kLocalMaxFactors = kLocalMaxFrames + 1, kLocalMaxN = 6 * kLocalMaxFrames;
constexpr int kLocalBand = 12;       // H = J^T J is block tridiagonal with 6 x 6 blocks: row i holds columns i - 11 .. i of the lower triangle, [i * kLocalBand + (i - j)]
constexpr int kLocalStageRows = 256; // sample rows kept in LDS for the walk; a longer subrange is read from global memory
constexpr int kLocalRow = 7;
enum { kLocalWalk = 1, kLocalEvaluate = 2, kLocalSolve = 4 };
struct LocalOptDev {                 // the members lm_trust_init reads
    int max_iter, pad_;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
};
struct LocalGraphIn {
    int n, mode, n_rows, f32_positions;
    LocalOptDev opt;
    double T[kLocalMaxFrames + 2];
    double P0[3], R0[9], V0[3], g[3];
    double left[7], right[7];
    double meas[kLocalMaxFactors * 7];      // read unless mode has kLocalWalk
    double poses[kLocalMaxFrames * 7];      // the state to evaluate / the initial state, unless mode has kLocalWalk
};
struct LocalGraphOut {
    double poses[kLocalMaxFrames * 7], end_state[15], meas[kLocalMaxFactors * 7];
    double cost, gradient[kLocalMaxN];
    lili_local_graph_summary summary;
    double jtj[kLocalMaxN * kLocalMaxN];    // kLocalEvaluate only: the leading (6 n)^2 doubles, row-major with stride 6 n
};
// Global pose graph (lili_pose_graph.hip).  Factor f of N nodes and L loops: 0 = the prior on node 0, 1 .. N - 1 = the chain factor (f - 1, f),
// N + l = loop l.  Separator k is node sep[k]; segment k = the nodes between separator k and separator k + 1 (or the end of the chain).
constexpr int kPgMaxNodes = LILI_PG_MAX_NODES, kPgMaxLoops = LILI_PG_MAX_LOOPS, kPgMaxLoopsExt = LILI_PG_MAX_LOOPS_EXT, kPgSegment = LILI_PG_SEGMENT;
constexpr int kPgMaxReduced = 768;   // reduced unknowns one workgroup factors (k_pg_reduced_solve): 6 x (64 + 2 x 32 separators), the default caps; beyond, the blocked solve
constexpr int kPgWide = 1024;        // threads of the single-workgroup stages (gate, reduced system, retract and cost)
constexpr int kPgCols = 13;          // columns a segment carries through its elimination: the right-hand side, 6 of its left separator, 6 of its right one
constexpr int kPgGram = kPgCols * kPgCols;
static_assert(6 * (kPgMaxNodes / kPgSegment + 2 * kPgMaxLoops) <= kPgMaxReduced && kPgMaxReduced <= kPgWide, "at the default caps the reduced system is factored by one workgroup, one row per thread");
// The blocked reduced solve: tiles of kPgTile unknowns (a multiple of 6: a separator never straddles two tiles, and of 16: the f64 matrix instruction's edge),
// the trailing update's operands staged kPgTileK columns at a time, rows padded to kPgTileLd doubles (stride = 32 banks mod 64: the four k-rows a wave reads
// at once fall on two disjoint halves of the banks)
constexpr int kPgTile = 96, kPgTileK = 16, kPgTileLd = kPgTile + 16;
static_assert(kPgTile % 6 == 0 && kPgTile % 16 == 0 && kPgTile % kPgTileK == 0 && kPgTileK % 4 == 0, "tile edge");
struct PgLoop { int from, to, sep_from, sep_to; double meas[7], w[6]; int loss, reserved_; double scale; };      // w = 1 / sqrt(variance); loss = LILI_PG_LOSS_*, scale = its k
struct PgSeg { int left, first, last, right; };      // separator node ids (right = -1: the chain ends first), interior nodes first .. last (first > last: none)
struct PgBlock { int p, q, begin, end; };            // a block (p, q), p >= q, of the reduced system that can be non-zero; its loops = ent[begin .. end)
// The fixed part, then the arrays that follow the graph (device pointers into one staged block).  An entry of a loop list is 2 l + side: in node_ent, side 1 =
// the node is loop l's `to`; in blk_ent, side 1 = the loop's (from, to) block is the transpose of block (p, q).  Every list is in loop order.
struct PgTables {
    int n, n_loops, n_sep, max_iter;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double w_prior[6], w_odom[6];
    int n_blk, damping;              // damping: 0 = none (every call but lili_pose_graph_solve_lm); 1 = + lambda on H's diagonal, 2 = + lambda h; lambda = PgState::lambda
    const int* sep;                  // n_sep
    const PgSeg* seg;                // n_sep
    const PgLoop* loop;              // n_loops
    const int* node_ptr;             // n + 1: node i's loops = node_ent[node_ptr[i] .. node_ptr[i + 1])
    const int* node_ent;             // 2 n_loops
    const PgBlock* blk;              // n_blk: the diagonal blocks, the blocks of adjacent separators, then the other pairs joined by a loop
    const int* blk_ent;              // n_loops
};
struct PgState {
    int done, fail;                  // done: the termination word — every later launch returns at its first instruction; fail: a segment met a non-positive pivot
    double cost, gmax;
    lili_pg_summary s;
    // lili_pose_graph_solve_lm only: the damping of the attempt in flight, its bounds, and the log next to s
    double lambda, lambda_factor, lambda_lower, lambda_upper;
    double lambda_log[LILI_PG_MAX_LOG];
    int accepted[LILI_PG_MAX_LOG];
    int steps_accepted, steps_rejected;
};
struct PgDev {
    const PgTables* tab;
    PgState* st;
    double *X, *Xn;                  // estimates, candidate (7 per node)
    const double* meas;              // meas[i] = the measurement of factor i (7 per node; 0: the prior's)
    double *fr, *fJ;                 // per factor: weighted residual (6), Jacobian blocks of its first and second node (2 x 36, row-major); a robust loop's carry sqrt(w) too
    double *lw;                      // per loop: its unweighted d^2 = |r|^2 and the weight w its loss gives it (1 without a loss), written by the linearisation
    double *g, *D, *S, *LB;          // gradient (6 N), diagonal blocks (36 N), sub[i] = chain block (i + 1, i) (36 N), loop blocks (from, to) (36 L)
    double *Ld, *Ls, *Y;             // per eliminated node: Cholesky factor of its pivot block (36), L block (i + 1, i) (36), the carried columns (6 x 13, column by column)
    double *gram;                    // per segment: sum of Y^T Y (13 x 13)
    double *red, *delta;             // the reduced system's lower triangle, column by column ([col * n + row]); the step (6 N)
    double *rhs;                     // the blocked solve's right-hand side in the reduced system's own order (6 n_sep)
    // lili_pose_graph_marginals only (null in a solve / an evaluation)
    double *sinv;                    // the reduced system's inverse, laid out as red; column c holds its rows >= c rounded down to a tile edge: read the lower triangle
    double *W, *P;                   // per eliminated node: -L_II^-T Y_E (6 x 12, column by column), the diagonal block of the segment's own inverse (36)
    double *cov, *cross;             // Sigma(i, i) of every node (36 N); Sigma(i, j) of every pair (36 per pair)
    const int* pairs;                // 2 ids per pair
};
struct ImuOutDev {                   // lili_window_imu's numbers, then the prediction
    double sum_dt, g[3], delta_p[3], delta_q[4], delta_v[3], lin_ba[3], lin_bg[3], jacobian[225], covariance[225];
    double P1[3], R1[9], V1[3];
};

}  // namespace lili
