// Internal: forward declarations of every kernel that a file other than its own launches (definitions: lili_s2m.hip, lili_s2m_coop.hip, lili_s2m_dense.hip,
// lili_s2m_lm.hip) — the only place a kernel is declared for another file — and the launch helper.
#pragma once
#include "lili_ctx.h"

#include <hip/hip_ext.h>

namespace lili {
// kernels (lili_s2m.hip)
__global__ void k_cloud_to_f4(const unsigned char*, int, int, int, float4*, unsigned*);
__global__ void k_bbox(const float4*, int, unsigned*);
__global__ void k_bbox_dev(const float4*, const int*, int, unsigned*);
__global__ void k_bbox_src(SrcCloud, int, unsigned*);
__global__ void k_cell_count(SrcCloud, int, GridView, int*, int*, unsigned long long*, int, float);
__global__ void k_scan_block_sums(const int*, int64_t, int*);
__global__ void k_scan_sums(int*, int);
__global__ void k_scan_apply(const int*, int64_t, const int*, int*);
template <bool NARROW> __global__ void k_scan_lookback_t(int*, const unsigned char*, int64_t, unsigned long long*, unsigned*);
__global__ void k_cell_count_narrow(SrcCloud, int, GridView, unsigned*, unsigned char*, unsigned long long*, int, float);
template <typename RankT> __global__ void k_scatter_t(SrcCloud, int, GridView, const RankT*, const int*, float4*, float*);
__global__ void k_start9(const int*, GridView, const int*, int*);
__global__ void k_rowtot9(const int*, GridView, int*);
template <int BS> __global__ void k_associate_lin(AssocArgs, AssocArgs, PoseArg, MatchParams, double*, double*);
__global__ void k_scatter9(const int*, GridView, const int*, float4*, float*, int);
template <int BS> __global__ void k_associate_surf(const float4*, int, GridView, PoseArg, MatchParams, float4*, double*, unsigned char*, int*, float*, int*);
template <int BS> __global__ void k_associate_edge(const float4*, int, GridView, PoseArg, MatchParams, float4*, float4*, unsigned char*, int*, float*, int*);
__global__ void k_associate_both(AssocArgs, AssocArgs, PoseArg, MatchParams);
__global__ void k_linearize(LinArgs, LinArgs, PoseArg, MatchParams, const SlotState*, const int*, FuseTail);
__global__ void k_reduce_partials(const double*, int, const double*, int, double*, SlotState*, int, P2PView, unsigned long long, double*, SlotState*, const SlotState*);
__global__ void k_sum_counts(const int*, int, const int*, int, SlotState*, int*, P2PView);
__global__ void k_gn_update(const double*, SlotState*, const SlotState*);
__global__ void k_pose_copy(SlotState*, const SlotState*);
__global__ void k_window_reduce(WindowArgs, double*, int, P2PView);
__global__ void k_linearize_window(WinLinArgs, MatchParams);
__global__ void k_window_gn(WindowArgs, const double*);
__global__ void k_window_counts(WindowArgs, int*, P2PView);
// lili_s2m_dense.hip: the association on a dense map (fine index)
__global__ void k_associate_fine(AssocArgs, int, int, int, PoseArg, MatchParams);
// lili_s2m_lm.hip: the Levenberg-Marquardt loop on fixed correspondences, one persistent launch
__global__ void k_solve_lm(LmArgs, MatchParams);
__global__ void k_solve_lm_window(WinLmArgs, MatchParams);
// lili_s2m_coop.hip: L lanes per query (small launches)
template <int L, bool LIN> __global__ void k_associate_coop(AssocArgs, AssocArgs, PoseArg, MatchParams, double*, double*, SlotState*, int);
template <int L> __global__ void k_associate_coop_window(WinAssocArgs, MatchParams);
template <int L> __global__ void k_iterate_coop(AssocArgs, AssocArgs, MatchParams, IterArgs);
// lili_imu.hip: IMU pre-integration, one workgroup per segment
__global__ void k_imu_preintegrate(const ImuSegDev*, const double*, ImuOutDev*);
// lili_local_graph.hip: IMU walk and local pose graph, one workgroup of one wave
__global__ void k_local_graph(const LocalGraphIn*, LocalGraphOut*);
// lili_pose_graph.hip: the global pose graph, one launch per stage of a Gauss-Newton iteration
__global__ void k_pg_append(const double*, int, int, double*, double*);
__global__ void k_pg_linearize(PgDev);
__global__ void k_pg_assemble(PgDev);
__global__ void k_pg_gate(PgDev, int);
__global__ void k_pg_eliminate(PgDev);
__global__ void k_pg_reduced_assemble(PgDev);
__global__ void k_pg_reduced_solve(PgDev);
__global__ void k_pg_backsub(PgDev);
__global__ void k_pg_retract_cost(PgDev);
}  // namespace lili

// lili_map.hip: the three-kernel exclusive scan (k_scan_block_sums, k_scan_sums, k_scan_apply) of n words into out[0 .. n]; in == out is allowed
int lili_scan_exclusive3(lili_ctx* ctx, const int* in, int64_t n, lili_detail::DevBuf& sums, int* out);
// lili_archive.hip: float4 rows of device memory into a caller's lili_feature_out — enqueued only (*copied: the rows covered), or with the stream synchronised behind it
int copy_rows_enqueue(lili_ctx* ctx, const void* d_rows, size_t count, lili_feature_out* out, const char* what, size_t* copied);
int copy_rows_out(lili_ctx* ctx, const void* d_rows, size_t count, lili_feature_out* out, const char* what);
// lili_archive.hip -> lili_place.hip: what place recognition reads of the archive — its size, its reset count (a descriptor outlives no reset), a keyframe's rows of one kind
// (device float4 rows, complete once the context's stream has been synchronised) and time
struct lili_archive_rows { const float4* p = nullptr; int n = 0; double time = 0; };
int lili_archive_size(lili_ctx* ctx);
unsigned long long lili_archive_resets(lili_ctx* ctx);
lili_archive_rows lili_archive_rows_of(lili_ctx* ctx, int id, int kind);
void lili_archive_map_pose_of(lili_ctx* ctx, int id, double pose[7]);      // keyframe id's LiDAR map pose (p, then q w x y z) as the archive holds it now
// lili_match.hip -> lili_window.hip (the lidar blocks of the joint window)
int lili_match_window_records(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params, const double* t, const double* q, double* d_gram);
int lili_match_lm_args(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, const lili_lm_options* options, int max_blocks, lili::LmArgs* out);
lili::MatchParams lili_match_device_params(const lili_s2m_params* params);

// A kernel launch that may drop the barrier against the kernels enqueued before it on the stream (`any_order`: hipExtAnyOrderLaunch — the AQL packet goes without the
// barrier bit, so it is dispatched as soon as the packets in front of it have been DISPATCHED, not completed).  Only the association that follows a reduction + GN
// kernel uses it (option "overlap_gn"): its waves poll for the pose that kernel publishes.  Where the runtime ignores the flag the launch is an ordinary one.
template <typename K, typename... A>
static inline void launch_k(hipStream_t stream, bool any_order, K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
    if (any_order) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, nullptr, nullptr, hipExtAnyOrderLaunch, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}
