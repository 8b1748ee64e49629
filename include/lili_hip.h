/*
 * lili_hip.h — C ABI of the MI355X (gfx950) hot path of LiLi-OM.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types, no
 * exceptions.  Every entry point names the reference code it replaces
 * (L/ = LiLi-OM/, R/ = LiLi-OM-ROT/ of KIT-ISAS/lili-om).  INTEGRATION.md shows the ROS-node /
 * ceres::CostFunction side binding.
 *
 * Conventions
 *   - quaternions are double[4] in (w, x, y, z) order — the order of the reference's Ceres parameter
 *     blocks (tmpQuat, L/src/BackendFusion.cpp:853-856); translations double[3].
 *   - point clouds are described by (pointer, count, stride, memory space): x,y,z are 3 floats at byte
 *     offset 0 of every point — true for pcl::PointXYZI (32 B) and pcl::PointXYZINormal (48 B,
 *     L/include/utils/common.h:71-73); `aux_offset` is the byte offset of one extra float per point
 *     (Livox: curvature = 0.1*reflectivity at 36; ROT: intensity at 16) or -1.
 *   - every function returns LILI_OK (0) or a negative error code and never throws;
 *     lili_last_error() gives the message of the last failure on that context.
 *   - a context owns one HIP stream (or borrows the caller's); it is NOT thread-safe; all work of a
 *     context is ordered on that stream.  Functions documented "async" only enqueue.
 *   - results are deterministic: no floating-point atomics anywhere; reductions have a fixed order.
 */
#ifndef LILI_HIP_H
#define LILI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LILI_ABI_VERSION 1

typedef struct lili_ctx lili_ctx;

enum {
    LILI_OK = 0,
    LILI_E_ARG = -1,      /* bad argument */
    LILI_E_HIP = -2,      /* HIP runtime error (message in lili_last_error) */
    LILI_E_STATE = -3,    /* call order violated (e.g. associate before map_set) */
    LILI_E_NOMEM = -4,
    LILI_E_NODEVICE = -5, /* no usable gfx950 device: there is no CPU fallback */
    LILI_E_NUMERIC = -6   /* a bounded iteration did not converge (lili_marg_schur, lili_window_marginalize, lili_window_cycle); nothing was written */
};
enum { LILI_KIND_SURF = 0, LILI_KIND_EDGE = 1 };
enum { LILI_MASK_SURF = 1, LILI_MASK_EDGE = 2 };
enum { LILI_VARIANT_LIVOX = 0, LILI_VARIANT_ROT = 1, LILI_VARIANT_FRONTEND = 2 };
enum { LILI_LOSS_NONE = 0, LILI_LOSS_CAUCHY = 1, LILI_LOSS_HUBER = 2 };
enum { LILI_MEM_HOST = 0, LILI_MEM_DEVICE = 1 };

#define LILI_MAX_SLOTS 8       /* sliding-window keyframes handled per context (slide_window_width = 3) */
#define LILI_GRAM_DOUBLES 72   /* device-side reduction record: 64 Gram + cost + 7 spare */

typedef struct lili_cloud {
    const void* data;   /* first point */
    size_t n;           /* number of points */
    size_t stride;      /* bytes between points (>= 12) */
    int aux_offset;     /* byte offset of the per-point auxiliary float, or -1 */
    int mem;            /* LILI_MEM_HOST or LILI_MEM_DEVICE */
} lili_cloud;

/* Matcher parameters — the ★ rows of SURVEY.md App. C. */
typedef struct lili_s2m_params {
    int variant;             /* LILI_VARIANT_*: which findCorresponding* / factor flavour */
    int loss;                /* LILI_LOSS_*: CauchyLoss(1.0) L/src/BackendFusion.cpp:845; HuberLoss(0.1) L/src/LidarOdometry.cpp:507 */
    double loss_a;
    double lidar_const;      /* L/config/config_fr_iosb.yaml:18 (20), R/config/config_fr_iosb.yaml:30 (7.5) */
    double kd_max_radius;    /* compared with a SQUARED distance, L/src/BackendFusion.cpp:1615 */
    double edge_gate;        /* 1.0, L/src/BackendFusion.cpp:1543 (squared distance too) */
    double surf_dist_thres;  /* L:1651 */
    double reflect_thres;    /* Livox only, L:1628 */
    double surf_weight_min;  /* 0.2 L:1665 / 0.3 R/src/BackendFusion.cpp:1504 / 0.4 L/src/LidarOdometry.cpp:400 */
    double edge_dist_max;    /* ROT only, R/src/BackendFusion.cpp:1443 (0.1); <= 0 disables */
    double q_lb[4];          /* extrinsic rotation, (w,x,y,z), L/config/config_fr_iosb.yaml:35-38 */
    double t_lb[3];          /* extrinsic translation */
    double scale_surf_num;   /* ROT: residual scale = num / N_surf (1000, R/src/BackendFusion.cpp:861); 0 = no count scaling */
    double scale_edge_num;   /* ROT: 200 / N_edge (R/src/BackendFusion.cpp:843); 0 = none */
} lili_s2m_params;

/* ---- context -------------------------------------------------------------------------------- */

/* Creates a context on HIP device `device`.  `stream` is a hipStream_t to enqueue on (e.g. the
 * caller's current stream so that RCCL collectives interleave correctly), or NULL to create one.
 * Fails with LILI_E_NODEVICE when no gfx950 device is usable — there is no CPU path. */
int lili_ctx_create(lili_ctx** out, int device, void* stream);
void lili_ctx_destroy(lili_ctx* ctx);
const char* lili_last_error(const lili_ctx* ctx);
int lili_abi_version(void);
/* Blocks until everything enqueued on the context's stream has finished. */
int lili_sync(lili_ctx* ctx);
/* When enabled, associate also stores the 5 neighbour indices / squared distances per query so that
 * lili_s2m_get_neighbors can return them (parity tests).  Off by default (extra HBM writes). */
int lili_set_debug(lili_ctx* ctx, int keep_neighbors);
/* Tuning knobs that never change any result bit (the closed experiments "bin_queries", "tiled", "nn_cache" and "balance" were removed in round 5:
 * profiles/EXPERIMENTS.md; an unknown name returns LILI_E_ARG):
 *   map index     "max_cells" (cap on grid cells; coarser cells stay exact), "grid_reach" (1 = cells of the gate radius, 27-cell search; 2 = smaller
 *                 cells, inner 27 first and the shell of the 125-cell block on demand; default 2), "cell_pct" (reach 2: cell edge in % of the gate radius,
 *                 50..100, default 65), "super_rows" (1 = the map is also stored in the super-row layout, see lili_map_focus; default 1), "fine_grid" (1 = a
 *                 map with more than "fine_occupancy" (default 12) points per gate-sized cell gets a second index with density-sized cells that the
 *                 association searches first — exact; default 1), "scan_lookback" (1 = single-pass decoupled look-back scans; default 1),
 *                 "map_narrow_counts" (1 = byte-wide cell counts while they fit; default 1), "map_guess_box" (1 = a rebuild guesses its bounding box from the
 *                 previous map of the kind and verifies it on the device; default 1; setting it resets the guess state).  All take effect at the next
 *                 lili_map_set;
 *   iteration     "fuse_tail" (1 = reduction + GN update run in the last block of the linearisation launch; default 0 = separate launch, faster on
 *                 MI355X), "merge_kinds" (1 = surf and edge of a keyframe share ONE association and ONE linearisation launch; default 1), "fuse_lin"
 *                 (1 = flavours without count scaling run two launches per iteration below ~100 k queries, the association linearises on the fly;
 *                 default 1; "fuse_lin_block" its workgroup size), "assoc_lpq" (lanes per query in the association of small scans: 0 = by size,
 *                 1 / 2 / 4 / 8 / 16 forces a value), "assoc_prio" (1 = the waves of the association kernels run at issue priority 1 while they search and at
 *                 0 from the fit on; default 1, same bits, 0 for A/B), "count_barrier" (default 0, measured no gain), "persistent_iterate" (1 = scans of <= 128
 *                 cooperative workgroups run a whole registration as ONE persistent launch; default 0, measured slower; poses then differ by the
 *                 partition of the Gram sum, <= 1e-10), "p2p_fusion" (0 = lili_s2m_iterate_sharded runs lili_p2p_allreduce as its own launches;
 *                 default 1);
 *   local map     "localmap_incremental" (default 1, see lili_localmap_commit), "localmap_super_rows" (1 = ring maps below 400 k points get the
 *                 super-row copy too; default 0), "sort_digit_bits" (8, or 4 = the round-2 radix passes), "sort_fused_scan" (1 = radix passes of at most
 *                 "sort_fused_max_tiles" (256) tiles derive their offsets inside the scatter kernel; default 1), "sort_ride_hist" (1 = in the frame pipeline's query filter the
 *                 digit histograms ride on the key kernel and the scatter passes, one launch per pass, for sorts of at most 256 tiles whatever sort_fused_max_tiles says;
 *                 default 1), "voxel_small" (1 = clouds of <= 8192
 *                 points are voxel-filtered / keyframe-sorted by ONE workgroup in LDS; default 1), "voxel_guess_bits" (see lili_voxel_filter_stats; default 1);
 *   host          "readback_gather" (1 = the small reads of a synchronisation are gathered by one kernel writing into page-locked memory instead of
 *                 one copy launch each; default 1), "frame_guess_counts" (1 = lili_frontend_frame_rot with LILI_FRAME_EXTERNAL_MAP and leaf_query 0 enqueues the
 *                 matcher behind the extractor for GUESSED feature counts — the previous scan's plus a margin, padding rows select nothing — and synchronises once;
 *                 a scan with more features than guessed is matched again the plain way; results identical either way; not taken with persistent_iterate; default 1), "frame_extract_stream" (1 = a frame whose
 *                 local map is still to be built runs its extraction on a stream of its own, next to the ring merge instead of in front of it: 15-30 us per frame faster in a
 *                 process with one context, ~100 us SLOWER in a process that holds many streams (they share the runtime's few hardware queues); default 0), "imu_time" (1 = lili_imu_preintegrate brackets its kernel with
 *                 two events for lili_imu_kernel_ms; default 0), "local_graph_time" (1 = the lili_local_graph* calls bracket their kernel with two events for
 *                 lili_local_graph_kernel_ms; default 0).
 *   extraction   "rot_fold" (1 = the ring stage of lili_extract_rot writes the scan's feature lists itself, four launches; 0 = per-ring lists and a concatenation
 *                 launch, also the fallback of a look-back that gave up; default 1), "rot_segment_wait" (1 = a segment whose pick may lie under marks of the
 *                 segment before it waits for them inside the segment stage; 0 = the ring stage repeats such a segment; default 1).
 *   archive / map "archive_max_mb" (bound on the keyframe archive's slab pool in MiB; 0 = unlimited, the default; a push beyond it fails), "archive_slab_mb" (size of
 *                 one slab in MiB, default 64; a keyframe larger than a slab gets a slab of its own), "global_map_batch_points" (points lili_global_map places,
 *                 sorts and folds at a time, 1024 .. 2^27, default 2^21: about 100 bytes of work buffers per point next to the table).
 *   pose graph    "pose_graph_max_loops" (loops the global pose graph accepts, LILI_PG_MAX_LOOPS .. LILI_PG_MAX_LOOPS_EXT, default LILI_PG_MAX_LOOPS; may be
 *                 raised at any time, lowering it below the graph's loop count is LILI_E_STATE; graphs that fit the default solve to the same bits either way).
 * One knob that DOES choose between two definitions of a result: "rot_atan" — lili_extract_rot's atan / atan2 on float arguments
 * (R/src/Preprocessing.cpp:285-288,315,349): 2 (default) = glibc's float routines statement for statement (atanf / atan2f of
 * every glibc up to 2.40 — the bits a build of the reference produces), 1 = the f64 functions rounded to f32 (libm-independent). */
int lili_set_option(lili_ctx* ctx, const char* name, int value);

/* Page-locked host memory for clouds handed over with LILI_MEM_HOST: a cloud in such a buffer is DMA'd straight into HBM (an 80 MB
 * map: ~1.5 ms), a pageable one is staged by the runtime page by page (~8 ms).  Plain hipHostMalloc / hipHostFree — a caller that
 * already owns pinned memory (hipHostRegister on a PCL cloud's buffer) needs neither. */
void* lili_host_alloc(size_t bytes);
void lili_host_free(void* p);

/* ---- local map index ------------------------------------------------------------------------ */

/* Replaces kd_tree_{surf,edge}_local_map->setInputCloud(...) (L/src/BackendFusion.cpp:839-840,
 * L/src/LidarOdometry.cpp:490).  Copies the cloud (if on the host), bins it into a uniform grid whose
 * cell edge covers sqrt(max_sq_radius) so that the 27-cell neighbourhood of a query contains every
 * point the reference's gate `d2[4] < max_sq_radius` can accept — the search is EXACT for all queries
 * the reference keeps.  Blocking.  The points are read where they lie (a device cloud is not copied; it must stay valid until the
 * call returns).  The first build of a kind measures the cloud's bounding box and reads it back before the grid exists; later builds of a cloud
 * of about the same size and gate start from the previous build's box grown by a margin of cells, and check at their final read-back — the one with
 * the density — that no point of THIS cloud lay outside it; if one did, the index is rebuilt with the true box before the call returns and the margin
 * doubles (option "map_guess_box" = 0: always measure first; lili_map_build_stats counts both).  Search results do not depend on where the grid's
 * origin lies. */
int lili_map_set(lili_ctx* ctx, int kind, const lili_cloud* cloud, double max_sq_radius);
/* Diagnostics of the index builds of this context: builds that started from a guessed box, those of them that had to be repeated with the true
 * box, builds repeated with the three-kernel scan because a single-pass scan gave up (never expected).  Any pointer may be NULL. */
int lili_map_build_stats(lili_ctx* ctx, int32_t* box_guesses, int32_t* box_guess_misses, int32_t* scan_fallbacks);
/* The same in two steps for pipelines that rebuild the local map every keyframe (L/src/BackendFusion.cpp:839-840 runs once per keyframe, before
 * the window's iterations): _begin builds the NEXT index of `kind` on a side stream into a second set of buffers — work already enqueued on the
 * context's stream (the previous keyframe's iterations, lili_s2m_iterate*) keeps the current index and overlaps with the build —, _end makes the
 * new index the current one for everything enqueued after it.  _begin waits for the build's small read-backs only (density and box check; the box itself on a first build).
 * The cloud must stay valid until _end.  Results are those of lili_map_set. */
int lili_map_set_begin(lili_ctx* ctx, int kind, const lili_cloud* cloud, double max_sq_radius);
int lili_map_set_end(lili_ctx* ctx, int kind);
/* Number of points / grid cells of the current index (diagnostics). */
int lili_map_info(lili_ctx* ctx, int kind, int64_t* n_points, int64_t* n_cells, double* cell_edge);
/* Density adaptation of the current index (diagnostics): the point-weighted mean number of points per gate-sized cell measured by
 * lili_map_set (0 with option "fine_grid" = 0), and — if the map got the second, density-sized index — its cell edge and the squared
 * radius it covers completely (both 0 otherwise).  Reference call sites: L/src/BackendFusion.cpp:839-840 (setInputCloud on maps
 * down-sampled at L:1488-1511 — leaf sizes down to centimetres make a gate-sized cell hold hundreds of points). */
int lili_map_density(lili_ctx* ctx, int kind, double* mean_occupancy, double* fine_cell_edge, double* fine_sq_radius);

/* The current index itself, for tests that check it cell by cell (read-only, blocking; nothing in the context changes).  `which`: 0 = the gate-sized index,
 * 1 = the fine index of a dense map. */
typedef struct lili_map_index_info {
    int32_t nx, ny, nz;                       /* cells per axis */
    int32_t bx0, by0, bz0, bnx, bny, bnz;     /* the box of cells that has super cells */
    int32_t n_points, reach;
    int32_t has_aux;                          /* the index carries the sorted auxiliary floats */
    int32_t has_super;                        /* the index has the super-row copy */
    int32_t narrow;                           /* built from the 8-bit count table */
    int32_t narrow_overflows, scan_fallbacks; /* the context's counters: builds repeated with 32-bit counters / with the three-kernel scan */
    double ox, oy, oz, inv_cell, cell;        /* origin, 1 / edge, 1 / (1 / edge) as the kernels use them */
    int64_t n_cells;                          /* nx * ny * nz */
    int64_t n_super;                          /* entries of the super-row copy (0 without one) */
} lili_map_index_info;
/* Fills `info` and copies, into every buffer that is not NULL: cell_start (n_cells + 1 words), base (n_points rows of four floats: x, y, z, original index as
 * int bits), aux (n_points floats, if has_aux), cell_start9 (bnx * bny * bnz + 1 words, if has_super), super / super_aux (n_super rows / floats, if has_super /
 * and has_aux).  Capacities count words, rows and floats.  LILI_E_STATE: no map set, an empty map, or no such index; LILI_E_ARG: NULL ctx or info, bad kind or
 * `which`, or a buffer too small for its array — then `info` holds the sizes and NO buffer is written. */
int lili_map_debug_index(lili_ctx* ctx, int kind, int which, lili_map_index_info* info, int32_t* cell_start, size_t cell_start_cap, float* base, size_t base_cap,
                         float* aux, size_t aux_cap, int32_t* cell_start9, size_t cell_start9_cap, float* super, size_t super_cap, float* super_aux, size_t super_aux_cap);

/* Performance hint (no reference counterpart: pcl::KdTreeFLANN indexes the whole cloud it is given, L/src/BackendFusion.cpp:839-840): a local
 * map may cover far more ground than one scan reaches.  lili_map_set stores, next to the cell-sorted points, a "super-row" copy in which the
 * 27-cell neighbourhood of a query is one contiguous run (option "super_rows", 9x the points); with a focus, that copy is built only for the
 * cells within `radius` of `center` (map frame; e.g. the sensor position and its maximum range + the pose uncertainty) at the following
 * lili_map_set calls.  Queries elsewhere take the nine-row walk over the base index: results never depend on the hint.  radius <= 0 or
 * center == NULL: the whole map again. */
int lili_map_focus(lili_ctx* ctx, const double center[3], double radius);

/* ---- feature extraction ----------------------------------------------------------------------- */

/* Caller-owned output cloud: `capacity` points of `stride` bytes (>= 16; 32 for pcl::PointXYZI, whose x,y,z
 * are floats at 0/4/8 — the 4th float written at offset 12 is the intensity, copy it to offset 16 for PCL or
 * pass stride 16 and repack); `count` receives the number of points available (may exceed capacity); entries of the buffer behind
 * `count` are unspecified (an extractor may have written there). */
typedef struct lili_feature_out {
    void* data;
    size_t capacity;
    size_t stride;
    int mem;          /* LILI_MEM_HOST or LILI_MEM_DEVICE */
    size_t count;     /* out */
} lili_feature_out;

typedef struct lili_rot_params {
    int n_scans;       /* 16 / 32 / 64  (R/src/Preprocessing.cpp:46, config line_num) */
    int ds_rate;       /* R/config/config_fr_iosb.yaml:13 */
    float ds_v;        /* 0.6, R/src/Preprocessing.cpp:14 */
    float near_range;  /* 3.0, R/src/Preprocessing.cpp:281 */
} lili_rot_params;

/* Replaces the body of Preprocessing::cloudHandler of LiLi-OM-ROT (R/src/Preprocessing.cpp:277-527) for one
 * scan: NaN / near-range filter, ring id + relative time, IMU deskew (q_imu = the integrated gyro quaternion of
 * R:179-223, computed by the caller; q_lb the extrinsic), ring concatenation, 11-tap curvature, per-segment
 * sharp / less-sharp / flat selection, per-ring VoxelGrid of the less-flat points.
 *   scan  : raw points in firing order, aux_offset = byte offset of the intensity field;
 *   full  : the ring-concatenated, deskewed cloud          (/lidar_cloud_cutted)
 *   edge  : cornerPointsLessSharp, in push order            (/edge_features)
 *   surf  : voxel-filtered less-flat points, ring by ring   (/surf_features)
 * Points are written as (x, y, z, intensity = ring + 0.1 * relTime).  Blocking.  A LILI_MEM_DEVICE scan of 16-byte rows (x, y, z, intensity)
 * is read in place; a scan in PAGE-LOCKED host memory (lili_host_alloc) is read by the first kernel where it lies instead of being uploaded first; a
 * `full` buffer in page-locked host memory receives min(scan->n, capacity) records while the features are selected — the records behind full->count
 * are unspecified —, `edge` / `surf` buffers in page-locked memory (16-byte aligned, stride a multiple of 16) are written by a kernel behind the
 * selection, `count` records each (only the first 16 bytes of a row), and the call synchronises once; pageable buffers are served by copies after the
 * counts have arrived. */
int lili_extract_rot(lili_ctx* ctx, const lili_cloud* scan, const double q_imu[4], const double q_lb[4], const lili_rot_params* params,
                     lili_feature_out* full, lili_feature_out* edge, lili_feature_out* surf);
/* Intermediate products of the last lili_extract_rot for parity tests (any pointer may be NULL):
 * counts = {n_full, n_edge, n_sharp, n_flat, n_lessflat, n_surf, halfPassed index, first valid index};
 * ring_start/ring_end: 64 ints (scanStartInd / scanEndInd); per-point arrays are n_full long; index lists point
 * into the full cloud. */
int lili_extract_rot_debug(lili_ctx* ctx, int32_t counts[8], int32_t* ring_start, int32_t* ring_end, int32_t* full_src, float* curvature,
                           int32_t* label, int32_t* edge_idx, int32_t* sharp_idx, int32_t* flat_idx, int32_t* lessflat_idx, int32_t* surf_cnt);

typedef struct lili_livox_params {
    double surf_thres;   /* L/config/config_fr_iosb.yaml:5 (0.28) */
    double edge_thres;   /* L/config/config_fr_iosb.yaml:6 (4)    */
    float near_range;    /* 0.1, L/src/Preprocessing.cpp:226      */
} lili_livox_params;

/* Replaces the body of Preprocessing::cloudHandler of LiLi-OM (L/src/Preprocessing.cpp:219-401) for one Livox
 * Horizon scan in FormatConvert's layout (L/src/FormatConvert.cpp:14-23): scan->aux_offset = byte offset of
 * `intensity` (line + 0.1 * t), curvature_offset = byte offset of `curvature` (0.1 * reflectivity) — 32 and 36 for
 * pcl::PointXYZINormal.  q_imu = the gyro quaternion integrated over the scan (L:129-171, caller side).
 * Outputs are records of 32 B (x,y,z,nx,ny,nz,intensity,curvature; stride 32) or pcl::PointXYZINormal (stride 48):
 *   cutted: every deskewed point with a valid line (/lidar_cloud_cutted), edge: /edge_features (normal = line
 *   direction), surf: /surf_features (normal = plane normal).  Blocking.  A valid line is int(intensity) in 0 .. 5: a negative line is skipped as in the
 *   reference, a line >= 6 (the reference would write outside its grid) and a non-finite intensity (NaN, +-inf: the reference's x86 build converts them to
 *   INT_MIN and skips the point) are dropped before lidar_cloud_cutted as well.  The rows are read as they are (one transfer for host memory);
 *   a `cutted` buffer in host memory receives min(scan->n, capacity) records while the features are selected — the records behind
 *   cutted->count are unspecified.  `edge` and `surf` buffers in PAGE-LOCKED host memory (lili_host_alloc, 16-byte aligned) are written by the
 *   packing kernel itself, `count` records each, and the call synchronises once; pageable buffers are served by copies after the counts have arrived. */
int lili_extract_livox(lili_ctx* ctx, const lili_cloud* scan, int curvature_offset, const double q_imu[4], const lili_livox_params* params,
                       lili_feature_out* cutted, lili_feature_out* edge, lili_feature_out* surf);
/* counts = {n_cutted, n_edge, n_surf}; cut_src[n_cutted]; cell_src[24000] (input index owning each grid cell or -1);
 * edge_cell / surf_cell: cell (line * 4000 + column) of each emitted feature.  Any pointer may be NULL. */
int lili_extract_livox_debug(lili_ctx* ctx, int32_t counts[3], int32_t* cut_src, int32_t* cell_src, int32_t* edge_cell, int32_t* surf_cell);

/* Device views (float4 x,y,z,aux; LILI_MEM_DEVICE clouds, valid until the next extract call on the context) of the last
 * extraction, so that features go from the extractor to lili_voxel_filter / lili_s2m_set_queries / lili_localmap_push
 * without leaving HBM.  ROT: aux = intensity (ring + 0.1 relTime); Livox: aux = curvature (0.1 * reflectivity). */
int lili_extract_rot_device(lili_ctx* ctx, lili_cloud* full, lili_cloud* edge, lili_cloud* surf);
int lili_extract_livox_device(lili_ctx* ctx, lili_cloud* edge, lili_cloud* surf);

/* ---- local map: keyframe ring buffer + VoxelGrid + index ------------------------------------ */

/* pcl::VoxelGrid<PointT>::filter with leaf (leaf, leaf, leaf) on (x, y, z, aux) points: one centroid per occupied
 * voxel (aux averaged too), output ordered by ascending voxel index, f32 accumulation in input order
 * (L/src/BackendFusion.cpp:1488-1511, R/src/Preprocessing.cpp:502-506).  `counts` (optional, capacity ints) receives
 * the number of points merged into each output point.  Blocking. */
int lili_voxel_filter(lili_ctx* ctx, const lili_cloud* cloud, float leaf, lili_feature_out* out, int32_t* counts);
/* Keyframe ring buffer of one map kind (recent_surf_keyframes / recent_edge_keyframes, L:1407-1477):
 * push = transformCloud(features, pose) appended, oldest dropped beyond `width` (local_map_width);
 * commit = concatenate (L:1479-1483) + VoxelGrid(leaf) (L:1488-1492) + lili_map_set on the result (L:839-840),
 * all on the device.  n_raw / n_map (optional) receive the point counts before / after the filter. */
int lili_localmap_reset(lili_ctx* ctx, int kind);
int lili_localmap_push(lili_ctx* ctx, int kind, const lili_cloud* features, const double t[3], const double q[4], int width);
int lili_localmap_commit(lili_ctx* ctx, int kind, float leaf, double max_sq_radius, int64_t* n_raw, int64_t* n_map);
/* The ring's keyframes (oldest first, n = ring size of every kind in kind_mask) take new map-frame poses (t: 3n, q: 4n, wxyz) —
 * buildLocalMapWithLandMark's warm-up branch (L/src/BackendFusion.cpp:1407-1443): transformCloud is re-run from the LiDAR-frame points the
 * ring keeps.  Asynchronous; the next lili_localmap_commit / lili_backend_keyframe_prepare builds the map from the new poses.  Only keyframes
 * whose pose is not bit-equal to the stored one (or was read on the device: lili_frontend_frame) are re-transformed; a repose that changes
 * nothing enqueues nothing.  After a change confined to the newest keyframes (at most 8 from the oldest changed one to the end, pending pushes
 * included) the next commit is one merge step on the sorted ring (counted as incremental); otherwise it rebuilds.  The map is the same bit for
 * bit as after lili_localmap_reset and pushes at the new poses.  LILI_E_ARG (ring untouched): empty or unknown mask, null pointer, n differing
 * from the size of a ring in the mask. */
int lili_localmap_repose(lili_ctx* ctx, int kind_mask, int n, const double* t, const double* q);
/* How the commits of this context were served: steps on the ring kept sorted by voxel (one keyframe popped / pushed since the last commit, the
 * reference's steady state, L/src/BackendFusion.cpp:1407-1477, or a re-posed suffix merged back, lili_localmap_repose) against full rebuilds (first commit, several keyframes pending, another leaf).
 * The map is the same bit for bit either way (option "localmap_incremental" = 0 forces rebuilds). */
int lili_localmap_stats(lili_ctx* ctx, int32_t* incremental_commits, int32_t* full_commits);
/* How the VoxelGrid filters of more than 8192 points (lili_voxel_filter, lili_localmap_commit's rebuild, lili_frontend_frame's query filter) were served: a filter
 * whose leaf size has been seen before keeps its bounding box on the device and sorts by as many key bits as the previous one needed ("voxel_guess_bits", default 1);
 * the device checks the guess, a filter it does not hold for is repeated with the box measured (key_guess_misses).  The output never depends on it. */
int lili_voxel_filter_stats(lili_ctx* ctx, int32_t* key_guesses, int32_t* key_guess_misses);
/* The down-sampled local map of the last lili_localmap_commit as (x, y, z, aux) rows in map order (out->count = its size; at most
 * out->capacity rows are copied).  Blocking. */
int lili_localmap_get(lili_ctx* ctx, lili_feature_out* out);

/* ---- front-end frame: the whole per-scan chain of the odometry node in ONE call ------------------ */

/* Replaces the body of LidarOdometry::run for one Livox scan (L/src/LidarOdometry.cpp:652-707) together with the extraction node in front of
 * it (L/src/Preprocessing.cpp:219-401): extraction -> down_size_filter_surf (L:155, 320-322) -> scan-to-map iterations against the local map
 * of the last `width` frames (buildLocalMap L:280-303, downSampleCloud L:314-318, kd_tree_surf_last->setInputCloud L:490,
 * findCorrespondingSurfFeatures + LidarPlaneNormIncreFactor + HuberLoss L:352-413, 483-561) -> the frame joins the ring at the pose found
 * (transformCloud, L:292-297); the local map that includes it (concatenate + VoxelGrid + index) is built at the start of the next call, under that frame's extraction.
 * Everything between the scan and the returned pose stays in HBM: features, down-sampled queries, ring, map and pose never visit the host;
 * the host synchronises three times per frame, for the counts that size the next launches (ring merge; index build + query filter, whose launches are enqueued
 * behind the build's so that both outcomes come back together) and for the result.
 *   scan / curvature_offset / q_imu / livox : as lili_extract_livox
 *   match   : matcher parameters (LILI_VARIANT_FRONTEND for the reference's front end)
 *   t_pred, q_pred : poseInitialization's guess (L:415-441: constant-velocity extrapolation, caller side); a frame that is not matched
 *                    (n_iters = 0, or a map of fewer than 10 points, L:485-488) keeps it.
 * `res` receives the pose, the solver status of the last update and the sizes; res->stage_us (opt->want_timing) the host-side time stamps
 * of the stages in microseconds since the call began ([0] pending local map built and query filter enqueued, [1] queries known, [2] iterations enqueued,
 * [3] pose known).  lili_frontend_reset empties the ring (a new sequence). */
typedef struct lili_frontend_options {
    float leaf_query;   /* down_size_filter_surf: 0.4 (L/src/LidarOdometry.cpp:155) */
    float leaf_map;     /* down_size_filter_surf_map: 0.4 (L:156) */
    int width;          /* frames in the local map: 20 (L:290) */
    int n_iters;        /* outer iterations (association + Gauss-Newton update) per frame */
    int slot;           /* matcher slot used for the frame's queries and pose */
    int want_timing;
    int flags;          /* LILI_FRAME_* */
} lili_frontend_options;
/* The reference node's start-up (L/src/LidarOdometry.cpp:659-663, 283-289, 501-504), expressed per call so that the caller's frame counter decides:
 *   frame 0 (system not initialised: savePoses + checkInitialization only): n_iters = 0 and LILI_FRAME_PUSH_EMPTY — the pose is the given one and the ring
 *            receives an EMPTY keyframe (surf_frames[0] is the not-yet-filled surf_last_ds);
 *   frame 1 (pose_cloud_frame holds one pose): LILI_FRAME_SELF_MAP — the local map is the frame's own surf features (L:286-289), n_iters = 8 (L:501-502);
 *   later frames: flags = 0, n_iters = scan_match_cnt. */
enum { LILI_FRAME_SELF_MAP = 1, LILI_FRAME_PUSH_EMPTY = 2,
       /* round 6 — the frame call for a caller that keeps its own maps (the BACK end's matcher on one scan: BASELINE configs[0]):
        *   LILI_FRAME_EXTERNAL_MAP  match against the index(es) the caller set with lili_map_set; nothing joins the ring, no local map is built;
        *   LILI_FRAME_EDGES         (with EXTERNAL_MAP) the edge features are queries too (kind mask surf | edge, findCorrespondingCornerFeatures);
        *   leaf_query = 0           (with EXTERNAL_MAP) the surf features themselves are the queries (no down_size_filter_surf). */
       LILI_FRAME_EXTERNAL_MAP = 4, LILI_FRAME_EDGES = 8 };
typedef struct lili_frontend_result {
    double t[3], q[4];
    int gn_status;      /* of the last update; 0 when the frame was not matched */
    int matched;        /* 0: first frame of a sequence, or a map of fewer than 10 points (L:485-488): pose = prediction */
    int32_t n_edge, n_surf, n_query, n_map_raw, n_map;   /* features, down-sampled queries; ring points and map points of the map the frame was MATCHED AGAINST (whichever call built it;
                                                          * a LILI_FRAME_SELF_MAP frame: its own features and their filtered cloud; LILI_FRAME_EXTERNAL_MAP: the caller's map, twice) */
    double stage_us[8];
} lili_frontend_result;
int lili_frontend_frame(lili_ctx* ctx, const lili_cloud* scan, int curvature_offset, const double q_imu[4], const lili_livox_params* livox,
                        const lili_s2m_params* match, const lili_frontend_options* opt, const double t_pred[3], const double q_pred[4],
                        lili_frontend_result* res);
/* The same chain behind the LOAM-style extractor of the LiLi-OM-ROT package (scan / q_imu / q_lb / rot: as lili_extract_rot; R/src/Preprocessing.cpp:248-535 in front of
 * R/src/LidarOdometry.cpp:638-693 — that node is the Livox package's but for the point type).  One call per spinning-LiDAR scan. */
int lili_frontend_frame_rot(lili_ctx* ctx, const lili_cloud* scan, const double q_imu[4], const double q_lb[4], const lili_rot_params* rot,
                            const lili_s2m_params* match, const lili_frontend_options* opt, const double t_pred[3], const double q_pred[4],
                            lili_frontend_result* res);
int lili_frontend_reset(lili_ctx* ctx);
/* lili_frontend_frame leaves the local map WITH the frame it has just pushed to the next call, which builds it under its own extraction (res->n_map_raw / n_map
 * describe the map the frame was matched against).  lili_frontend_flush builds it now — for a caller that reads the map between frames (lili_localmap_get,
 * lili_map_info) or ends a sequence.  Blocking; n_map_raw / n_map optional. */
int lili_frontend_flush(lili_ctx* ctx, const lili_s2m_params* match, const lili_frontend_options* opt, int32_t* n_map_raw, int32_t* n_map);

/* ---- keyframe hand-over: what LidarOdometry::run does once it has a pose (L/src/LidarOdometry.cpp:565-586, 624-650, 675-680; the same text in R/) ---------------- */

/* The keyframe decision of the odometry node (L:565-585 with the counters of L:325-331, 675-676), host code without a context.  One lili_kf_rule_step per frame, in order, with the
 * pose the frame ended at (t, q = abs_pose) and whether it was matched (lili_frontend_result.matched; a frame that was not — the early return of L:485-488 — keeps the flag of
 * the frame before it).  Returns LILI_KF_NO (0), LILI_KF_YES (1: publish /odom and the three clouds, deskewed when if_to_deskew is set) or, for the FIRST call after a reset,
 * LILI_KF_FIRST (2: checkInitialization, L:201-219 — the clouds go out as they are, never deskewed, and no /odom; `matched` and the pose are not looked at, the flag stays
 * set as `bool kf = true` leaves it).  The condition is the reference's with its precedence, ((dis > 0.2 || ang > 0.1) && n - kf_num > 1 || n - kf_num > 2) || n <= 1, n =
 * pose_cloud_frame->points.size() BEFORE this frame's savePoses and kf_num = that size AFTER the savePoses of the last keyframe; ang = 2 acos(w) of quat_last_kF^-1 * q is
 * NaN for w > 1 and then compares false. */
enum { LILI_KF_NO = 0, LILI_KF_YES = 1, LILI_KF_FIRST = 2 };
typedef struct lili_kf_rule_state {
    double t_last[3], q_last[4];   /* trans_last_kf, quat_last_kF (w, x, y, z) */
    int64_t n_frames;              /* pose_cloud_frame->points.size() */
    int64_t kf_num;
    int32_t kf;                    /* the node's flag */
    int32_t reserved_;
} lili_kf_rule_state;
void lili_kf_rule_reset(lili_kf_rule_state* st);
int lili_kf_rule_step(lili_kf_rule_state* st, const double t[3], const double q[4], int matched);
/* computeRelative (L:444-480) in Eigen's order of operations: q_rel = q_prev^-1 * q_cur, t_rel = q_prev^-1 * (t_cur - t_prev), inverse = conjugate / squared norm.
 * Host code, no context.  LILI_E_ARG for a null pointer. */
int lili_pose_relative(const double t_prev[3], const double q_prev[4], const double t_cur[3], const double q_cur[4], double t_rel[3], double q_rel[4]);

/* undistortion(cloud, trans, quat) of the odometry node (L:178-199) for up to three clouds in ONE launch.  Per point, with I the float at byte `time_offset[k]` of the row
 * (intensity = line or ring + time within the scan: 32 in pcl::PointXYZINormal, 16 in pcl::PointXYZI, 12 in the library's float4 rows of the ROT extractor):
 *     line = (int) I;  ratio = (double)(I - (float) line) / 0.1, at most 1 (no lower bound);  p' = Identity.slerp(ratio, q_rel) * p + ratio * t_rel   in f64, stored as f32.
 * q_rel NULL or exactly (1, 0, 0, 0) — what publishCloudLast passes — : p' = p + ratio * t_rel, the reference's bits.  Any other q_rel: Eigen 3.3's slerp and q * v.
 * (int) converts as the reference's x86 build does (NaN and values beyond int: INT_MIN).  A NaN or -inf time channel gives NaN coordinates (+inf clamps to ratio 1); a row with a non-finite coordinate
 * gives three NaN (Eigen's cross product with it).
 *   clouds[k]     : NULL or n = 0: nothing for k.  Host (pageable: one staged copy; page-locked: read where it lies) or device memory, any stride that is a multiple of 4;
 *                   aux_offset = the float that becomes the 4th of the output row (-1: 0) — need not be the time channel (Livox: curvature at 36);
 *   out[k]        : caller-owned DEVICE buffer of float4 rows (x', y', z', aux): stride 16, mem LILI_MEM_DEVICE, capacity >= clouds[k]->n; count receives n.  The layout
 *                   lili_voxel_filter, lili_backend_keyframe_prepare and lili_archive_push take.  out[k].data may be clouds[k]->data when that is a device cloud of stride 16.
 * LILI_E_ARG before anything is enqueued: a stride or offset that is no multiple of 4 or reaches beyond the row, a negative time_offset, capacity too small.
 * Asynchronous (a pageable host cloud is consumed before the call returns). */
int lili_keyframe_undistort(lili_ctx* ctx, const lili_cloud* const clouds[3], const int time_offset[3], const double t_rel[3], const double q_rel[4],
                            lili_feature_out out[3]);

/* publishCloudLast (L:624-650) for the scan of the last lili_frontend_frame / lili_frontend_frame_rot / lili_extract_* on this context (flavour LILI_VARIANT_LIVOX or
 * LILI_VARIANT_ROT; LILI_E_STATE when there is none): the three clouds the back end receives — /laser_cloud_corner_last, /laser_cloud_surf_last, /full_point_cloud — taken from
 * the extractor's own device lists (the edge list included, which a Livox frame call does not convert; the true counts after a frame matched with guessed ones) and moved by
 * undistortion(cloud, t_rel, q_rel) in one launch when `deskew` is set; deskew = 0 (if_to_deskew off, or LILI_KF_FIRST) gives the clouds as they are.  edge / surf / full
 * receive LILI_MEM_DEVICE clouds of float4 rows (any may be NULL); the 4th float is what lili_extract_*_device carries for edge and surf (Livox: curvature, ROT: intensity) and the
 * intensity for full.  The views are the library's and stay valid until the next extraction or lili_frontend_keyframe on the context.  Asynchronous.
 * lili_frontend_keyframe_get copies one of them out (kind 0 = edge, 1 = surf, 2 = full; out->count = its size, at most capacity rows of 16 bytes are written, stride >= 16;
 * host or device memory).  Blocking. */
int lili_frontend_keyframe(lili_ctx* ctx, int flavour, const double t_rel[3], const double q_rel[4], int deskew, lili_cloud* edge, lili_cloud* surf, lili_cloud* full);
int lili_frontend_keyframe_get(lili_ctx* ctx, int kind, lili_feature_out* out);

/* ---- back-end keyframe: everything between "a keyframe has arrived" and ceres::Solve in ONE call ---------------- */

/* Replaces, for one keyframe of the reference's back end (L/src/BackendFusion.cpp:830-980):
 *   buildLocalMapWithLandMark (L:1387-1484, steady state :1444-1476) — the keyframe whose pose the previous solve fixed (`join_*`, its LiDAR pose in the map frame
 *       t_join / q_join = q_po * q_bl, q_po * t_bl + t_po; NULL: nothing joins, e.g. the first call) is transformed and appended to both rings, the oldest leaves
 *       beyond opt->width (warm-up, the rings shorter than opt->width, L:1407-1443: lili_localmap_repose of both rings at the solve's poses comes first);
 *   downSampleCloud (L:1486-1519) — both rings -> VoxelGrid(leaf_*_map) -> kd_tree_*_local_map->setInputCloud (L:839-840); the NEW keyframe's features
 *       (`new_surf`, `new_edge`, LiDAR frame) -> VoxelGrid(leaf_surf / leaf_edge) = surf_lasts_ds / edge_lasts_ds -> the queries of slots[n_slots - 1];
 *   findCorrespondingCornerFeatures / findCorrespondingSurfFeatures (L:919-936) — every keyframe of the window (slots[i], oldest first; the older slots keep the
 *       queries earlier calls gave them) at its association pose (t_assoc 3, q_assoc 4 values per slot: q * q_lb^-1, t - Q2 t_lb, L:929-930).
 * Rings, maps, indices, queries and correspondence records stay in HBM; afterwards the window is ready for lili_s2m_linearize_window (LidarWindowFactor),
 * lili_s2m_solve_lm_window or lili_marg_add_lidar.  n_res (optional): 2 per slot {surf, edge}.  Records and counts equal the calls one by one
 * (lili_localmap_push x 2, lili_localmap_commit x 2, lili_voxel_filter x 2, lili_s2m_set_queries x 2, lili_s2m_associate_window) bit for bit. */
typedef struct lili_backend_options {
    float leaf_surf, leaf_edge;           /* ds_filter_surf / ds_filter_edge: surf_ds 0.4, edge_ds 0.2 (L/config/config_fr_iosb.yaml:22-23) */
    float leaf_surf_map, leaf_edge_map;   /* ds_filter_surf_map / ds_filter_edge_map: the same values in the reference (L:491-494) */
    int width;                            /* local_map_width: 40 (L/config :16) */
    int want_timing;
    int join_slot;                        /* >= 0 (and join_surf = join_edge = NULL): the joining keyframe's features are the QUERIES of that matcher slot — the reference stores
                                           * surf_lasts_ds / edge_lasts_ds of a keyframe as its surf_frames / edge_frames entry (L:1505-1519, saveKeyFramesAndFactors), i.e. what an
                                           * earlier call left in the slot that was then the newest: the keyframe never leaves HBM.  < 0: not used */
} lili_backend_options;
typedef struct lili_backend_result {
    int32_t n_map_raw[2], n_map[2];       /* ring points and map points per kind {surf, edge} */
    int32_t n_query[2];                   /* the new keyframe's down-sampled features per kind */
    int32_t associated;                   /* 0: a map was missing (first keyframes), nothing associated */
    double stage_us[8];                   /* opt->want_timing: host time since the call began after [0] the surf side, [1] the edge side, [2] the associations */
} lili_backend_result;
int lili_backend_keyframe_prepare(lili_ctx* ctx, const lili_cloud* join_surf, const lili_cloud* join_edge, const double t_join[3], const double q_join[4],
                                  const lili_cloud* new_surf, const lili_cloud* new_edge, const int* slots, int n_slots, const double* t_assoc, const double* q_assoc,
                                  const lili_s2m_params* match, const lili_backend_options* opt, int32_t* n_res, lili_backend_result* res);

/* ---- scan-to-map matcher -------------------------------------------------------------------- */

/* Uploads the feature points of keyframe `slot` (surf_lasts_ds[idx] / edge_lasts_ds[idx],
 * L/src/BackendFusion.cpp:1536,1606).  Async when the cloud is already on the device. */
int lili_s2m_set_queries(lili_ctx* ctx, int slot, int kind, const lili_cloud* cloud);

/* Replaces findCorresponding{Surf,Corner}Features(idx, q, t) (L/src/BackendFusion.cpp:1531-1681,
 * R/src/BackendFusion.cpp:1394-1520, L/src/LidarOdometry.cpp:352-413): transform with (q_assoc,
 * t_assoc), exact 5-NN, line / plane fit, gates, weights.  Correspondence records stay on the device.
 * n_res (optional) receives the number of correspondences — passing it makes the call blocking. */
int lili_s2m_associate(lili_ctx* ctx, int slot, int kind, const double t_assoc[3], const double q_assoc[4],
                       const lili_s2m_params* params, int* n_res);
/* The same for the keyframes of the sliding window in one call (L/src/BackendFusion.cpp:919-936 calls both finders per keyframe): t_assoc = 3,
 * q_assoc = 4 values per slot; n_res (optional) = 2 per slot, {surf, edge} (0 for a kind outside kind_mask).  Both kinds of a slot share a launch,
 * the slots run concurrently, and with n_res the call synchronises once.  Records equal lili_s2m_associate per slot and kind. */
int lili_s2m_associate_window(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const double* t_assoc, const double* q_assoc,
                              const lili_s2m_params* params, int* n_res);

/* Replaces N x (AutoDiffCostFunction::Evaluate + loss corrector) and the J^T J / J^T r accumulation
 * (L/include/factors/LidarKeyframeFactor.h:12-139, L/src/MarginalizationFactor.cpp:3-29,44-70) for the
 * records of `slot` selected by `kind_mask`, at the body pose (t, q).
 *   gram[64] : row-major 8x8, sum over residuals of [J r]^T [J r] after robustification, with J the
 *              1x7 GLOBAL Jacobian ordered (t0,t1,t2,qw,qx,qy,qz) and r the residual;
 *   cost     : sum of 1/2 rho(r^2);  counts[0] = surf residuals, counts[1] = edge residuals.
 * Blocking. */
int lili_s2m_linearize(lili_ctx* ctx, int slot, int kind_mask, const double t[3], const double q[4],
                       const lili_s2m_params* params, double gram[64], double* cost, int counts[2]);
/* The same for several slots at once — ONE evaluation of the joint sliding window (a Gram per keyframe; ceres::Solve evaluates the window up to 15
 * times per keyframe, L/src/BackendFusion.cpp:919-992): t = 3, q = 4, gram = 64, cost = 1 (optional), counts = 2 (optional) values per slot, in the
 * order of `slots`.  The slots run concurrently and the call synchronises once; results equal lili_s2m_linearize per slot bit for bit.  Blocking. */
int lili_s2m_linearize_window(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const double* t, const double* q,
                              const lili_s2m_params* params, double* gram, double* cost, int* counts);

/* Copy-out of the ordered correspondence lists (the vec_surf_cur_pts / vec_surf_normal /
 * vec_surf_scores and vec_edge_cur_pts / vec_edge_match_j / vec_edge_match_l of the reference).
 * Arrays may be NULL; capacity in records; *n_out = number of records available.  Blocking. */
int lili_s2m_get_surf_records(lili_ctx* ctx, int slot, size_t capacity, int32_t* query_index, float* cur_pt /*3*/,
                              float* normal /*3, weight-scaled*/, float* neg_oa_dot_norm, double* score, size_t* n_out);
int lili_s2m_get_edge_records(lili_ctx* ctx, int slot, size_t capacity, int32_t* query_index, float* cur_pt /*3*/,
                              float* pt_a /*3*/, float* pt_b /*3*/, float* s, size_t* n_out);
/* Per-query neighbour lists of the last associate (requires lili_set_debug(ctx, 1)): idx/d2 are n_q x 5. */
int lili_s2m_get_neighbors(lili_ctx* ctx, int slot, int kind, size_t n_q, int32_t* idx, float* d2);

/* ---- device-resident outer iterations (no host round trip) ----------------------------------- */

/* Body pose of `slot` kept in device memory. */
int lili_s2m_pose_set(lili_ctx* ctx, int slot, const double t[3], const double q[4]);
int lili_s2m_pose_get(lili_ctx* ctx, int slot, double t[3], double q[4], int* gn_status /*0 ok, 1 singular*/);

/* The last Gauss-Newton step of `slot`: delta[6] = (dt[3], rotation vector[3]) of the local parameterisation, the number of updates since
 * lili_s2m_pose_set and the status of the last one (0 ok, 1 = normal matrix not positive definite: pose left unchanged, 2 = a multi-GPU
 * exchange gave up).  The device loops take plain Gauss-Newton steps (one per re-association, like one accepted step of the reference's
 * ceres::Solve, L/src/BackendFusion.cpp:984-992); callers that need Ceres' step acceptance drive lili_s2m_linearize from their own solver
 * (include/lili_ceres_adapter.h) — this call lets the others at least see how far a step went.  Blocking. */
int lili_s2m_last_step(lili_ctx* ctx, int slot, double delta[6], int* n_updates, int* gn_status);

/* ---- Levenberg-Marquardt on the device (fixed correspondences) -------------------------------------
 * The reference's inner loop: ceres::Solve on the residual blocks of the last association (L/src/BackendFusion.cpp:984-992: DENSE_QR,
 * max_num_iterations = max_num_iter, otherwise Ceres 2.0 defaults — TRUST_REGION / LEVENBERG_MARQUARDT, initial radius 1e4, Jacobi scaling,
 * monotonic steps, function / gradient / parameter tolerances 1e-6 / 1e-10 / 1e-8).  lili_s2m_solve_lm runs that loop for
 * the lidar blocks of ONE slot — both kinds in kind_mask, robustified by params->loss — as ONE persistent launch: every iteration evaluates
 * all records at the candidate pose (robust cost + Gram), the workgroups exchange their partials inside the launch and each takes the same
 * accept / reject decision; the pose of the slot ends at the last accepted point — a candidate that triggers the parameter or the function
 * tolerance is NOT taken (Ceres returns before HandleSuccessfulStep).  Decisions and final pose equal the oracle's restatement
 * of Ceres' loop on per-residual rows (oracle/lo_window.py::ceres_lm; tests/test_lm_gpu.py).  Needs lili_s2m_associate* first.
 * options == NULL: the defaults above with max_iterations = 15.  summary (host memory, optional): filled after a synchronisation of the
 * context's stream; with summary == NULL the call is asynchronous.  Not to be overlapped with other persistent launches of the same
 * device beyond what lili_s2m_solve_lm_window does itself (every workgroup of the launch has to be resident; waits are bounded and end in
 * LILI_LM_STALLED rather than a hang). */
#define LILI_LM_MAX_LOG 32
enum { LILI_LM_MAX_ITERATIONS = 0, LILI_LM_GRADIENT_TOLERANCE = 1, LILI_LM_PARAMETER_TOLERANCE = 2, LILI_LM_FUNCTION_TOLERANCE = 3,
       LILI_LM_STALLED = 4, LILI_LM_NUMERICAL_FAILURE = 5 /* a non-positive pivot, or 5 consecutive invalid steps (Ceres: FAILURE) */,
       LILI_LM_MIN_RADIUS = 6 /* trust-region radius <= min_radius (Ceres: CONVERGENCE, "minimum trust region radius reached") */ };
typedef struct lili_lm_options {
    int32_t max_iterations;
    int32_t reserved_;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
} lili_lm_options;
typedef struct lili_lm_iteration {       /* one evaluated candidate */
    double cost, new_cost, rho, radius, step_norm;
    int32_t accepted, iteration;
} lili_lm_iteration;
typedef struct lili_lm_summary {
    int32_t iterations, successful_steps, termination, n_logged;
    int32_t n_surf, n_edge;              /* correspondences the rows were scaled with (ROT: num / N) */
    double initial_cost, final_cost, final_radius;
    lili_lm_iteration it[LILI_LM_MAX_LOG];
} lili_lm_summary;
void lili_lm_default_options(lili_lm_options* opt);
int lili_s2m_solve_lm(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, const lili_lm_options* options,
                      lili_lm_summary* summary);
/* The same for several slots (the keyframes of the sliding window) concurrently, one launch per slot on forked streams; summaries:
 * n_slots entries (optional).  The joint window of the reference couples the keyframes through the IMU factors: that problem is
 * lili_window_solve below (or the caller's solver around include/lili_ceres_adapter.h); this call is for per-keyframe refinements and
 * for the front-end. */
int lili_s2m_solve_lm_window(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params,
                             const lili_lm_options* options, lili_lm_summary* summaries);

/* One outer iteration, first half (async): re-associate at the device pose (association transform
 * Q2 = Q*q_lb^-1, T2 = T - Q2*t_lb as in L/src/BackendFusion.cpp:929-930), linearise, and reduce this
 * rank's partial into d_gram (DEVICE pointer to LILI_GRAM_DOUBLES doubles owned by the caller:
 * [0..63] Gram, [64] cost, [65] n_surf, [66] n_edge).  Between the two halves a multi-GPU caller
 * all-reduces d_gram (sum) over ranks on the same stream. */
int lili_s2m_accumulate(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, double* d_gram);
/* The same in two steps, for callers that shard the queries of one scan over several GPUs AND use the
 * ROT residual scaling num / N (R/src/BackendFusion.cpp:843,861), where N must be the GLOBAL count:
 *   lili_s2m_associate_dev   -> per-block counts of this rank in device memory
 *   lili_s2m_counts_export   -> this rank's {n_surf, n_edge} into a caller-owned DEVICE int32[2]   (async)
 *   [caller: all-reduce(sum) that buffer over ranks on the same stream]
 *   lili_s2m_counts_import   -> the next linearize_dev scales with that buffer (read by its kernels, no copy:
 *                               keep it valid and unchanged until that call's work has run)            (async)
 *   lili_s2m_linearize_dev   -> d_gram as above.                                                          */
int lili_s2m_associate_dev(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params);
int lili_s2m_counts_export(lili_ctx* ctx, int slot, int32_t* d_counts);
int lili_s2m_counts_import(lili_ctx* ctx, int slot, const int32_t* d_counts);
int lili_s2m_linearize_dev(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, double* d_gram);
/* Second half (async): one Gauss-Newton step on the 6-dof local parameterisation
 * (ceres::QuaternionParameterization plus-Jacobian and Plus()), pose updated in device memory. */
int lili_s2m_gn_update(lili_ctx* ctx, int slot, const double* d_gram);

/* The sharded iteration loop in ONE host call (queries block-sharded over the GPUs of a node, map replicated):
 * n_iters x [ associate_dev -> (count-scaled flavours only: counts_export -> all-reduce(int32[2]) -> counts_import) ->
 *             linearize_dev(d_gram) -> all-reduce(f64[LILI_GRAM_DOUBLES]) -> gn_update ]
 * everything enqueued on the context's stream, so that no host code sits between the kernels and the two collectives.
 * `allreduce` has the signature of ncclAllReduce (RCCL: sendbuff, recvbuff, count, ncclDataType_t, ncclRedOp_t, ncclComm_t,
 * hipStream_t) and is called in place with datatype 2 (ncclInt32) / 8 (ncclFloat64) and op 0 (ncclSum); the library does not
 * link RCCL — the caller hands over the function and its communicator (lili_om_amd/rccl.py does it with the librccl.so that
 * PyTorch loaded).  allreduce == NULL runs the same staged launches without collectives (one rank).  restart_every /
 * restart_slot as in lili_s2m_iterate_restart.  d_counts: DEVICE int32[2], d_gram: DEVICE double[LILI_GRAM_DOUBLES],
 * both caller-owned and valid until the stream has drained.  Every rank then holds the same pose (same reduced Gram, same
 * GN step), no broadcast is needed.  With allreduce == lili_p2p_allreduce (below) the exchange is folded into the count kernel and
 * into the reduce + Gauss-Newton kernel: associate, counts + exchange, linearise, reduce + exchange + GN = 4 launches per iteration. */
typedef int (*lili_allreduce_fn)(const void* sendbuff, void* recvbuff, size_t count, int datatype, int op, void* comm, void* stream);
int lili_s2m_iterate_sharded(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, int n_iters, int restart_every,
                             int restart_slot, lili_allreduce_fn allreduce, void* comm, int32_t* d_counts, double* d_gram);
/* The sliding window across ranks (BASELINE configs[4]: the reference evaluates the lidar blocks of ALL keyframes of the window per solver
 * evaluation, L/src/BackendFusion.cpp:919-992).  Every rank holds its shard of every slot's queries (set_queries with the shard) and the
 * whole map; per evaluation ONE exchange of n_slots x LILI_GRAM_DOUBLES doubles makes every rank hold the same n Gram records bit for bit
 * (lili_p2p: folded into the reduction launch; any other lili_allreduce_fn: one call on the n x 72 doubles; NULL: one rank).
 *   lili_s2m_counts_window_sharded     after the slots' associations (lili_s2m_associate / _associate_dev per slot): the GLOBAL correspondence
 *                                      counts of every slot in ONE exchange of 2 n int32 into d_counts (DEVICE, [surf, edge] per slot; kept valid
 *                                      by the caller) — the count-scaled ROT flavour needs them, the others may skip the call.  They stay
 *                                      in force for the slots' linearisations until the next association.  Async.
 *   lili_s2m_linearize_window_dev      the n records at the slots' DEVICE poses into d_gram (DEVICE, n x LILI_GRAM_DOUBLES).  Async.
 *   lili_s2m_linearize_window_sharded  the same at host poses t (3 per slot) / q (4 per slot), blocking, records copied out like
 *                                      lili_s2m_linearize_window: one evaluation of the caller's solver.
 *   lili_s2m_iterate_window_sharded    n_iters x [associate every slot, counts exchange (count-scaled flavours), linearise every slot, ONE
 *                                      reduction launch + exchange + Gauss-Newton update of every slot]: the lidar-only registration of
 *                                      every keyframe as in lili_s2m_iterate_window, 2 exchanges per iteration whatever n_slots is. */
int lili_s2m_counts_window_sharded(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, lili_allreduce_fn allreduce, void* comm, int32_t* d_counts);
int lili_s2m_linearize_window_dev(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params,
                                  lili_allreduce_fn allreduce, void* comm, double* d_gram);
int lili_s2m_linearize_window_sharded(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const double* t, const double* q,
                                      const lili_s2m_params* params, lili_allreduce_fn allreduce, void* comm, double* d_gram,
                                      double* gram, double* cost, int* counts);
int lili_s2m_iterate_window_sharded(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params, int n_iters,
                                    lili_allreduce_fn allreduce, void* comm, int32_t* d_counts, double* d_gram);
/* Peer-to-peer all-reduce for the two records of the sharded loop (the loop being sharded is
 * L/src/BackendFusion.cpp:1536,1606): every rank owns a mailbox in its HBM that all peers map through hipIpc; one small kernel per
 * all-reduce stores this rank's record into every peer's mailbox over xGMI, waits for the peers' records in its own, and adds them IN
 * RANK ORDER — so all ranks hold bit-identical sums.  lili_p2p_allreduce has the signature of ncclAllReduce (lili_allreduce_fn) with
 * comm = the lili_p2p*; records of at most 640 elements (a window of 8 Gram records is 576 doubles), datatype 2 (int32) or 8 (f64), op 0 (sum).
 *   lili_p2p_create   one per rank (rank, world <= 16), on the context's device
 *   lili_p2p_handle   this rank's mailbox handle (LILI_P2P_HANDLE_BYTES, opaque) — the caller all-gathers the handles (MPI,
 *                     torch.distributed, a file ...) and hands all of them, in rank order, to
 *   lili_p2p_connect  (maps the peers' mailboxes; one process per GPU, or several processes on one GPU)
 *   lili_p2p_status   0 = ok, 1 = a wait for a peer gave up (the record is then undefined, the slot's gn_status is 2).  The failure is
 *                     sticky and contagious: the rank publishes nothing any more and raises the failure word of every peer, whose
 *                     next exchange fails at its first look; lili_s2m_iterate_sharded then returns LILI_E_STATE on every rank.
 *   lili_p2p_set_timeout  how long an exchange may wait for a peer (device time, default 10 s).  The FIRST exchange absorbs the ranks'
 *                     start-up skew (code-object load, data loading): keep it generous, or barrier the control plane first. */
#define LILI_P2P_HANDLE_BYTES 64
/* Slot-per-rank window (the split of the sliding window that scales, SURVEY §8e / L/src/BackendFusion.cpp:919-980): keyframe slots[i] lives on rank owner[i] at FULL
 * size (all its queries; the other ranks hold only its pose slot) and every evaluation ends with ONE exchange of the n x LILI_GRAM_DOUBLES doubles in which each record has
 * a single non-zero contributor — an all-gather carried by the rank-order sum of `allreduce` (lili_p2p_allreduce: inside the reduction launch).  No count exchange: the
 * owner's count is the global one.  _linearize_: records of one evaluation at the slots' DEVICE poses into d_gram (device, n x LILI_GRAM_DOUBLES; identical on every
 * rank, slot i's record = what lili_s2m_linearize_window returns for it on the owner, a -0.0 entry read as +0.0); _iterate_: n_iters x (association of the owned
 * keyframes, their linearisation, exchange, Gauss-Newton update of EVERY slot on every rank).  Every rank must have set the same pose in every slot.  Async. */
int lili_s2m_linearize_window_gather(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params, const int* owner, int rank,
                                     lili_allreduce_fn allreduce, void* comm, double* d_gram);
int lili_s2m_iterate_window_gather(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params, int n_iters, const int* owner, int rank,
                                   lili_allreduce_fn allreduce, void* comm, double* d_gram);
/* _linearize_ at the body poses (t[3 n], q[4 n]) of the call instead of the device poses, records copied out as lili_s2m_linearize_window returns them (gram 64 n, cost n,
 * counts 2 n; one synchronisation): one solver evaluation of the slot-per-rank window (ceres::CostFunction::Evaluate of the joint window, L/src/BackendFusion.cpp:919-992;
 * include/lili_ceres_adapter.h LidarWindowFactor::gather_over_ranks). */
int lili_s2m_linearize_window_gather_at(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const double* t, const double* q, const lili_s2m_params* params,
                                        const int* owner, int rank, lili_allreduce_fn allreduce, void* comm, double* d_gram, double* gram, double* cost, int32_t* counts);

typedef struct lili_p2p lili_p2p;
int lili_p2p_create(lili_ctx* ctx, int rank, int world, lili_p2p** out);
int lili_p2p_handle(lili_p2p* comm, void* handle);
int lili_p2p_connect(lili_p2p* comm, const void* all_handles);
int lili_p2p_allreduce(const void* sendbuff, void* recvbuff, size_t count, int datatype, int op, void* comm, void* stream);
int lili_p2p_status(lili_p2p* comm);
int lili_p2p_set_timeout(lili_p2p* comm, double seconds);
void lili_p2p_destroy(lili_p2p* comm);
/* Convenience: n_iters x (accumulate + gn_update) on an internal buffer.  Async. */
int lili_s2m_iterate(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, int n_iters);

/* The INNER iteration of the reference back-end (ceres::Solve on fixed correspondences, L/src/BackendFusion.cpp:984-992; the
 * front-end's L/src/LidarOdometry.cpp:533): n_iters x [linearise the records of the LAST association at the device pose, reduce,
 * Gauss-Newton update] — no re-association.  One launch per iteration.  want_cost != 0 also evaluates sum 1/2 rho (slot 64 of the
 * internal record), as an LM caller needs it.  Async. */
int lili_s2m_iterate_inner(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, int n_iters, int want_cost);

/* lili_s2m_iterate for several slots at once (the keyframes of one sliding window, or several sensors): every slot
 * runs its own chain on its own stream, forked from / joined to the context's stream, so the latency-bound linearise /
 * reduce launches of one slot overlap the association of another.  Same results as iterating the slots one after the
 * other; all slots share the map index.  Async. */
int lili_s2m_iterate_window(lili_ctx* ctx, const int* slots, int n_slots, int kind_mask, const lili_s2m_params* params, int n_iters);
/* Profiling aid: with LILI_DEBUG bit 256 set, kernels stamp a 100 MHz device clock at their phases; returns the 16 stamps. */
int lili_s2m_debug_times(lili_ctx* ctx, int slot, long long out[16]);
/* Async device-to-device copy of the body pose of src_slot into dst_slot (no host round trip). */
int lili_s2m_pose_copy(lili_ctx* ctx, int dst_slot, int src_slot);
/* lili_s2m_iterate that re-initialises the pose from restart_slot before iterations 0, restart_every, 2*restart_every...
 * ("one scan registration = restart_every GN iterations"; restart_every = 0 disables).  If assoc_ms is non-NULL the
 * association launches are bracketed by HIP events on the context's stream, their total duration (ms) is returned and
 * the call synchronises; with NULL it is async like lili_s2m_iterate. */
int lili_s2m_iterate_restart(lili_ctx* ctx, int slot, int kind_mask, const lili_s2m_params* params, int n_iters, int restart_every,
                             int restart_slot, float* assoc_ms);

/* Host-side helper used by the ceres adapter and the host LM: Gauss-Newton step from a host Gram. */
int lili_gn_step_host(const double gram[64], double t[3], double q[4], double delta[6]);

/* Square-root form of a Gram record for ceres (see include/lili_ceres_adapter.h): a 9-residual block whose
 * J^T J, J^T r and cost equal those of the N robustified lidar residuals the Gram was reduced from. */
int lili_gram_to_factor(const double gram[64], double cost, double residuals[9], double jacobian[63]);

/* ---- the joint keyframe window on the device: lidar + IMU factors + priors (lili_window.hip) -----------------
 * The problem ceres::Solve gets in optimizeSlidingWindowWithLandMark (L/src/BackendFusion.cpp:843-1007): n_kf keyframes x (t[3], q[4] w x y z
 * with QuaternionParameterization, speed-bias[9] = v, ba, bg), the lidar blocks of every keyframe (the records of the slots' last association,
 * robustified by params->loss; correspondences stay fixed), one IMU factor between consecutive keyframes (ImuFactor.h:18-144), and either the
 * marginalisation prior (MarginalizationFactor::Evaluate) or the speed-bias priors (PriorFactor.h:13-23); the last three enter without a loss.
 * The prior of the NEXT window (MarginalizationInfo::PreMarginalize + Marginalize: the factors again at the solved state, Schur complement over the
 * oldest keyframe, two eigen-decompositions) is lili_window_marginalize below; lili_window_cycle does solve, sign unification, that prior and the
 * write-back gates in one call and keeps the prior on the device: a keyframe cycle is prepare -> pre-integrate -> cycle.
 * The IMU factors' records come from lili_imu_preintegrate below (raw samples in, lili_window_imu out).  With the separate calls the write-back
 * gates and the quaternion sign unification stay with the caller — their RESULTS are handed in as the plain arrays below (host memory, copied once per call).  A state is n_kf x 16 doubles: t[3], q[4], speed-bias[9] per keyframe; "local" means 15 per keyframe: t, the 3 quaternion-plus
 * coordinates, speed-bias. */
#define LILI_WINDOW_MAX_KF 4          /* 15 * n_kf <= 60 local dimensions: every matrix of the solve stays in LDS */
#define LILI_WINDOW_STATE_DOUBLES 16
typedef struct lili_window_imu {      /* what Preintegration holds when the solve starts */
    double sum_dt, g[3];
    double delta_p[3], delta_q[4] /* w x y z */, delta_v[3];
    double lin_ba[3], lin_bg[3];      /* the biases the pre-integration was linearised at */
    double jacobian[225], covariance[225];   /* 15 x 15 row-major, order O_P O_R O_V O_BA O_BG */
} lili_window_imu;
typedef struct lili_window_prior {    /* r = r0 + J0 * dx(x, x0) over the kept blocks */
    int32_t n_rows, n_cols;           /* J0 is n_rows x n_cols row-major, both <= 60; n_cols = sum of the blocks' local sizes (3, 3, 9) */
    int32_t n_blocks, reserved_;
    const int32_t* block_kind;        /* per kept block: 0 = t, 1 = q (dx = +-2 vec(normalized(q0^-1 q)), sign of its w), 2 = speed-bias */
    const int32_t* block_keyframe;    /* keyframe of the window the block belongs to; a (keyframe, kind) pair at most once */
    const double* x0;                 /* the blocks' linearisation points, global sizes (3, 4, 9), concatenated */
    const double* J0;
    const double* r0;
} lili_window_prior;
typedef struct lili_window_problem {
    int32_t n_kf;                     /* 2 .. LILI_WINDOW_MAX_KF */
    int32_t kind_mask;                /* lidar kinds; 0 = no lidar blocks (lili_window_evaluate only) */
    const int32_t* slots;             /* matcher slot of every keyframe */
    const lili_window_imu* imu;       /* n_kf - 1 factors, or NULL */
    const lili_window_prior* prior;   /* or NULL */
    const double* sb_prior;           /* n_kf x 9 speed-bias prior means, a row starting with NaN = none on that keyframe; or NULL.  r = 15 (sb - mean) */
    double q_lb[4], t_lb[3];          /* extrinsic of the lidar blocks; q_lb all zero = the one in params */
} lili_window_problem;
/* sqrt_info = LLT(covariance^-1).matrixL()^T of an IMU factor, as the calls below compute it once per solve on the host (15 x 15 row-major).
 * LILI_E_ARG if the covariance is not positive definite.  Needs no context and no GPU. */
int lili_window_sqrt_info(const double covariance[225], double sqrt_info[225]);
/* What Ceres' evaluator hands its minimiser at `state`: cost = sum 1/2 rho(r^2) of the lidar records + 1/2 |r|^2 of every other block, gradient
 * (15 n_kf) and J^T J ((15 n_kf)^2 row-major, optional) in local coordinates.  The slots' poses are not touched.  Blocking. */
int lili_window_evaluate(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const double* state,
                         double* cost, double* gradient, double* JtJ);
/* ceres::Solve on that problem as ONE persistent launch (the loop of lili_s2m_solve_lm on 15 n_kf dimensions, the accept / reject decision
 * taken on the whole window).  state: in = initial, out = final (written when summary != NULL; with summary == NULL the call is asynchronous
 * and lili_window_state_get fetches it later).  The slots' device poses end at the final (t, q) of their keyframes.  Refusals (bad n_kf,
 * a slot without records, a covariance that is not positive definite, a prior whose n_cols does not match its blocks) leave them untouched.
 * summary->n_surf / n_edge: the first keyframe's. */
int lili_window_solve(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const lili_lm_options* options,
                      double* state, lili_lm_summary* summary);
/* the final state of the last lili_window_solve of this context (n_kf x 16 doubles).  Blocking. */
int lili_window_state_get(lili_ctx* ctx, int n_kf, double* state);

/* ---- the window's next prior (MarginalizationInfo::Marginalize, L/src/MarginalizationFactor.cpp:128-202) ----
 * Schur complement and square-root prior of a GIVEN system, MarginalizationFactor.cpp:176-201 in f64 on the device (one workgroup, everything in
 * LDS): A is pos x pos (leading dimension ld, symmetric, 2 <= pos <= 60), b has pos entries, the first m dimensions (1 <= m < pos) go, n = pos - m.
 *   Amm = (Amm + Amm^T) / 2, eigen-decomposition, pseudo-inverse with the reference's ABSOLUTE threshold 1e-8 (eigenvalues > 1e-8 are inverted, the
 *   others become 0);  S = Arr - Arm Amm^+ Amr,  bs = brr - Arm Amm^+ bmm;  eigen-decomposition of S;  J0 = diag(sqrt(lambda+)) V^T (n x n row-major),
 *   r0 = diag(sqrt(1 / lambda)+) V^T bs;  rows whose eigenvalue is <= 1e-8 are exactly zero;  *rank = the number of the others.
 * The eigen-solver is a cyclic Jacobi method with fixed sums and a fixed order of rotations: two calls give identical bits.  Rows are ordered by
 * ascending eigenvalue and each eigenvector has its largest-magnitude component positive (the first such on ties) — Eigen's order is the same, its
 * signs are arbitrary; J0 and r0 are unique only up to an orthogonal transform of the rows, and nothing may depend on either choice (J0^T J0, J0^T r0,
 * r0^T r0 and the rank do not).  Blocking, host pointers.  LILI_E_ARG (bad sizes, a null pointer, a non-finite entry) and LILI_E_NUMERIC (the sweep
 * cap was reached) write nothing. */
int lili_marg_schur(lili_ctx* ctx, const double* A, size_t ld, const double* b, int pos, int m, double* J0, double* r0, int* rank);

/* A marginalisation prior with its storage: `prior` points into the arrays of the SAME object, so the object is not to be copied or moved once
 * filled; &storage->prior goes to the next lili_window_solve / lili_window_evaluate as lili_window_problem::prior. */
typedef struct lili_window_prior_storage {
    lili_window_prior prior;
    int32_t block_kind[3 * LILI_WINDOW_MAX_KF], block_keyframe[3 * LILI_WINDOW_MAX_KF];
    int32_t rank;                     /* rows of J0 that are not zero */
    int32_t sweeps_mm, sweeps_s;      /* Jacobi sweeps the two eigen-decompositions (Amm, Schur complement) took: diagnosis only */
    int32_t reserved_;
    double x0[LILI_WINDOW_STATE_DOUBLES * LILI_WINDOW_MAX_KF];
    double r0[15 * LILI_WINDOW_MAX_KF];
    double J0[15 * LILI_WINDOW_MAX_KF * 15 * LILI_WINDOW_MAX_KF];
} lili_window_prior_storage;
/* The prior of the next window from this window's problem and its solved `state` (n_kf x 16): what PreMarginalize + Marginalize leave in
 * last_marginalization_info (L/src/BackendFusion.cpp:1009-1184).  Exactly the reference's factor set is evaluated at `state`, correspondences fixed,
 * every quaternion block by the LAST THREE of its four global columns (MarginalizationFactor.cpp:9-17):
 *   problem->prior, if present (MarginalizationFactor::Evaluate);  a speed-bias prior for every row of problem->sb_prior that is present, with the
 *   mean as given;  the IMU factor between keyframes 0 and 1 ONLY (further entries of problem->imu are ignored, as in the reference);  the lidar
 *   blocks of every keyframe, kinds problem->kind_mask, linearised at `state` by the launches of lili_window_evaluate.
 * Keyframe 0's blocks are marginalised; the blocks of the later keyframes that at least one factor touches are kept, in (keyframe, kind) order —
 * with the reference's set and n_kf = 3 the last keyframe's speed-bias is touched by nothing and is no block of the prior (21 columns).  `out` lists
 * each kept block with its keyframe index SHIFTED BY -1 (addr_shift, L:1170-1177: the next window's numbering) and x0 = its value in `state`;
 * n_rows = n_cols, rows beyond out->rank are zero.  The lidar launches, then one single-workgroup launch (assembly + the code of lili_marg_schur);
 * blocking, one synchronisation.  Refusals — those of lili_window_evaluate, a state that is not finite, no factor on keyframe 0 or on the others,
 * LILI_E_NUMERIC — leave `out` and the slots' poses untouched. */
int lili_window_marginalize(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const double* state,
                            lili_window_prior_storage* out);

/* ---- the window cycle in one call: solve, sign unification, next prior, write-back gates (DESIGN.md §7h "The cycle") ----
 * lili_window_cycle is the chain
 *   1. lili_window_solve(problem, state_in);
 *   2. every keyframe's q with w < 0 negated (unifyQuaternion, L/src/BackendFusion.cpp:994-1006; -0.0 and NaN are left alone, as `< 0` leaves them);
 *   3. lili_window_marginalize(problem, the unified state), every PRESENT row of problem->sb_prior replaced by that keyframe's solved speed-bias, as the
 *      reference hands it in (L:1045-1057: the first marginalisation's speed-bias priors have residual 0 and information 225 I) — the prior stays in
 *      device memory, in a buffer of the context no other call writes (the RESIDENT prior); lili_window_prior_get copies it out;
 *   4. the write-back gates of L:1187-1284 between state_in and the unified state,
 * as one upload, the solve launch, a single-wave write-back launch, the lidar launches at the slots' DEVICE poses, the marginalisation launch, one
 * synchronisation and one read-back.  With use_resident_prior = 1 the problem's prior is the resident one — the prior step 3 of the previous cycle
 * left, or the one lili_window_prior_set seeded — and reaches the kernels by a device-to-device copy.  The same kernels run on the same doubles:
 * summary, `solved` and the prior are the chain's bits.
 * Gates (strict '<' accepts; a NaN refuses):  pnorm = sqrt(d0*d0 + d1*d1 + d2*d2) of state_in - solved, summed left to right, likewise vnorm;
 * qnorm = |vec(inverse(normalized(q_solved)) * q_in)| with normalized = q / sqrt(x*x + y*y + z*z + w*w), inverse = conjugate / squared norm and
 * Eigen's product; the six bias components one by one, |d| < gate.  A refused component keeps the value of state_in.  next_state's q is, where the
 * q gate accepts, Eigen 3.3's Quaterniond(normalized(q).toRotationMatrix()) (all four branches of the conversion), else state_in's q.  Only + - * /
 * and sqrt, compiled without contraction: the bits of a plain IEEE restatement (tests/cycle_model.py).
 * Returns and refuses what the chain returns and refuses (LILI_E_ARG, LILI_E_STATE, LILI_E_NUMERIC of lili_window_marginalize included), and:
 * use_resident_prior = 1 together with problem->prior is LILI_E_ARG, without a resident prior LILI_E_STATE.  A refused cycle enqueues nothing; one that fails behind the solve's
 * launches (LILI_E_NUMERIC, a launch or read-back error) puts the slots' states back and drains the stream: either way the resident prior, `out` and the
 * slots' device poses are as they were.  A solve that ends LILI_LM_STALLED marginalises nothing (prior_updated = 0, the
 * resident prior stays); one that ends LILI_LM_NUMERICAL_FAILURE goes on at the unchanged state, as the reference does.  Afterwards the slots'
 * device poses are the unified (t, q) of `solved`. */
typedef struct lili_window_cycle_options {
    double gate_p, gate_q, gate_v, gate_ba, gate_bg;  /* 10, 10, 10, 22, 22: the literals of L:1215-1283; strict '<' accepts */
    int32_t use_resident_prior;   /* 0: problem->prior (may be NULL) as today; 1: the prior the previous cycle left in this context */
    int32_t reserved_;
} lili_window_cycle_options;     /* NULL = the defaults, use_resident_prior = 0 */
typedef struct lili_window_cycle_result {
    lili_lm_summary summary;
    double solved[16 * LILI_WINDOW_MAX_KF];      /* the solve's final state after sign unification (tmpTrans / tmpQuat / tmpSpeedBias) */
    double abs_state[16 * LILI_WINDOW_MAX_KF];   /* after the gates: abs_poses (raw unified q), Ps, Vs / para_speed_bias */
    double next_state[16 * LILI_WINDOW_MAX_KF];  /* abs_state with q replaced by Quaterniond(Rs): what the next "eigen to double" reads */
    uint32_t refused[LILI_WINDOW_MAX_KF];        /* bit 0 p, 1 q, 2 v, 3..5 ba, 6..8 bg */
    int32_t prior_updated, prior_n, prior_blocks, rank, sweeps_mm, sweeps_s;
} lili_window_cycle_result;      /* rows of keyframes >= n_kf and summary rows that were not logged are zero */
int lili_window_cycle(lili_ctx* ctx, const lili_window_problem* problem, const lili_s2m_params* params, const lili_lm_options* options,
                      const lili_window_cycle_options* cycle_options, const double* state_in, lili_window_cycle_result* out);
/* drops the resident prior (loop closure: L:2635-2638, marg = false) */
int lili_window_cycle_reset(lili_ctx* ctx);
/* copy of the resident prior (blocking); LILI_E_STATE when there is none.  rank / sweeps: those of the cycle that built it; after
 * lili_window_prior_set the number of non-zero rows and 0, 0. */
int lili_window_prior_get(lili_ctx* ctx, lili_window_prior_storage* out);
/* seeds the resident prior from host memory (restart from a saved prior): validated as lili_window_problem::prior is, except that its keyframes
 * are checked against LILI_WINDOW_MAX_KF here and against n_kf by the cycle that uses it.  A refusal leaves the resident prior as it was. */
int lili_window_prior_set(lili_ctx* ctx, const lili_window_prior* prior);

/* ---- IMU pre-integration on the device (lili_imu.hip) ---------------------------------------------
 * What the constructor plus one push_back(dt, acc, gyr) per sample leave in a Preintegration object (L/include/factors/Preintegration.h:27-173): the
 * mid-point step of (delta_p, delta_q, delta_v) with delta_q.normalize() after every sample, sum_dt, jacobian = F ... F I and covariance
 * P <- F P F^T + V N V^T from 1e-4 I, F / V with the reference's literal coefficients, N from its four noise constants.  f64, no contraction: the eleven
 * state values are the bits a build of the reference header produces; Jacobian and covariance agree with it to rounding.
 * One segment = one IMU factor (the samples between two keyframes); segments are independent, one workgroup each, so every factor of a window — or
 * the same samples at new linearisation biases, Preintegration::Repropagate — goes in ONE call.  out[i] can be used as lili_window_problem::imu[i].
 * With predict != 0 a segment also carries processIMU's state propagation (L/src/BackendFusion.cpp:815-821) from (P0, R0, V0) — R0 a row-major 3 x 3
 * that is multiplied on, never re-normalised, as in the reference — with the same biases; processIMU's own g, subtracted from the rotated accelerations,
 * is the negative of the segment's g (g_vec_ = -g, L:807): pred[i] = the next keyframe's initial guess.  pred may be NULL when no segment predicts; entries of segments with predict == 0 are not written.
 * One packed upload from page-locked staging, one launch, one synchronisation; blocking.  LILI_E_ARG — a null pointer, n_seg outside
 * 1 .. LILI_IMU_MAX_SEGMENTS, n outside 0 .. LILI_IMU_MAX_SAMPLES, a sample / bias / g / start state that is not finite, a negative dt, a predicting
 * segment without pred — leaves out and pred untouched. */
#define LILI_IMU_MAX_SAMPLES 4096     /* per segment */
#define LILI_IMU_MAX_SEGMENTS 64
typedef struct lili_imu_segment {
    const double* dt; const double* acc; const double* gyr;   /* n, n x 3, n x 3: the arguments of push_back, host memory (may be NULL when n == 0) */
    int32_t n, predict;                                       /* n >= 0; predict != 0: P0 / R0 / V0 are read, P1 / R1 / V1 written */
    double acc0[3], gyr0[3], lin_ba[3], lin_bg[3], g[3];      /* constructor arguments; g = the factor's gravity (g_vec_), copied to out[i].g */
    double P0[3], R0[9], V0[3];
} lili_imu_segment;
typedef struct lili_imu_prediction { double P1[3], R1[9], V1[3]; } lili_imu_prediction;
int lili_imu_preintegrate(lili_ctx* ctx, const lili_imu_segment* seg, int n_seg, lili_window_imu* out, lili_imu_prediction* pred);
/* Device time of the last lili_imu_preintegrate's kernel in milliseconds, taken with two events around the launch when option "imu_time" is 1
 * (measurement aid, tools/preint_time.py); LILI_E_STATE when there is none. */
int lili_imu_kernel_ms(lili_ctx* ctx, float* ms);

/* The sample slicing of saveKeyFramesAndFactors for one keyframe (L/src/BackendFusion.cpp:1700-1771), host code without a context: the samples with
 * stamp < t_kf from st->idx on are consumed — dt from the running st->t_cur (< 0: unset, the first dt is then 0), accelerations clamped to +-15 / +-15 /
 * +-18 —, then, if a sample is left, ONE boundary sample at t_kf interpolated with w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2) between the last
 * consumed values (zeros when none was consumed, as in the reference) and the next sample, clamped again; st->t_cur = t_kf, st->idx = the first sample
 * not consumed.  The rows written (dt_out n, acc_out / gyr_out n x 3; *n_out of them) are the push_back arguments of the keyframe's segment.
 * st->acc0 / gyr0 on entry are the segment's constructor arguments, on exit the next segment's (the last row written).  A state that is all zero (or
 * after lili_imu_kf_reset) takes acc0 / gyr0 from the first sample as it is, unclamped (imuHandler, L:636-662), before anything else: read them after
 * the call in that case, they are unchanged by a call that consumes nothing.  LILI_E_ARG — a null pointer, or cap smaller than the rows to write —
 * writes nothing and leaves the state as it was.  n = 0 or st->idx >= n: no rows, st->t_cur = t_kf. */
typedef struct lili_imu_kf_state { int64_t idx; double t_cur; double acc0[3], gyr0[3]; int32_t first, reserved; } lili_imu_kf_state;
void lili_imu_kf_reset(lili_imu_kf_state* st);
int lili_imu_keyframe_samples(lili_imu_kf_state* st, const double* stamps, const double* acc, const double* gyr, size_t n, double t_kf,
                              double* dt_out, double* acc_out, double* gyr_out, size_t cap, size_t* n_out);

/* ---- Per-frame trajectory: IMU chain and local pose graph on the device (lili_local_graph.hip) --------------------------
 * What buildLocalPoseGraph and optimizeLocalGraph (L/src/BackendFusion.cpp:1892-2175, 1309-1384, L/include/factors/LidarPoseFactor.h) do after a window
 * solve: a pose for each of the n scans between two keyframes.  A pose is 7 doubles, p (3) then q (w, x, y, z); a measurement is 7 doubles, delta p then
 * delta q.  Everything is host memory; every call is blocking: one packed upload from page-locked staging, ONE launch of one workgroup (f64, no
 * contraction), one synchronisation.
 *
 * LILI_LOCAL_MAX_FRAMES: L/src/LidarOdometry.cpp:575 makes a scan a keyframe at the latest when two non-keyframes precede it, so the reference itself
 * never produces n > 2; 16 leaves room for other keyframe rules and keeps every matrix of the solve (6 n = 96 columns, block tridiagonal) in LDS.
 *
 * lili_local_graph_propagate — the IMU walk of L:1897-2108 and the measurements of L:2110-2170.  walk: the raw sample buffer (stamps / acc / gyr, n_imu
 *   entries), ii0 = imu_idx_in_kf of the left keyframe, scan_stamps = the n + 2 stamps t_0 (left keyframe), t_1 .. t_n (the scans), t_{n+1} (right keyframe),
 *   the start state (P0, R0 row-major and multiplied on as it is, V0: INTEGRATION.md says which Ps / Rs / Vs the reference passes), g (subtracted from the
 *   rotated accelerations) and the left anchor's pose, which the first measurement is relative to.  Kept from the text: biases are zero; deltaQ is the
 *   un-normalised small-angle quaternion, turned into a matrix and multiplied on, R is never re-normalised; accelerations are clamped to +-15 / +-15 / +-18
 *   wherever the text clamps (not at the opening interpolation of a non-keyframe interval, but at the one of the closing interval); the sample loop compares
 *   with a strict <; the index steps back by one after every frame but the last; the closing partial step takes dt1 from the sample in front of the index
 *   even when the loop consumed nothing; the quaternion of a matrix follows Eigen's branches.  f32_positions != 0: a frame's position goes through the float
 *   members of pcl::PointXYZI as pose_each_frame stores it (the quaternions are PointPoseInfo's doubles); 0: f64 throughout.
 *   Out: poses (n x 7), end_state (15: P, R row-major, V at t_{n+1}), meas ((n + 1) x 7).
 * lili_local_graph_evaluate — cost, gradient (6 n) and J^T J (6 n x 6 n, row-major, exactly zero outside the block tridiagonal) of the n + 1 factors at
 *   `poses`, in the local coordinates of ceres::QuaternionParameterization (translation block, then rotation block per frame); anchors = p_L q_L p_R q_R (14).
 *   Residual k = 2 vec(dq^-1 q_a^-1 q_b), then q_a^-1 (p_b - p_a) - dp on nodes k, k + 1 of [L, x_1 .. x_n, R], unit weight, no loss, inverse() = conjugate /
 *   squared norm; the Jacobians are analytic.
 * lili_local_graph_solve — Ceres 2.0's TrustRegionMinimizer with DoglegStrategy (TRADITIONAL_DOGLEG, Jacobi scaling) on that problem from `poses`
 *   (in: the initial frame poses, out: the solved ones) as one persistent single-workgroup launch; options NULL = lili_lm_default_options (max_iterations
 *   15, as optimizeLocalGraph sets it).  The regularised normal equations are solved by a banded Cholesky factorisation where Ceres uses QR on the augmented
 *   Jacobian.  A candidate that triggers the parameter or the function tolerance is not taken.
 * lili_local_graph — propagate, then solve from the propagated poses between the left anchor and `right` (the right keyframe's solved pose), in the same
 *   single launch: poses, meas and summary are byte-identical to the two calls in a row.
 * n = 0 (two keyframes in a row) is valid everywhere: no poses, one measurement, zero iterations, termination LILI_LM_GRADIENT_TOLERANCE (nothing to move),
 *   initial_cost = final_cost = the cost of the one factor between the anchors.
 * LILI_E_ARG — a null pointer, n outside 0 .. LILI_LOCAL_MAX_FRAMES, a non-finite input, scan stamps that are not strictly increasing, ii0 < 0, any sample
 *   index the walk would read at or beyond n_imu (the text reads imu_buf[ii + 1] past the last scan stamp; checked on the host before the launch), an
 *   interpolation with dt1 + dt2 == 0, more than LILI_IMU_MAX_SAMPLES samples between the first and the last index read, options as lili_s2m_solve_lm
 *   refuses them — leaves every output untouched. */
#define LILI_LOCAL_MAX_FRAMES 16
typedef struct lili_local_walk {
    const double* stamps; const double* acc; const double* gyr;    /* n_imu, n_imu x 3, n_imu x 3 */
    int64_t n_imu, ii0;
    const double* scan_stamps;                                      /* n + 2 */
    double P0[3], R0[9], V0[3], g[3];
    double left[7];                                                 /* the left anchor's pose */
    int32_t f32_positions, reserved_;
} lili_local_walk;
typedef struct lili_local_graph_summary {
    lili_lm_summary lm;                          /* termination: LILI_LM_*; n_surf / n_edge are 0 */
    double final_mu;                             /* DoglegStrategy's mu after the last linearisation */
    int32_t dogleg_case[LILI_LM_MAX_LOG];        /* per logged candidate: 1 = Gauss-Newton step, 2 = scaled gradient, 3 = interpolated between the two */
    int32_t reused[LILI_LM_MAX_LOG];             /* ... and whether it came from the previous candidate's subproblem (after a rejected step) */
} lili_local_graph_summary;
int lili_local_graph_propagate(lili_ctx* ctx, const lili_local_walk* walk, int n, double* poses, double* end_state, double* meas);
int lili_local_graph_evaluate(lili_ctx* ctx, int n, const double* anchors, const double* meas, const double* poses, double* cost, double* gradient, double* jtj);
int lili_local_graph_solve(lili_ctx* ctx, int n, const double* anchors, const double* meas, double* poses, const lili_lm_options* options,
                           lili_local_graph_summary* summary);
int lili_local_graph(lili_ctx* ctx, const lili_local_walk* walk, int n, const double* right, const lili_lm_options* options, double* poses, double* meas,
                     lili_local_graph_summary* summary);
/* Device time of the last lili_local_graph* call's kernel in milliseconds (option "local_graph_time", tools/local_graph_time.py); LILI_E_STATE when there is none. */
int lili_local_graph_kernel_ms(lili_ctx* ctx, float* ms);

/* ---- Global pose graph over every frame: loop-closure correction on the device (lili_pose_graph.hip) ------------------
 * What saveKeyFramesAndFactors (L/src/BackendFusion.cpp:1820-1889), performLoopClosure (L:2587-2633) and correctPoses (L:2177-2311) do with GTSAM: one node per
 * scan, a prior on node 0, a chain factor between consecutive scans, a few loop factors; solved as a batch by Gauss-Newton with full relinearisation.
 *
 * Conventions.  A pose is 7 doubles, p (3) then q (w, x, y, z).  The tangent is xi = (omega, v), ROTATION FIRST (gtsam::Pose3's order: the reference's variance
 * vectors apply index for index).  X (+) xi = (p + R v, normalise(q * Exp(omega)));  between(A, B) = (R_A^T (p_B - p_A), q_A^-1 * q_B).
 * Between-factor on nodes (a, b), measurement Z = (t_Z, q_Z), variances s^2 (6):  e = (Log(R_Z^T R_A^T R_B), R_Z^T (R_A^T (p_B - p_A) - t_Z)),  r = e / s.
 * Prior on node 0: e = (Log(R_Z^T R_0), R_Z^T (p_0 - t_Z)).  Cost = 1/2 sum |r|^2; a loop may carry a robust loss (lili_pose_graph_add_loop_robust below).  The right Jacobian inverse of SO(3) inside the factor
 * Jacobians uses its series below LILI_PG_SMALL_ANGLE (rad) and the closed form above it.
 * Node 0's prior sits at its own pose as given; the chain measurement of node i is between(pose[i - 1], pose[i]) of the poses AS GIVEN AT APPEND TIME and is
 * frozen from then on; the initial estimate of a new node is its given pose.  Quaternions are normalised on entry.
 *
 * lili_pose_graph_reset    — empties the graph (device memory is kept).
 * lili_pose_graph_append   — n >= 1 new nodes.  prev: NULL for the first call on an empty graph (node 0 gets the prior), otherwise the pose of the graph's LAST
 *                            node in the frame of `poses` (the caller's current value for it; the first new node's measurement is between(prev, poses[0])).
 *                            *first_id (optional) = the id of poses[0].
 * lili_pose_graph_add_loop — BetweenFactor(from, to, meas, var): meas = between(corrected pose of `from`, pose of `to`) (lili_loop_measurement), var = 6 variances.
 * lili_pose_graph_info / _get / _set — sizes; estimates of nodes first .. first + n - 1; overwrite those estimates (measurements stay as they are).
 * lili_pose_graph_evaluate — at the current estimates: cost, gradient (6 N), the diagonal blocks of H = J^T J (N x 36, row-major 6 x 6, loop factors included),
 *                            sub (N - 1 blocks): sub[i] = H block (i + 1, i) of the CHAIN factor alone, loop_blocks[l] = H block (from, to) of loop l alone.
 *                            sub may be NULL for N == 1, loop_blocks for no loops.  options NULL = the defaults (only the variances are read).
 * lili_pose_graph_solve    — Gauss-Newton: H delta = -g, X <- X (+) delta.  Per iteration, in this order: |g|inf <= gradient_tolerance ends it before a step
 *                            (LILI_LM_GRADIENT_TOLERANCE); a non-positive pivot ends it with the previous estimate (LILI_LM_NUMERICAL_FAILURE); a step that raises
 *                            the cost is NOT taken (LILI_PG_COST_INCREASED, the previous estimate); otherwise the step is taken and |delta|inf <=
 *                            parameter_tolerance (LILI_LM_PARAMETER_TOLERANCE), |cost - new cost| <= function_tolerance * cost (LILI_LM_FUNCTION_TOLERANCE), then
 *                            max_iterations (LILI_LM_MAX_ITERATIONS) end it.  summary: iterations = steps computed; cost[k], step_inf[k] = the candidate's cost and
 *                            |delta|inf of iteration k, grad_inf[k] = |g|inf at its linearisation (the first 16).  The elimination is a one-level nested
 *                            dissection: separators = every loop endpoint and every node id that is a multiple of LILI_PG_SEGMENT; the stretches between them are
 *                            eliminated side by side; the reduced system over the separators is factored by one workgroup up to 768 unknowns and by a blocked
 *                            Cholesky over the whole chip beyond (tiles of 96 unknowns: diagonal tile, panel, trailing update on the f64 matrix units; the two
 *                            substitutions tile by tile).  Every launch of the solve is enqueued up front; one synchronisation, one read-back; blocking.  The
 *                            same graph gives the same bits on every run, and a graph of <= 768 reduced unknowns the same bits whatever "pose_graph_max_loops" is.
 *                            The reference's isam->update(graph); isam->update() is nearest to max_iterations = 2.
 * lili_pose_graph_kernel_ms — device time of the last lili_pose_graph_solve's or lili_pose_graph_solve_lm's launches in milliseconds; LILI_E_STATE when there is none.
 *
 * Loops.  A graph takes LILI_PG_MAX_LOOPS loops by default; lili_set_option(ctx, "pose_graph_max_loops", v) with v in LILI_PG_MAX_LOOPS .. LILI_PG_MAX_LOOPS_EXT
 * moves that bound (any time; LILI_E_STATE when the graph already holds more than v loops).  The tables and work arrays follow the graph's actual size; the dense
 * reduced system takes 8 (6 K)^2 bytes for K separators (K <= 64 + 2 loops): 4.7 MB at 32 loops, 1.3 GB at 1024 loops (12 672 unknowns).
 *
 * LILI_E_ARG, with every output and the graph untouched: a null pointer (ctx, poses, meas, var, summary, cost, gradient, diag; sub / loop_blocks where they have
 * entries), a non-finite input, a quaternion more than 1e-6 from unit norm, a non-positive variance, from == to, an id or a range outside the graph, n < 1,
 * more than LILI_PG_MAX_NODES nodes or "pose_graph_max_loops" (default LILI_PG_MAX_LOOPS) loops, append with prev != NULL on an empty graph or prev == NULL on a non-empty one, max_iterations
 * outside 1 .. 1000, a tolerance that is negative or not finite.  LILI_E_STATE: evaluate / solve on an empty graph. */
#define LILI_PG_MAX_NODES 32768
#define LILI_PG_MAX_LOOPS 32               /* the default of option "pose_graph_max_loops" */
#define LILI_PG_MAX_LOOPS_EXT 1024         /* the largest value of option "pose_graph_max_loops" */
#define LILI_PG_SEGMENT 512                /* fixed separators sit at multiples of it: 64 + 2 x 32 separators = 768 reduced unknowns at the default caps */
#define LILI_PG_MAX_LOG 16
#define LILI_PG_SMALL_ANGLE 0.1
#define LILI_PG_COST_INCREASED 7           /* termination, next to the LILI_LM_* codes */
typedef struct lili_pg_options {
    int32_t max_iterations, reserved_;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double prior_var[6], odom_var[6];      /* variances in tangent order (omega, v) */
} lili_pg_options;
typedef struct lili_pg_summary {
    int32_t iterations, termination, n_nodes, n_loops;
    double initial_cost, final_cost;
    double cost[LILI_PG_MAX_LOG], step_inf[LILI_PG_MAX_LOG], grad_inf[LILI_PG_MAX_LOG];
} lili_pg_summary;
/* max_iterations 10, tolerances 1e-6 / 1e-10 / 1e-8 (lili_lm_default_options), prior 1e-6 x 3, 1e-8 x 3, odometry 1e-6 x 3, 1e-4 x 3 (L:552-557) */
void lili_pg_default_options(lili_pg_options* opt);
int lili_pose_graph_reset(lili_ctx* ctx);
int lili_pose_graph_append(lili_ctx* ctx, const double* prev, const double* poses, int n, int* first_id);
int lili_pose_graph_add_loop(lili_ctx* ctx, int from, int to, const double meas[7], const double var[6]);
int lili_pose_graph_info(lili_ctx* ctx, int* n_nodes, int* n_loops);
int lili_pose_graph_get(lili_ctx* ctx, int first, int n, double* poses);
int lili_pose_graph_set(lili_ctx* ctx, int first, int n, const double* poses);
int lili_pose_graph_evaluate(lili_ctx* ctx, const lili_pg_options* options, double* cost, double* gradient, double* diag, double* sub, double* loop_blocks);
int lili_pose_graph_solve(lili_ctx* ctx, const lili_pg_options* options, lili_pg_summary* summary);
int lili_pose_graph_kernel_ms(lili_ctx* ctx, float* ms);
/* Robust loop factors (GTSAM's noiseModel::Robust on the loop's BetweenFactor).  lili_pose_graph_add_loop_robust is lili_pose_graph_add_loop with a loss kind and
 * its scale k; lili_pose_graph_add_loop means LILI_PG_LOSS_NONE.  The prior and the chain factors never carry a loss.  With r = e / s the loop's whitened residual,
 * d^2 = |r|^2 (summed in tangent order) and d = sqrt(d^2):
 *   Huber          w = 1 if d <= k, else k / d         rho = d^2 / 2 if d <= k, else k (d - k / 2)
 *   Cauchy         w = k^2 / (k^2 + d^2)               rho = (k^2 / 2) log1p(d^2 / k^2)
 *   Geman-McClure  w = (k^2 / (k^2 + d^2))^2           rho = (k^2 / 2) d^2 / (k^2 + d^2)
 * The factor is linearised as sqrt(w) r, sqrt(w) J (iteratively re-weighted least squares, no second-order term) and adds rho to the cost where every other factor
 * adds |r|^2 / 2: g = J^T W r is the robust cost's exact gradient, H = J^T W J its approximation.  evaluate (cost, gradient, every block), solve, solve_lm and
 * marginals (Sigma = the inverse of that weighted H) all read the graph this way.
 * LILI_E_ARG, the graph untouched: what lili_pose_graph_add_loop refuses, a loss that is none of the four, and for a loss other than NONE a scale that is not
 * positive and finite (the scale of NONE is ignored).
 *
 * lili_pose_graph_loop_status — what the loss decided: at the current estimates, d^2 (chi2) and w (weight; 1 for NONE) of loops first .. first + n - 1 in the order
 * they were added.  One small launch; no step, nothing changes; a sub-range equals the slice of the full result byte for byte.  Only the variances of `options` are
 * checked (NULL = the defaults).  LILI_E_ARG, outputs untouched: a null pointer, n < 1, a range outside the graph's loops, a variance that is not positive and finite. */
#define LILI_PG_LOSS_NONE 0
#define LILI_PG_LOSS_HUBER 1
#define LILI_PG_LOSS_CAUCHY 2
#define LILI_PG_LOSS_GEMAN_MCCLURE 3
int lili_pose_graph_add_loop_robust(lili_ctx* ctx, int from, int to, const double meas[7], const double var[6], int loss, double scale);
int lili_pose_graph_loop_status(lili_ctx* ctx, const lili_pg_options* options, int first, int n, double* chi2, double* weight);
/* Levenberg-Marquardt on the same graph, the same elimination and the same robust cost.  Attempt k, k < max_iterations, at the estimate X with the damping lambda
 * (initial_lambda at first):
 *   1. linearise at X; |g|inf <= gradient_tolerance ends the solve (LILI_LM_GRADIENT_TOLERANCE);
 *   2. damp H: diagonal_damping = 0 adds lambda to every diagonal entry of every 6 x 6 diagonal block, diagonal_damping = 1 turns every such entry h into h + lambda h;
 *   3. solve (segments, reduced system, either reduced path); form X (+) delta and its robust cost;
 *   4. new cost <= cost: the step is taken, lambda <- max(lambda / lambda_factor, lambda_lower), then the parameter, function and max-iterations tests of
 *      lili_pose_graph_solve; otherwise X stays, lambda <- lambda * lambda_factor, and lambda > lambda_upper ends the solve (LILI_PG_LAMBDA_LIMIT).  A non-positive
 *      pivot anywhere is a rejected attempt (as GTSAM treats an indeterminate system), never LILI_LM_NUMERICAL_FAILURE; its cost[k] is the unchanged cost and its
 *      step_inf[k] is 0.
 * Summary: base.iterations = attempts; base.cost[k], step_inf[k], grad_inf[k] as in lili_pg_summary; lambda[k] = the lambda attempt k was solved with; accepted[k] = 0 / 1;
 * base.final_cost and the estimates are those of the last accepted attempt; final_lambda = lambda after the last decision.  Every launch of every attempt is enqueued
 * up front, the device decides each attempt, one synchronisation, one read-back; no atomics, every sum in a fixed order: the same graph and options give the same
 * bytes on every run.  The damping exists in this call only: evaluate, marginals and lili_pose_graph_solve are unchanged by it.
 * LILI_E_ARG, everything untouched: what lili_pose_graph_solve refuses, a null summary, an LM option that is not finite, initial_lambda <= 0, lambda_factor <= 1,
 * lambda_lower <= 0, lambda_upper < lambda_lower, diagonal_damping other than 0 or 1.  LILI_E_STATE: an empty graph. */
#define LILI_PG_LAMBDA_LIMIT 8             /* termination: a rejected attempt raised lambda above lambda_upper */
typedef struct lili_pg_lm_options {
    double initial_lambda, lambda_factor, lambda_lower, lambda_upper;
    int32_t diagonal_damping, reserved_;
} lili_pg_lm_options;
typedef struct lili_pg_lm_summary {
    lili_pg_summary base;
    double lambda[LILI_PG_MAX_LOG];
    int32_t accepted[LILI_PG_MAX_LOG];
    int32_t steps_accepted, steps_rejected;
    double final_lambda;
} lili_pg_lm_summary;
/* initial_lambda 1e-5, lambda_factor 10, lambda_lower 1e-10, lambda_upper 1e8, diagonal_damping 0 */
void lili_pg_lm_default_options(lili_pg_lm_options* opt);
int lili_pose_graph_solve_lm(lili_ctx* ctx, const lili_pg_options* options, const lili_pg_lm_options* lm_options, lili_pg_lm_summary* summary);
/* Marginal covariances (gtsam: marginalCovariance / jointMarginalCovariance).  Sigma = H^-1 with H = J^T J of the graph as it is, linearised at the current
 * estimates: the matrix whose blocks lili_pose_graph_evaluate returns.  Only the variances of `options` are read (NULL = the defaults).  No step is taken: estimates
 * and measurements are untouched, and a following solve gives the bytes it would have given without the call.  A block is a row-major 6 x 6 in the node's own tangent
 * (omega, v), rotation first, under X (+) xi above — gtsam::Pose3's convention, the one prior_var / odom_var are expressed in.
 *   cov   (n x 36):        Sigma(i, i), i = first .. first + n - 1; n may be 0 with cov NULL.  A sub-range equals the slice of the full result bit for bit.
 *   cross (n_pairs x 36):  Sigma(i, j) of pairs[2 k], pairs[2 k + 1], rows: node i, columns: node j; n_pairs <= LILI_PG_MAX_PAIRS, NULL / 0 for none.  A pair may
 *                          repeat, take either order (the two blocks are transposes bit for bit) and have i == j (the diagonal block).
 *   info  (optional):      status 0 or LILI_LM_NUMERICAL_FAILURE, the graph's sizes, the reduced system's unknowns, the device time of the call's launches.
 * The call repeats the front half of a solve iteration — linearise, assemble, eliminate the segments, assemble and factor the reduced system over the separators,
 * whatever |g|inf is — and adds the inverse side: the reduced inverse S^-1 (one workgroup per separator: six unit columns through L and L^T, tile by tile; only its
 * lower triangle is kept and read), then per segment, last node first, W = -L_II^-T Y_E, the diagonal blocks P of the segment's own inverse, and
 * Sigma(i, i) = P_i + W_i Sigma_sep W_i^T with Sigma_sep the joint block of the segment's two separators; a separator's block is its block of S^-1; a pair is
 * W_i Sigma_sep(i),sep(j) W_j^T, plus a substitution along the segment when both nodes are interior nodes of one segment.  Every launch is enqueued up front, one
 * synchronisation, outputs through page-locked staging; no atomics, every sum in a fixed order: the same graph gives the same bytes on every run, and a graph of
 * <= 768 reduced unknowns the same bytes whatever "pose_graph_max_loops" is.  Memory, allocated by the first call: a second dense array of the reduced system's size
 * (8 (6 K)^2 bytes: 4.7 MB at 32 loops, 1.3 GB at 1024 loops), 144 doubles per node and the outputs.
 * LILI_E_ARG, nothing written: a null pointer where entries are expected, a range or an id outside the graph, n < 0, n_pairs < 0 or > LILI_PG_MAX_PAIRS, n == 0
 * together with n_pairs == 0, a variance that is not positive and finite.  LILI_E_STATE: an empty graph.  A non-positive pivot (H is not positive definite in
 * double precision): info->status = LILI_LM_NUMERICAL_FAILURE, LILI_E_NUMERIC, cov and cross untouched. */
#define LILI_PG_MAX_PAIRS 4096
typedef struct lili_pg_marginals_info {
    int32_t status;            /* 0, or LILI_LM_NUMERICAL_FAILURE (a non-positive pivot: no output written) */
    int32_t n_nodes, n_loops, reduced_unknowns;
    float   kernel_ms;         /* device time of this call's launches */
    int32_t reserved_;
} lili_pg_marginals_info;
int lili_pose_graph_marginals(lili_ctx* ctx, const lili_pg_options* options, int first, int n, double* cov, const int32_t* pairs, int n_pairs, double* cross,
                              lili_pg_marginals_info* info);
/* First-order covariance of between(X_i, X_j) in its own tangent, host side, no context:
 * J_a Sigma_ii J_a^T + J_a Sigma_ij J_b^T + J_b Sigma_ij^T J_a^T + J_b Sigma_jj J_b^T with the between-factor's Jacobians at Z = between(X_i, X_j) (zero residual):
 * J_b = I, J_a = [-R_Z^T, 0; R_Z^T [t_Z]x, -R_Z^T].  cov_ij = Sigma(i, j), rows: node i.  On a zero-residual chain the result for (i, i + 1) is diag(odom_var).
 * LILI_E_ARG (cov_rel untouched): a null pointer, a non-finite input, a quaternion more than 1e-6 from unit norm. */
int lili_pose_relative_covariance(const double pose_i[7], const double pose_j[7], const double cov_ii[36], const double cov_jj[36], const double cov_ij[36],
                                  double cov_rel[36]);
/* The loop factor's measurement (L:2587-2615), host side, no context: T_icp (row-major 4 x 4) corrects the latest keyframe's pose, meas = between(T_icp o
 * pose_latest, pose_closest) with both quaternions normalised.  LILI_E_ARG: a null pointer, a non-finite input, a zero quaternion. */
int lili_loop_measurement(const double T_icp[16], const double pose_latest[7], const double pose_closest[7], double meas[7]);
/* correctPoses (L:2177-2311) statement by statement on host arrays, no context.  In: solution (n_frames x 7, p then q: the solved nodes),
 * keyframe_id_in_frame (n_keyframes), slide_window_width (>= 2), f32_positions (as lili_local_walk: positions go through pcl's floats).  In / out: abs_poses
 * (n_abs x 7 in the reference's layout q (w, x, y, z) then p; the window's tail is re-chained from its own relative transforms), keyframe_poses (n_keyframes x 7,
 * p then q: pose_cloud_frame / pose_info_cloud_frame).  Out: frame_poses (n_frames x 7, p then q: pose_each_frame / pose_info_each_frame), last_pose (7, the
 * abs_poses layout), select_pose (3).  Rs / Ps of the window follow from abs_poses and are the caller's.  The text's index arithmetic is kept; LILI_E_ARG (nothing
 * written) where it would leave an array: a null pointer, slide_window_width < 2 or > n_abs or > n_keyframes, n_abs > n_keyframes + 1,
 * n_keyframes - slide_window_width + 2 > n_abs, a keyframe id outside 0 .. n_frames - 1, a non-finite input. */
int lili_correct_poses(const double* solution, int n_frames, const int32_t* keyframe_id_in_frame, int n_keyframes, int slide_window_width, int f32_positions,
                       double* abs_poses, int n_abs, double* frame_poses, double* keyframe_poses, double last_pose[7], double select_pose[3]);

/* ---- callers / data formats either side of the path ------------------------- */

/* Livox CustomMsg points -> the PointXYZINormal cloud the Livox extractor consumes; replaces livoxLidarHandler
 * (L/src/FormatConvert.cpp:11-35).  `points` = point_num records of the serialised livox_ros_driver/CustomPoint
 * (little endian: uint32 offset_time, float32 x, y, z, uint8 reflectivity, tag, line; `stride` >= 19 bytes).
 * Output: pcl::PointXYZINormal records (48 B: x y z 1.0 | normal 0 0 0 0 | intensity curvature 0 0) with
 *   intensity = line + 0.1 * (float(offset_time) / float(offset_time of the LAST point)),  curvature = 0.1 * reflectivity
 * (float / double expression widths of the reference).  in_mem / out_mem: LILI_MEM_HOST or LILI_MEM_DEVICE; the output
 * can be handed to lili_extract_livox as {data = out, stride = 48, aux_offset = 32, curvature_offset = 36}.  Blocking for
 * host memory, asynchronous on the context's stream when both sides are device memory. */
int lili_livox_custom_to_cloud(lili_ctx* ctx, const void* points, size_t point_num, size_t stride, int in_mem, void* out, int out_mem);

/* Gyro integration over one scan, host side (L/src/Preprocessing.cpp:129-171 processIMU / solveRotation, 176-191
 * imuHandler state, 232-234 NaN reset, 403 identity reset; deltaQ = utils/math_tools.h:125-138): mid-point rule on the
 * un-normalised small-angle quaternion, linear interpolation of the rate at the scan boundary.  The caller keeps the IMU
 * samples (stamps[n] seconds, gyr[n*3] rad/s, in arrival order, n may grow between calls) and one lili_imu_state per
 * sensor; q_out (w,x,y,z) is the q_imu argument of lili_extract_livox / lili_extract_rot for the scan ending at
 * t_scan_next.  Zero-initialise the state (or lili_imu_reset) before the first call. */
typedef struct lili_imu_state {
    int64_t idx;        /* idx_imu: first sample not yet consumed */
    double t_cur;       /* current_time_imu (< 0: unset) */
    double gyr0[3];     /* gyr_0 */
    int32_t first;      /* first_imu seen */
    int32_t reserved;
} lili_imu_state;
void lili_imu_reset(lili_imu_state* st);
int lili_imu_integrate(lili_imu_state* st, const double* stamps, const double* gyr, size_t n, double t_scan_next, double q_out[4]);

/* Lidar contribution of one keyframe to MarginalizationInfo's A, b (L/src/MarginalizationFactor.cpp:3-29, 151-174):
 * the reference evaluates every lidar residual again and adds J_i^T J_j / J_i^T r per block with rightCols(3) of the
 * 1x4 quaternion Jacobian; the same sums are rows / columns {0,1,2} (t) and {4,5,6} (q: x,y,z) of the Gram record
 * and its column 7.  A is a dense pos x pos matrix with leading dimension ld (symmetric: both triangles are
 * updated, so row- and column-major callers are served alike), b has pos entries; idx_t / idx_q are
 * parameter_block_idx of the keyframe's translation / rotation block.  Host function. */
int lili_marg_add_lidar(const double gram[64], double* A, size_t ld, double* b, size_t pos, size_t idx_t, size_t idx_q);

/* ---- loop-closure registration (performLoopClosure, L/src/BackendFusion.cpp:2552-2642) ---------------
 * The submaps of detectLoopClosure (L:2423-2550) are assembled on the device and registered by the restatement of
 * pcl::IterativeClosestPoint's default pipeline (no rejectors, TransformationEstimationSVD, DefaultConvergenceCriteria) in
 * f64.  The pose-graph update (iSAM2) stays with the caller.  A context holds one source and one target cloud of its own:
 * nothing here touches the matcher's maps and slots, the local map or the voxel filter's state. */
enum { LILI_LOOP_SOURCE = 0, LILI_LOOP_TARGET = 1 };
/* pcl::registration::DefaultConvergenceCriteria::ConvergenceState, same order */
enum { LILI_ICP_NOT_CONVERGED = 0, LILI_ICP_ITERATIONS = 1, LILI_ICP_TRANSFORM = 2, LILI_ICP_ABS_MSE = 3,
       LILI_ICP_REL_MSE = 4, LILI_ICP_NO_CORRESPONDENCES = 5 };
typedef struct lili_icp_params {
    double max_corr_dist;              /* 30 (setMaxCorrespondenceDistance): a correspondence is rejected when d2 > max_corr_dist^2 */
    int32_t max_iterations;            /* 100 (>= 1) */
    int32_t reserved_;
    double transformation_epsilon;     /* 1e-6: |t_inc|^2 <= eps and cos(angle of R_inc) >= 1 - eps */
    double euclidean_fitness_epsilon;  /* 1e-6: |mse - prev| / prev */
} lili_icp_params;
#define LILI_ICP_MAX_LOG 128
typedef struct lili_icp_iteration {
    double mse;                        /* mean d2 of the iteration's correspondences (before its update) */
    double cos_angle, translation_sqr; /* of the iteration's increment */
    int32_t n_corr, state;             /* correspondences; LILI_ICP_* after the convergence check */
} lili_icp_iteration;
typedef struct lili_icp_result {
    double transform[16];              /* final_transformation_, row-major, f64 */
    int32_t converged, state, iterations, n_logged;
    double fitness;                    /* getFitnessScore() (max_range = DBL_MAX); DBL_MAX if no source point has a finite distance */
    double stage_us[4];                /* [0] wall time of the call (us), [1] host synchronisations, [2] iterations enqueued (a batch may run past the end), [3] spare */
    lili_icp_iteration it[LILI_ICP_MAX_LOG];
} lili_icp_result;
void lili_icp_default_params(lili_icp_params* p);
/* transformCloud of cloud i by (t + 3i, q + 4i) (the LiDAR pose q_po*q_bl, q_po*t_bl + t_po), concatenated in the given order
 * (per keyframe edge then surf, keyframes ascending: L:2476-2493, 2502-2521), then VoxelGrid(leaf) (leaf <= 0: none) -> the
 * context's source or target (`which`).  The clouds may be host, page-locked host or device memory.  The target is indexed
 * for the search.  n_raw / n_ds (optional): points before / after the filter.  Blocking. */
int lili_loop_cloud(lili_ctx* ctx, int which, const lili_cloud* clouds, int n_clouds, const double* t, const double* q, float leaf, int64_t* n_raw, int64_t* n_ds);
/* an already assembled cloud as the source / target (copied; the target is indexed).  Blocking. */
int lili_icp_set_cloud(lili_ctx* ctx, int which, const lili_cloud* cloud);
/* the context's source / target as float4 rows (x, y, z, aux) */
int lili_icp_get_cloud(lili_ctx* ctx, int which, lili_feature_out* out);
/* align(source -> target) from `guess` (row-major 4x4, NULL = identity).  LILI_E_STATE if a cloud is missing.  Blocking. */
int lili_icp_align(lili_ctx* ctx, const lili_icp_params* p, const double guess[16], lili_icp_result* res);
/* mean exact 1-NN d2 of the source under T over the points with d2 <= max_range (getFitnessScore(max_range)); DBL_MAX and
 * n_used = 0 if there is none.  Blocking. */
int lili_icp_fitness(lili_ctx* ctx, const double T[16], double max_range, double* fitness, int64_t* n_used);
/* the correspondences of the last iteration of the last align, per source point: target index (-1: rejected or none) and d2
 * (+inf where rejected).  capacity = entries the arrays hold (either may be NULL).  Blocking. */
int lili_icp_get_correspondences(lili_ctx* ctx, size_t capacity, int32_t* target_idx, float* d2);

/* ---- keyframe archive and global map (saveKeyFramesAndFactors L/src/BackendFusion.cpp:1494-1514, correctPoses L:2177-2311,
 * publishCompleteMap L:2644-2685 and the PCD save L:2697-2723) -------------------------------------------
 * Every keyframe's clouds stay in device memory as float4 rows (x, y, z, aux) in the LiDAR frame, as pushed, with the
 * keyframe's body pose and time on the host; a pose change moves no point.  Storage is a pool of large slabs ("archive_slab_mb")
 * that never move: a view stays valid until lili_archive_reset / lili_ctx_destroy.  Nothing is ever evicted.  The archive and
 * the global map have buffers of their own: the matcher, the local map, the voxel filter's state and the loop-closure clouds
 * (other than through lili_loop_cloud_archive) are untouched.  Argument errors return LILI_E_ARG with the archive as it was. */
enum { LILI_ARCHIVE_EDGE = 0, LILI_ARCHIVE_SURF = 1, LILI_ARCHIVE_FULL = 2 };
int lili_archive_reset(lili_ctx* ctx);
/* body -> LiDAR extrinsic (default identity): a keyframe's map pose is (q_po * q_bl, q_po * t_bl + t_po), f64 on the host */
int lili_archive_set_extrinsic(lili_ctx* ctx, const double t_bl[3], const double q_bl[4]);
/* Appends a keyframe; *id (optional) = number of keyframes before the call.  Any cloud may be NULL (kind absent) and may lie in
 * host, page-locked host or device memory with any stride / aux offset (aux absent: 0).  Fails with LILI_E_NOMEM, archive
 * untouched, if the pool would exceed "archive_max_mb".  Blocking. */
int lili_archive_push(lili_ctx* ctx, const lili_cloud* edge, const lili_cloud* surf, const lili_cloud* full, double time,
                      const double t_po[3], const double q_po[4], int* id);
/* the same with edge / surf = the QUERIES of matcher slot `slot` (what lili_s2m_set_queries or lili_backend_keyframe_prepare
 * left there), copied device to device on the context's stream; a kind without queries is absent */
int lili_archive_push_slot(lili_ctx* ctx, int slot, const lili_cloud* full, double time, const double t_po[3], const double q_po[4], int* id);
/* keyframes first .. first + n - 1 take new body poses (t_po: 3 n doubles, q_po: 4 n doubles w x y z) */
int lili_archive_set_poses(lili_ctx* ctx, int first, int n, const double* t_po, const double* q_po);
/* n_points: edge, surf, full; bytes_used: device memory of the slab pool (all pointers optional) */
int lili_archive_info(lili_ctx* ctx, int* n_keyframes, int64_t n_points[3], int64_t* bytes_used);
/* body pose and time of keyframe id (any pointer may be NULL) */
int lili_archive_pose(lili_ctx* ctx, int id, double t_po[3], double q_po[4], double* time);
/* the rows of keyframe id / kind; out->count = the cloud's size (0: absent or empty).  Blocking. */
int lili_archive_get(lili_ctx* ctx, int id, int kind, lili_feature_out* out);
/* LILI_MEM_DEVICE view (stride 16, aux offset 12) of the rows, complete when the call returns */
int lili_archive_view(lili_ctx* ctx, int id, int kind, lili_cloud* view);
/* lili_loop_cloud with clouds and poses from the archive: per id, in the order given, edge then surf, at the keyframe's map pose.
 * Same gather, filter and buffers: bit for bit the submap lili_loop_cloud makes of the same clouds and poses. */
int lili_loop_cloud_archive(lili_ctx* ctx, int which, const int* ids, int n_ids, float leaf, int64_t* n_raw, int64_t* n_ds);
/* detectLoopClosure's candidate selection (L:2431-2473, R:2240-2263), host code without a context: the keyframes with f32
 * d2 = (dx dx + dy dy) + dz dz < (float)(radius radius) of select_pose in ascending d2 (ties: smaller index); his = the first whose
 * |time - t_now| exceeds global_thres; variant 0 (Livox): failing that the one with the largest |time - t_now| inside
 * (local_thres, global_thres); variant 1 (ROT): none, and none either within 0.2 s of time_last_loop.  Returns 1 and fills
 * latest = n - slide_window_width and his, 0 if there is no candidate, LILI_E_ARG on a bad argument. */
int lili_loop_detect(const float* positions, const double* times, int n, const float select_pose[3], double t_now, int variant, double radius,
                     double local_thres, double global_thres, double time_last_loop, int slide_window_width, int* latest, int* his);
/* publishCompleteMap: keyframes 0, interval, 2 interval, ... of `kind` at their current map poses -> VoxelGrid(leaf), on the
 * device.  The result equals lili_voxel_filter(leaf) of the concatenation, in keyframe order, of the selected clouds placed
 * as lili_loop_cloud places them (centroids, counts and order, bit for bit), but is kept as an accumulating table
 * (voxel key, running f32 sum, count): a call folds only the keyframes the table does not hold yet (`incremental`) when the
 * table was built with the same kind, interval, leaf and extrinsic and every keyframe it holds still has the map pose, bit
 * for bit, it was folded at; otherwise it starts from an empty table (`rebuild`).  Points are folded in batches of
 * "global_map_batch_points".  PCL's int32 voxel-index guard applies to everything folded: beyond it the call fails with
 * lili_voxel_filter's error and the next call rebuilds; so does a point farther than 2^20 voxels from the origin.
 * n_raw = points folded in all (non-finite ones included, which the filter drops), n_map = voxels.  An empty selection
 * gives an empty map.  Blocking. */
int lili_global_map(lili_ctx* ctx, int kind, int interval, float leaf, int64_t* n_raw, int64_t* n_map);
/* the map of the last successful lili_global_map: rows (x, y, z, aux) in voxel-index order; `out` may be device memory;
 * counts (optional, host or device, out->capacity entries): members per voxel.  Blocking. */
int lili_global_map_get(lili_ctx* ctx, lili_feature_out* out, int32_t* counts);
/* calls served incrementally / from an empty table so far, and the points the last call folded */
int lili_global_map_stats(lili_ctx* ctx, int32_t* incremental, int32_t* rebuilds, int64_t* points_folded_last);
/* device memory of the global map: the table and the work buffers of a batch (bytes) */
int lili_global_map_info(lili_ctx* ctx, int64_t* table_bytes, int64_t* work_bytes);
/* The part of the map inside a box: the voxels whose index lies in [floorf(lo * inv_leaf), floorf(hi * inv_leaf)] on every axis — inv_leaf the
 * table's own f32 1.0f / leaf, the product rounded to f32, the index offset by 2^20 and clipped to [0, 2^21 - 1] as the table's keys are formed —, that is the
 * voxels a point of the closed box would fall into.  Rows (the centroid bits lili_global_map_get gives) and counts come out in table order (ascending key).
 * out->count = *n = the voxels in the box; the first min(n, out->capacity) rows and counts are copied (capacity 0: only counted); `out` and `counts` (optional)
 * may be host or device memory; +-inf is allowed on any face.  The cost follows the box, not the table: one bisection pair per (k, j) row of the box (k clipped to
 * the table's own range), a scan of the run lengths and a gather; no floating-point arithmetic and no atomics — the same bytes on every run.
 * LILI_E_ARG: lo > hi on an axis, a NaN, or more than 2^24 (k, j) rows after clipping (the message names the count); LILI_E_STATE: no successful
 * lili_global_map / lili_global_map_import.  Blocking (one read-back: the count). */
int lili_global_map_crop(lili_ctx* ctx, const float lo[3], const float hi[3], lili_feature_out* out, int32_t* counts, int64_t* n);
/* The table itself — per voxel the key ((k << 42) | (j << 21) | i, each index offset by 2^20), the running f32 sum (4 floats) and the count, in ascending key order —
 * and the leaf and kind it was built with: what another context needs to hand back the same centroid bits (centroids alone would not do).  *n = voxels; the first
 * min(n, capacity) entries are copied (host or device memory; any array may be NULL).  LILI_E_STATE without a map.  Blocking. */
int lili_global_map_export(lili_ctx* ctx, int64_t capacity, uint64_t* keys, float* sums, int32_t* counts, int64_t* n, float* leaf, int* kind);
/* An exported table into this context: uploaded, validated on the device (keys strictly ascending, every index below 2^21, counts >= 1: otherwise LILI_E_ARG and an
 * EMPTY table) and its centroids computed as lili_global_map computes them.  An imported table serves lili_global_map_get, _crop, _export and _info.  The list of
 * keyframes a table was folded from does NOT travel with it: the next lili_global_map does not extend an imported table, it starts from an empty one and folds
 * this context's archive (a rebuild, as after a failed call).  Blocking. */
int lili_global_map_import(lili_ctx* ctx, float leaf, int kind, int64_t n, const uint64_t* keys, const float* sums, const int32_t* counts);

/* ---- place recognition: polar descriptors over the archive (lili_place.hip) -------------------------------
 * Appearance-based loop candidates in the manner of Scan Context (Kim & Kim, IROS 2018): per keyframe an n_sector x n_ring image
 * of maximum heights, compared column-wise under every circular shift.  Not in the reference, whose detectLoopClosure searches
 * keyframe POSITIONS (lili_loop_detect) and so finds a loop only while the drift is below its radius.
 * The descriptor, exactly (all f32, every operation rounded on its own).  A point with a non-finite coordinate is skipped;
 * r2 = x x + y y; a point with r2 > max_radius max_radius is skipped.  Ring = number of k in 1 .. n_ring - 1 with r2 > b_k b_k,
 * b_k = (max_radius (float)k) / (float)n_ring (a point on a boundary belongs to the inner ring).  Quadrant q: x >= 0, y >= 0 -> 0;
 * x < 0, y >= 0 -> 1; x < 0, y < 0 -> 2; otherwise 3.  (u, v) = the point turned back by q quarter turns: (x, y), (y, -x), (-x, -y),
 * (-y, x).  j = number of m in 1 .. n_sector / 4 - 1 with v C_m >= u S_m, C_m / S_m = cos / sin(2 pi m / n_sector) computed in f64 and
 * rounded to f32.  Sector = q n_sector / 4 + j.  Cell (sector, ring) = the maximum of z + lidar_height over its points, 0 without
 * one; stored sector-major: desc[sector * n_ring + ring].  A maximum does not depend on order: the descriptor is the same bytes
 * on every run and for every split of the work (integer atomics on an order-preserving word; no floating-point atomics).
 * Descriptors live in a buffer of their own that grows by half; it is NOT counted against "archive_max_mb". */
typedef struct lili_place_params {
    int32_t n_ring;        /* 1 .. 32, default 20 */
    int32_t n_sector;      /* a multiple of 4 in 4 .. 64, default 60 */
    float max_radius;      /* default 80 */
    float lidar_height;    /* default 2 */
    int32_t kind;          /* LILI_ARCHIVE_*: the cloud described, default LILI_ARCHIVE_FULL */
    int32_t reserved_;
} lili_place_params;
typedef struct lili_place_query {
    int32_t id;            /* an archived, described keyframe, or -1: `desc` */
    int32_t max_id;        /* candidates c <= max_id only */
    const float* desc;     /* id = -1: n_sector * n_ring floats on the host (the parameters of the last lili_place_update) */
    double time;           /* the query's time */
    double min_time_gap;   /* candidates with |time_c - time| > min_time_gap only (time_c: the archive's) */
} lili_place_query;
typedef struct lili_place_match { int32_t id, shift; double distance; } lili_place_match;
void lili_place_default_params(lili_place_params* p);
/* the tables the kernels decide by, host code without a context: ring_r2[k] = b_k b_k for k < n_ring, sec_cos[m] / sec_sin[m] = C_m /
 * S_m for m < n_sector / 4, zeros behind them.  LILI_E_ARG on parameters outside the ranges above. */
int lili_place_layout(const lili_place_params* params, float ring_r2[32], float sec_cos[16], float sec_sin[16]);
/* Describes every archived keyframe that has no descriptor yet from its cloud of params->kind (absent: all zeros) — one launch
 * over a table of the keyframes' rows, however many there are.  A descriptor depends on the cloud alone: lili_archive_set_poses
 * and _set_extrinsic invalidate nothing; lili_archive_reset drops all descriptors; other `params` than the last call's rebuild all.
 * (In a submap setting — lili_place_set_submap below — a descriptor also depends on its window's poses: see the rebuild rule there.)
 * n_built (optional): descriptors built (or rebuilt) by this call.  Blocking. */
int lili_place_update(lili_ctx* ctx, const lili_place_params* params, int* n_built);
/* the descriptor of any cloud (host, page-locked host or device rows, any stride; lili_archive_push's checks) into
 * desc[n_sector * n_ring] on the host: bit for bit what lili_place_update builds from the same rows.  Blocking. */
int lili_place_describe(lili_ctx* ctx, const lili_cloud* cloud, const lili_place_params* params, float* desc);
/* keyframe id's descriptor into desc[n_sector * n_ring] on the host.  Blocking. */
int lili_place_get(lili_ctx* ctx, int id, float* desc);
/* described keyframes, the parameters they were built with (the defaults before the first update), device bytes of the store */
int lili_place_info(lili_ctx* ctx, int* n_described, lili_place_params* params, int64_t* bytes);
/* The k best candidates of each of n_q queries (1 <= n_q <= 64, 1 <= k <= 16) among ALL described keyframes at ALL shifts: no
 * pre-selection, the exact minimum.  Candidate c is eligible iff c <= max_id, |time_c - time| > min_time_gap, c is not the query
 * itself and c has a descriptor.  With unit columns a_j = A_j / |A_j| (f64, from the f32 cells),
 *   d(s) = 1 - mean over { j : |A_j| > 0 and |B_(j+s) mod n_sector| > 0 } of a_j . b_(j+s),     +inf when the set is empty;
 * a pair's distance = min_s d(s), its shift = the smallest s that attains it.  Column j of the query matches column j + s of the
 * candidate: the candidate's scan is the query's turned by +s sectors about the LiDAR z axis.  matches[q * k + i], i < n_found[q]
 * <= k, ascend by (distance, id); pairs at +inf are never reported.  A pair's distance and shift depend on the two descriptors
 * alone — not on the candidate's place in the archive nor on the rest of the batch — and are the same bytes on every run.
 * Without a described keyframe every n_found is 0.  One synchronisation, one read-back.  Blocking. */
int lili_place_search(lili_ctx* ctx, const lili_place_query* queries, int n_q, int k, lili_place_match* matches, int* n_found);
/* The ICP's initial guess from a match, host code without a context: poses are LiDAR map poses (p then q w x y z; the archive's
 * (q_po q_bl, q_po t_bl + t_po)), T = M_dst Rz(2 pi shift / n_sector) M_src^-1 row-major — the transform that puts the source
 * keyframe on the candidate with the matched yaw, as lili_icp_align's `guess` wants it.  LILI_E_ARG: a null pointer, a non-finite
 * input, a zero quaternion, n_sector < 1. */
int lili_place_guess(const double pose_src[7], const double pose_dst[7], int shift, int n_sector, double T[16]);

/* ---- levelled submap descriptors (a narrow-field LiDAR sees a wedge: one keyframe does not describe a place) -------------
 * With a setting other than all zeros a keyframe's descriptor is the image of the rows of a WINDOW of keyframes, placed in
 * the frame F_i of the keyframe it belongs to.  All zeros (the default): today's descriptor of the keyframe's own rows, byte for byte.
 * Window of keyframe i in an archive of n: max(0, i - back) .. min(n - 1, i + fwd), by index (not by time).
 * Frame F_i from the keyframe's LiDAR map pose (q_i, t_i) (the archive's (q_po q_bl, q_po t_bl + t_po)), host f64 (lili_place_frame):
 *   level = 0: F_i = (q_i, t_i) as they are.
 *   level = 1: origin t_i, z = the map's z (the back end's gravity is (0, 0, 9.805) in the map frame), x = the horizontal projection of
 *     the LiDAR's x axis.  (w, x, y, z) = q_i / sqrt(((w w + x x) + y y) + z z); R00 = 1 - 2 (y y + z z); R10 = 2 (x y + w z);
 *     h = sqrt(R00 R00 + R10 R10); h < 1e-9 (x axis vertical): c = 1, s = 0; otherwise c = R00 / h clamped to [-1, 1], s = R10 / h;
 *     F_i.q = (sqrt((1 + c) / 2), 0, 0, sqrt((1 - c) / 2)), the last negated iff s < 0.  At c = -1 (a half turn) s is +-0 and the
 *     comparison s < 0 is false for both zeros: the frame is (0, 0, 0, +1).
 * Placement of member k (lili_place_relative, host f64): f = F_i.q / |F_i.q|, f' = its conjugate, p = q_k / |q_k|,
 *   q_rel = f' (x) p (Hamilton product, the sums left to right), t_rel = f' . (t_k - t_i) as v + w (2 u x v) + u x (2 u x v).
 *   On the device a row becomes (float)(q_rel . (double)p + t_rel) — the ONE transform every kernel places a keyframe with — and
 *   is then binned exactly as above.  With level = 0 the centre keyframe's own rows are read untransformed (its segment carries
 *   an identity flag): back = fwd = level = 0 is today's descriptor.  A maximum is order-free: the bytes do not depend on the run,
 *   on the split into tiles or on the batches of an update.
 * Rebuild rule: a descriptor remembers its BUILD KEY, the list of (member id, identity flag, q_rel, t_rel) it was built from.
 *   lili_place_update builds every descriptor without a key and rebuilds every descriptor whose key, recomputed from the archive
 *   as it is now, differs in any byte: a new successor inside a window, lili_archive_set_poses, lili_archive_set_extrinsic.  In the
 *   all-zero setting the key never changes and nothing is rebuilt.  n_built counts built plus rebuilt descriptors. */
#define LILI_PLACE_TILE_ROWS 2048      /* rows of a descriptor's concatenation one workgroup bins into its LDS image */
typedef struct lili_place_submap {
    int32_t back;          /* 0 .. 64 predecessors */
    int32_t fwd;           /* 0 .. 16 successors */
    int32_t level;         /* 0 or 1 */
    int32_t reserved_;
} lili_place_submap;
/* another setting than the current one drops every descriptor; NULL = all zeros.  LILI_E_ARG (state untouched) outside the ranges. */
int lili_place_set_submap(lili_ctx* ctx, const lili_place_submap* s);
int lili_place_get_submap(lili_ctx* ctx, lili_place_submap* s);
/* the window keyframe id's descriptor was built from (id .. id in the all-zero setting).  LILI_E_ARG: id has no descriptor. */
int lili_place_window(lili_ctx* ctx, int id, int* first, int* last);
/* F of a LiDAR map pose (p then q w x y z), host code without a context.  LILI_E_ARG: null, non-finite, zero quaternion, level not 0 / 1. */
int lili_place_frame(const double pose[7], int level, double frame[7]);
/* (q_rel, t_rel) of a member at `pose` in `frame`, host code without a context.  LILI_E_ARG: null, non-finite, a zero quaternion. */
int lili_place_relative(const double frame[7], const double pose[7], double q_rel[4], double t_rel[3]);
/* The descriptor of n clouds (1 <= n <= 81; host, page-locked or device rows, any stride; lili_archive_push's checks) placed at
 * q_rel[4 i ..], t_rel[3 i ..] into desc[n_sector * n_ring] on the host — the kernel and the bytes of the archive path.  A cloud whose
 * q_rel is four zeros is read untransformed (the identity flag); q_rel = t_rel = NULL: every cloud is.  Blocking. */
int lili_place_describe_submap(lili_ctx* ctx, const lili_cloud* clouds, int n, const double* q_rel, const double* t_rel, const lili_place_params* params,
                               float* desc);

#ifdef __cplusplus
}
#endif
#endif /* LILI_HIP_H */
