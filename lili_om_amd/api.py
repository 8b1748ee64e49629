"""ctypes binding of include/lili_hip.h (liblili_hip.so) plus a thin host-side mirror of the reference's
matcher interface.  There is NO fallback: if the HIP library is missing or no gfx950 device is present
every entry point raises.  Nothing here imports oracle/.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblili_hip.so")

OK = 0
KIND_SURF, KIND_EDGE = 0, 1
MASK_SURF, MASK_EDGE = 1, 2
VARIANT_LIVOX, VARIANT_ROT, VARIANT_FRONTEND = 0, 1, 2
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
MEM_HOST, MEM_DEVICE = 0, 1
MAX_SLOTS = 8
GRAM_DOUBLES = 72


class LiliError(RuntimeError):
    pass


class Cloud(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n", C.c_size_t), ("stride", C.c_size_t), ("aux_offset", C.c_int), ("mem", C.c_int)]


class MapIndexInfo(C.Structure):
    """lili_map_index_info: the scalars of an index as lili_map_debug_index reports them."""
    _fields_ = [(k, C.c_int32) for k in ("nx", "ny", "nz", "bx0", "by0", "bz0", "bnx", "bny", "bnz", "n_points", "reach", "has_aux", "has_super", "narrow",
                                         "narrow_overflows", "scan_fallbacks")] + \
               [(k, C.c_double) for k in ("ox", "oy", "oz", "inv_cell", "cell")] + [("n_cells", C.c_int64), ("n_super", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FeatureOut(C.Structure):
    _fields_ = [("data", C.c_void_p), ("capacity", C.c_size_t), ("stride", C.c_size_t), ("mem", C.c_int), ("count", C.c_size_t)]


class RotParams(C.Structure):
    _fields_ = [("n_scans", C.c_int), ("ds_rate", C.c_int), ("ds_v", C.c_float), ("near_range", C.c_float)]


class LivoxParams(C.Structure):
    _fields_ = [("surf_thres", C.c_double), ("edge_thres", C.c_double), ("near_range", C.c_float)]


class FrontendOptions(C.Structure):
    _fields_ = [("leaf_query", C.c_float), ("leaf_map", C.c_float), ("width", C.c_int), ("n_iters", C.c_int), ("slot", C.c_int), ("want_timing", C.c_int), ("flags", C.c_int)]


FRAME_SELF_MAP, FRAME_PUSH_EMPTY, FRAME_EXTERNAL_MAP, FRAME_EDGES = 1, 2, 4, 8
KF_NO, KF_YES, KF_FIRST = 0, 1, 2


class KfRuleState(C.Structure):
    _fields_ = [("t_last", C.c_double * 3), ("q_last", C.c_double * 4), ("n_frames", C.c_int64), ("kf_num", C.c_int64), ("kf", C.c_int32), ("reserved_", C.c_int32)]


class FrontendResult(C.Structure):
    _fields_ = [("t", C.c_double * 3), ("q", C.c_double * 4), ("gn_status", C.c_int), ("matched", C.c_int), ("n_edge", C.c_int32), ("n_surf", C.c_int32),
                ("n_query", C.c_int32), ("n_map_raw", C.c_int32), ("n_map", C.c_int32), ("stage_us", C.c_double * 8)]


LM_MAX_LOG = 32
LM_TERMINATION = {0: "max_iterations", 1: "gradient_tolerance", 2: "parameter_tolerance", 3: "function_tolerance", 4: "stalled", 5: "numerical_failure", 6: "min_radius"}


class BackendOptions(C.Structure):
    _fields_ = [("leaf_surf", C.c_float), ("leaf_edge", C.c_float), ("leaf_surf_map", C.c_float), ("leaf_edge_map", C.c_float), ("width", C.c_int), ("want_timing", C.c_int), ("join_slot", C.c_int)]


class BackendResult(C.Structure):
    _fields_ = [("n_map_raw", C.c_int32 * 2), ("n_map", C.c_int32 * 2), ("n_query", C.c_int32 * 2), ("associated", C.c_int32), ("stage_us", C.c_double * 8)]


class LmOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved_", C.c_int32), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double)]


class LmIteration(C.Structure):
    _fields_ = [("cost", C.c_double), ("new_cost", C.c_double), ("rho", C.c_double), ("radius", C.c_double), ("step_norm", C.c_double),
                ("accepted", C.c_int32), ("iteration", C.c_int32)]


class LmSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("successful_steps", C.c_int32), ("termination", C.c_int32), ("n_logged", C.c_int32),
                ("n_surf", C.c_int32), ("n_edge", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double),
                ("it", LmIteration * LM_MAX_LOG)]

    def as_dict(self):
        return dict(iterations=self.iterations, successful_steps=self.successful_steps, termination=LM_TERMINATION.get(self.termination, self.termination),
                    n_surf=self.n_surf, n_edge=self.n_edge, initial_cost=self.initial_cost, final_cost=self.final_cost, final_radius=self.final_radius,
                    log=[dict(it=e.iteration, cost=e.cost, new_cost=e.new_cost, rho=e.rho, radius=e.radius, step=e.step_norm, accepted=bool(e.accepted))
                         for e in self.it[:self.n_logged]])


class WindowImu(C.Structure):
    _fields_ = [("sum_dt", C.c_double), ("g", C.c_double * 3), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
                ("lin_ba", C.c_double * 3), ("lin_bg", C.c_double * 3), ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225)]


class ImuSegment(C.Structure):
    _fields_ = [("dt", C.POINTER(C.c_double)), ("acc", C.POINTER(C.c_double)), ("gyr", C.POINTER(C.c_double)), ("n", C.c_int32), ("predict", C.c_int32),
                ("acc0", C.c_double * 3), ("gyr0", C.c_double * 3), ("lin_ba", C.c_double * 3), ("lin_bg", C.c_double * 3), ("g", C.c_double * 3),
                ("P0", C.c_double * 3), ("R0", C.c_double * 9), ("V0", C.c_double * 3)]


class ImuPrediction(C.Structure):
    _fields_ = [("P1", C.c_double * 3), ("R1", C.c_double * 9), ("V1", C.c_double * 3)]


class ImuKfState(C.Structure):
    _fields_ = [("idx", C.c_int64), ("t_cur", C.c_double), ("acc0", C.c_double * 3), ("gyr0", C.c_double * 3), ("first", C.c_int32), ("reserved", C.c_int32)]


LOCAL_MAX_FRAMES = 16


class LocalWalk(C.Structure):
    _fields_ = [("stamps", C.POINTER(C.c_double)), ("acc", C.POINTER(C.c_double)), ("gyr", C.POINTER(C.c_double)), ("n_imu", C.c_int64), ("ii0", C.c_int64),
                ("scan_stamps", C.POINTER(C.c_double)), ("P0", C.c_double * 3), ("R0", C.c_double * 9), ("V0", C.c_double * 3), ("g", C.c_double * 3),
                ("left", C.c_double * 7), ("f32_positions", C.c_int32), ("reserved_", C.c_int32)]


class LocalGraphSummary(C.Structure):
    _fields_ = [("lm", LmSummary), ("final_mu", C.c_double), ("dogleg_case", C.c_int32 * LM_MAX_LOG), ("reused", C.c_int32 * LM_MAX_LOG)]

    def as_dict(self):
        d = self.lm.as_dict()
        for e, case, reused in zip(d["log"], self.dogleg_case, self.reused):
            e["case"], e["reused"] = int(case), bool(reused)
        d["final_mu"] = self.final_mu
        return d


PG_MAX_NODES, PG_MAX_LOOPS, PG_SEGMENT, PG_MAX_LOG, PG_COST_INCREASED = 32768, 32, 512, 16, 7
PG_MAX_LOOPS_EXT = 1024      # LILI_PG_MAX_LOOPS_EXT: the largest value of option "pose_graph_max_loops" (default PG_MAX_LOOPS)
PG_MAX_REDUCED = 768         # reduced unknowns (6 per separator) one workgroup factors; beyond, the blocked solve in tiles of PG_REDUCED_TILE (lili_kernels.h: kPgMaxReduced, kPgTile)
PG_REDUCED_TILE = 96


class PgOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved_", C.c_int32), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("prior_var", C.c_double * 6), ("odom_var", C.c_double * 6)]


class PgSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("termination", C.c_int32), ("n_nodes", C.c_int32), ("n_loops", C.c_int32), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("cost", C.c_double * PG_MAX_LOG), ("step_inf", C.c_double * PG_MAX_LOG), ("grad_inf", C.c_double * PG_MAX_LOG)]

    def as_dict(self):
        k = min(self.iterations, PG_MAX_LOG)
        kg = min(self.iterations + (1 if self.termination in (1, 5) else 0), PG_MAX_LOG)      # a solve that ends at a linearisation (gradient, pivot) has one more of them than steps
        return dict(iterations=self.iterations, termination=self.termination, n_nodes=self.n_nodes, n_loops=self.n_loops, initial_cost=self.initial_cost,
                    final_cost=self.final_cost, cost=list(self.cost[:k]), step_inf=list(self.step_inf[:k]), grad_inf=list(self.grad_inf[:kg]))


PG_LOSS_NONE, PG_LOSS_HUBER, PG_LOSS_CAUCHY, PG_LOSS_GEMAN_MCCLURE = 0, 1, 2, 3      # LILI_PG_LOSS_*: the robust loss of a loop factor
PG_LOSSES = {None: PG_LOSS_NONE, "none": PG_LOSS_NONE, "huber": PG_LOSS_HUBER, "cauchy": PG_LOSS_CAUCHY, "geman_mcclure": PG_LOSS_GEMAN_MCCLURE}
PG_LAMBDA_LIMIT = 8          # LILI_PG_LAMBDA_LIMIT: lili_pose_graph_solve_lm ended on a rejected attempt that raised lambda above lambda_upper


class PgLmOptions(C.Structure):
    _fields_ = [("initial_lambda", C.c_double), ("lambda_factor", C.c_double), ("lambda_lower", C.c_double), ("lambda_upper", C.c_double),
                ("diagonal_damping", C.c_int32), ("reserved_", C.c_int32)]


class PgLmSummary(C.Structure):
    _fields_ = [("base", PgSummary), ("lambda_", C.c_double * PG_MAX_LOG), ("accepted", C.c_int32 * PG_MAX_LOG), ("steps_accepted", C.c_int32),
                ("steps_rejected", C.c_int32), ("final_lambda", C.c_double)]

    def as_dict(self):
        d = self.base.as_dict()
        k = min(self.base.iterations, PG_MAX_LOG)
        d["lambda"], d["accepted"] = list(self.lambda_[:k]), [int(v) for v in self.accepted[:k]]
        d["steps_accepted"], d["steps_rejected"], d["final_lambda"] = self.steps_accepted, self.steps_rejected, self.final_lambda
        return d


PG_MAX_PAIRS = 4096          # LILI_PG_MAX_PAIRS: pairs one lili_pose_graph_marginals call takes


class PgMarginalsInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_nodes", C.c_int32), ("n_loops", C.c_int32), ("reduced_unknowns", C.c_int32), ("kernel_ms", C.c_float), ("reserved_", C.c_int32)]

    def as_dict(self):
        return dict(status=self.status, n_nodes=self.n_nodes, n_loops=self.n_loops, reduced_unknowns=self.reduced_unknowns, kernel_ms=float(self.kernel_ms))


class WindowPrior(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_blocks", C.c_int32), ("reserved_", C.c_int32), ("block_kind", C.POINTER(C.c_int32)),
                ("block_keyframe", C.POINTER(C.c_int32)), ("x0", C.POINTER(C.c_double)), ("J0", C.POINTER(C.c_double)), ("r0", C.POINTER(C.c_double))]


class WindowPriorStorage(C.Structure):
    """lili_window_prior_storage: `prior` points into the arrays of the same object (do not copy it once filled)."""
    _fields_ = [("prior", WindowPrior), ("block_kind", C.c_int32 * 12), ("block_keyframe", C.c_int32 * 12), ("rank", C.c_int32), ("sweeps_mm", C.c_int32), ("sweeps_s", C.c_int32), ("reserved_", C.c_int32),
                ("x0", C.c_double * 64), ("r0", C.c_double * 60), ("J0", C.c_double * 3600)]


class WindowCycleOptions(C.Structure):
    """lili_window_cycle_options; the defaults are the literals of the reference's write-back gates."""
    _fields_ = [("gate_p", C.c_double), ("gate_q", C.c_double), ("gate_v", C.c_double), ("gate_ba", C.c_double), ("gate_bg", C.c_double),
                ("use_resident_prior", C.c_int32), ("reserved_", C.c_int32)]

    def __init__(self, gate_p=10.0, gate_q=10.0, gate_v=10.0, gate_ba=22.0, gate_bg=22.0, use_resident_prior=0):
        super().__init__(gate_p, gate_q, gate_v, gate_ba, gate_bg, int(use_resident_prior), 0)


class WindowCycleResult(C.Structure):
    _fields_ = [("summary", LmSummary), ("solved", C.c_double * 64), ("abs_state", C.c_double * 64), ("next_state", C.c_double * 64), ("refused", C.c_uint32 * 4),
                ("prior_updated", C.c_int32), ("prior_n", C.c_int32), ("prior_blocks", C.c_int32), ("rank", C.c_int32), ("sweeps_mm", C.c_int32), ("sweeps_s", C.c_int32)]


class WindowProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kind_mask", C.c_int32), ("slots", C.POINTER(C.c_int32)), ("imu", C.POINTER(WindowImu)), ("prior", C.POINTER(WindowPrior)),
                ("sb_prior", C.POINTER(C.c_double)), ("q_lb", C.c_double * 4), ("t_lb", C.c_double * 3)]


class S2MParams(C.Structure):
    _fields_ = [("variant", C.c_int), ("loss", C.c_int), ("loss_a", C.c_double), ("lidar_const", C.c_double),
                ("kd_max_radius", C.c_double), ("edge_gate", C.c_double), ("surf_dist_thres", C.c_double),
                ("reflect_thres", C.c_double), ("surf_weight_min", C.c_double), ("edge_dist_max", C.c_double),
                ("q_lb", C.c_double * 4), ("t_lb", C.c_double * 3), ("scale_surf_num", C.c_double),
                ("scale_edge_num", C.c_double)]


class IcpParams(C.Structure):
    _fields_ = [("max_corr_dist", C.c_double), ("max_iterations", C.c_int32), ("reserved_", C.c_int32), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double)]


ICP_MAX_LOG = 128


class IcpIteration(C.Structure):
    _fields_ = [("mse", C.c_double), ("cos_angle", C.c_double), ("translation_sqr", C.c_double), ("n_corr", C.c_int32), ("state", C.c_int32)]


class IcpResult(C.Structure):
    _fields_ = [("transform", C.c_double * 16), ("converged", C.c_int32), ("state", C.c_int32), ("iterations", C.c_int32), ("n_logged", C.c_int32),
                ("fitness", C.c_double), ("stage_us", C.c_double * 4), ("it", IcpIteration * ICP_MAX_LOG)]


class PlaceParams(C.Structure):
    _fields_ = [("n_ring", C.c_int32), ("n_sector", C.c_int32), ("max_radius", C.c_float), ("lidar_height", C.c_float), ("kind", C.c_int32), ("reserved_", C.c_int32)]


class PlaceQuery(C.Structure):
    _fields_ = [("id", C.c_int32), ("max_id", C.c_int32), ("desc", C.c_void_p), ("time", C.c_double), ("min_time_gap", C.c_double)]


class PlaceMatch(C.Structure):
    _fields_ = [("id", C.c_int32), ("shift", C.c_int32), ("distance", C.c_double)]


class PlaceSubmap(C.Structure):
    _fields_ = [("back", C.c_int32), ("fwd", C.c_int32), ("level", C.c_int32), ("reserved_", C.c_int32)]


PLACE_TILE_ROWS = 2048      # LILI_PLACE_TILE_ROWS: rows of a descriptor's concatenation one workgroup bins


def make_params(variant="rot", **kw):
    """Matcher parameters of the reference configs:
    L/config/config_fr_iosb.yaml ('livox'), R/config/config_fr_iosb.yaml ('rot'),
    L/src/LidarOdometry.cpp:365,389,400,507 ('frontend')."""
    p = S2MParams()
    if variant == "livox":
        p.variant, p.loss, p.loss_a = VARIANT_LIVOX, LOSS_CAUCHY, 1.0
        p.lidar_const, p.kd_max_radius, p.edge_gate = 20.0, 1.0, 1.0
        p.surf_dist_thres, p.reflect_thres, p.surf_weight_min, p.edge_dist_max = 0.12, 15.0, 0.2, 0.0
        p.q_lb[:] = [0.0, 0.0, 0.0, 1.0]
        p.t_lb[:] = [-0.0265, 0.0202, 0.05309]
        p.scale_surf_num = p.scale_edge_num = 0.0
    elif variant == "rot":
        p.variant, p.loss, p.loss_a = VARIANT_ROT, LOSS_CAUCHY, 1.0
        p.lidar_const, p.kd_max_radius, p.edge_gate = 7.5, 1.0, 1.0
        p.surf_dist_thres, p.reflect_thres, p.surf_weight_min, p.edge_dist_max = 0.12, 0.0, 0.3, 0.1
        p.q_lb[:] = [0.7071, 0.0, 0.0, 0.7071]
        p.t_lb[:] = [-0.18, 0.0, -0.095]
        p.scale_surf_num, p.scale_edge_num = 1000.0, 200.0
    elif variant == "frontend":
        p.variant, p.loss, p.loss_a = VARIANT_FRONTEND, LOSS_HUBER, 0.1
        p.lidar_const, p.kd_max_radius, p.edge_gate = 1.0, 1.0, 1.0
        p.surf_dist_thres, p.reflect_thres, p.surf_weight_min, p.edge_dist_max = 0.06, 0.0, 0.4, 0.0
        p.q_lb[:] = [1.0, 0.0, 0.0, 0.0]
        p.t_lb[:] = [0.0, 0.0, 0.0]
        p.scale_surf_num = p.scale_edge_num = 0.0
    else:
        raise ValueError(variant)
    for k, v in kw.items():
        if k in ("q_lb", "t_lb"):
            getattr(p, k)[:] = list(v)
        else:
            setattr(p, k, v)
    return p


_lib = None

_SIGS = {
    "lili_abi_version": (C.c_int, []),
    "lili_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "lili_ctx_destroy": (None, [C.c_void_p]),
    "lili_last_error": (C.c_char_p, [C.c_void_p]),
    "lili_sync": (C.c_int, [C.c_void_p]),
    "lili_set_debug": (C.c_int, [C.c_void_p, C.c_int]),
    "lili_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "lili_extract_rot": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.c_void_p, C.c_void_p, C.POINTER(RotParams), C.POINTER(FeatureOut), C.POINTER(FeatureOut), C.POINTER(FeatureOut)]),
    "lili_extract_rot_debug": (C.c_int, [C.c_void_p] + [C.c_void_p] * 11),
    "lili_extract_livox": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.c_int, C.c_void_p, C.POINTER(LivoxParams), C.POINTER(FeatureOut), C.POINTER(FeatureOut), C.POINTER(FeatureOut)]),
    "lili_extract_livox_debug": (C.c_int, [C.c_void_p] * 6),
    "lili_extract_rot_device": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.POINTER(Cloud), C.POINTER(Cloud)]),
    "lili_extract_livox_device": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.POINTER(Cloud)]),
    "lili_frontend_frame": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.c_int, C.c_void_p, C.POINTER(LivoxParams), C.POINTER(S2MParams), C.POINTER(FrontendOptions), C.c_void_p, C.c_void_p,
                                      C.POINTER(FrontendResult)]),
    "lili_frontend_frame_rot": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.c_void_p, C.c_void_p, C.POINTER(RotParams), C.POINTER(S2MParams), C.POINTER(FrontendOptions), C.c_void_p, C.c_void_p,
                                          C.POINTER(FrontendResult)]),
    "lili_backend_keyframe_prepare": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.POINTER(Cloud), C.c_void_p, C.c_void_p, C.POINTER(Cloud), C.POINTER(Cloud), C.POINTER(C.c_int), C.c_int,
                                                C.c_void_p, C.c_void_p, C.POINTER(S2MParams), C.POINTER(BackendOptions), C.c_void_p, C.POINTER(BackendResult)]),
    "lili_kf_rule_reset": (None, [C.POINTER(KfRuleState)]),
    "lili_kf_rule_step": (C.c_int, [C.POINTER(KfRuleState), C.c_void_p, C.c_void_p, C.c_int]),
    "lili_pose_relative": (C.c_int, [C.c_void_p] * 6),
    "lili_keyframe_undistort": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(Cloud)), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.POINTER(FeatureOut)]),
    "lili_frontend_keyframe": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Cloud), C.POINTER(Cloud), C.POINTER(Cloud)]),
    "lili_frontend_keyframe_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FeatureOut)]),
    "lili_frontend_reset": (C.c_int, [C.c_void_p]),
    "lili_frontend_flush": (C.c_int, [C.c_void_p, C.POINTER(S2MParams), C.POINTER(FrontendOptions), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lili_voxel_filter": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.c_float, C.POINTER(FeatureOut), C.c_void_p]),
    "lili_localmap_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "lili_localmap_push": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Cloud), C.c_void_p, C.c_void_p, C.c_int]),
    "lili_localmap_commit": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lili_localmap_get": (C.c_int, [C.c_void_p, C.POINTER(FeatureOut)]),
    "lili_localmap_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lili_localmap_repose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lili_voxel_filter_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lili_map_set": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Cloud), C.c_double]),
    "lili_map_density": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "lili_map_debug_index": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(MapIndexInfo)] + [C.c_void_p, C.c_size_t] * 6),
    "lili_s2m_linearize_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_associate_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_map_set_begin": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Cloud), C.c_double]),
    "lili_map_set_end": (C.c_int, [C.c_void_p, C.c_int]),
    "lili_map_focus": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_double]),
    "lili_map_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "lili_map_build_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lili_s2m_set_queries": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Cloud)]),
    "lili_s2m_associate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2MParams), C.POINTER(C.c_int)]),
    "lili_s2m_linearize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2MParams), C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "lili_s2m_get_surf_records": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "lili_s2m_get_edge_records": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "lili_s2m_get_neighbors": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lili_s2m_pose_set": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "lili_s2m_pose_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "lili_s2m_last_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lili_s2m_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.c_void_p]),
    "lili_s2m_associate_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams)]),
    "lili_s2m_counts_export": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lili_s2m_counts_import": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lili_s2m_linearize_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.c_void_p]),
    "lili_s2m_gn_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lili_s2m_iterate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int]),
    "lili_s2m_iterate_inner": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int, C.c_int]),
    "lili_s2m_iterate_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int]),
    "lili_s2m_debug_times": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]),
    "lili_s2m_pose_copy": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "lili_s2m_iterate_restart": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "lili_s2m_iterate_sharded": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_lm_default_options": (None, [C.POINTER(LmOptions)]),
    "lili_s2m_solve_lm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(S2MParams), C.POINTER(LmOptions), C.POINTER(LmSummary)]),
    "lili_s2m_solve_lm_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(S2MParams), C.POINTER(LmOptions), C.POINTER(LmSummary)]),
    "lili_s2m_counts_window_sharded": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_linearize_window_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(S2MParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_linearize_window_sharded": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2MParams), C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_iterate_window_sharded": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_linearize_window_gather": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(S2MParams), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_linearize_window_gather_at": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2MParams), C.POINTER(C.c_int), C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_s2m_iterate_window_gather": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(S2MParams), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_host_alloc": (C.c_void_p, [C.c_size_t]),
    "lili_host_free": (None, [C.c_void_p]),
    "lili_p2p_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "lili_p2p_handle": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lili_p2p_connect": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lili_p2p_allreduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lili_p2p_status": (C.c_int, [C.c_void_p]),
    "lili_p2p_set_timeout": (C.c_int, [C.c_void_p, C.c_double]),
    "lili_p2p_destroy": (None, [C.c_void_p]),
    "lili_livox_custom_to_cloud": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_int]),
    "lili_imu_reset": (None, [C.c_void_p]),
    "lili_imu_integrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p]),
    "lili_imu_preintegrate": (C.c_int, [C.c_void_p, C.POINTER(ImuSegment), C.c_int, C.POINTER(WindowImu), C.POINTER(ImuPrediction)]),
    "lili_imu_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "lili_imu_kf_reset": (None, [C.c_void_p]),
    "lili_imu_keyframe_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "lili_local_graph_propagate": (C.c_int, [C.c_void_p, C.POINTER(LocalWalk), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_local_graph_evaluate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "lili_local_graph_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LmOptions), C.POINTER(LocalGraphSummary)]),
    "lili_local_graph": (C.c_int, [C.c_void_p, C.POINTER(LocalWalk), C.c_int, C.c_void_p, C.POINTER(LmOptions), C.c_void_p, C.c_void_p, C.POINTER(LocalGraphSummary)]),
    "lili_local_graph_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "lili_pg_default_options": (None, [C.POINTER(PgOptions)]),
    "lili_pose_graph_reset": (C.c_int, [C.c_void_p]),
    "lili_pose_graph_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "lili_pose_graph_add_loop": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lili_pose_graph_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lili_pose_graph_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lili_pose_graph_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lili_pose_graph_evaluate": (C.c_int, [C.c_void_p, C.POINTER(PgOptions), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_pose_graph_solve": (C.c_int, [C.c_void_p, C.POINTER(PgOptions), C.POINTER(PgSummary)]),
    "lili_pose_graph_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "lili_pose_graph_add_loop_robust": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    "lili_pose_graph_loop_status": (C.c_int, [C.c_void_p, C.POINTER(PgOptions), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lili_pg_lm_default_options": (None, [C.POINTER(PgLmOptions)]),
    "lili_pose_graph_solve_lm": (C.c_int, [C.c_void_p, C.POINTER(PgOptions), C.POINTER(PgLmOptions), C.POINTER(PgLmSummary)]),
    "lili_pose_graph_marginals": (C.c_int, [C.c_void_p, C.POINTER(PgOptions), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PgMarginalsInfo)]),
    "lili_pose_relative_covariance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_loop_measurement": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_correct_poses": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_marg_add_lidar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lili_gn_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_gram_to_factor": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "lili_icp_default_params": (None, [C.POINTER(IcpParams)]),
    "lili_loop_cloud": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Cloud), C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lili_icp_set_cloud": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Cloud)]),
    "lili_icp_get_cloud": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(FeatureOut)]),
    "lili_icp_align": (C.c_int, [C.c_void_p, C.POINTER(IcpParams), C.c_void_p, C.POINTER(IcpResult)]),
    "lili_icp_fitness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "lili_icp_get_correspondences": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lili_archive_reset": (C.c_int, [C.c_void_p]),
    "lili_archive_set_extrinsic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_archive_push": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.POINTER(Cloud), C.POINTER(Cloud), C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "lili_archive_push_slot": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Cloud), C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "lili_archive_set_poses": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lili_archive_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lili_archive_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "lili_archive_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(FeatureOut)]),
    "lili_archive_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Cloud)]),
    "lili_loop_cloud_archive": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lili_loop_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lili_global_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lili_global_map_get": (C.c_int, [C.c_void_p, C.POINTER(FeatureOut), C.c_void_p]),
    "lili_global_map_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "lili_global_map_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lili_global_map_crop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FeatureOut), C.c_void_p, C.POINTER(C.c_int64)]),
    "lili_global_map_export": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "lili_global_map_import": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_place_default_params": (None, [C.POINTER(PlaceParams)]),
    "lili_place_layout": (C.c_int, [C.POINTER(PlaceParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_place_update": (C.c_int, [C.c_void_p, C.POINTER(PlaceParams), C.POINTER(C.c_int)]),
    "lili_place_describe": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.POINTER(PlaceParams), C.c_void_p]),
    "lili_place_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lili_place_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(PlaceParams), C.POINTER(C.c_int64)]),
    "lili_place_search": (C.c_int, [C.c_void_p, C.POINTER(PlaceQuery), C.c_int, C.c_int, C.POINTER(PlaceMatch), C.POINTER(C.c_int)]),
    "lili_place_guess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lili_place_set_submap": (C.c_int, [C.c_void_p, C.POINTER(PlaceSubmap)]),
    "lili_place_get_submap": (C.c_int, [C.c_void_p, C.POINTER(PlaceSubmap)]),
    "lili_place_window": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lili_place_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lili_place_relative": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_place_describe_submap": (C.c_int, [C.c_void_p, C.POINTER(Cloud), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PlaceParams), C.c_void_p]),
    "lili_window_sqrt_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lili_window_evaluate": (C.c_int, [C.c_void_p, C.POINTER(WindowProblem), C.POINTER(S2MParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lili_window_solve": (C.c_int, [C.c_void_p, C.POINTER(WindowProblem), C.POINTER(S2MParams), C.POINTER(LmOptions), C.c_void_p, C.POINTER(LmSummary)]),
    "lili_window_state_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lili_marg_schur": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "lili_window_marginalize": (C.c_int, [C.c_void_p, C.POINTER(WindowProblem), C.POINTER(S2MParams), C.c_void_p, C.POINTER(WindowPriorStorage)]),
    "lili_window_cycle": (C.c_int, [C.c_void_p, C.POINTER(WindowProblem), C.POINTER(S2MParams), C.POINTER(LmOptions), C.POINTER(WindowCycleOptions), C.c_void_p,
                                    C.POINTER(WindowCycleResult)]),
    "lili_window_cycle_reset": (C.c_int, [C.c_void_p]),
    "lili_window_prior_get": (C.c_int, [C.c_void_p, C.POINTER(WindowPriorStorage)]),
    "lili_window_prior_set": (C.c_int, [C.c_void_p, C.POINTER(WindowPrior)]),
}


def exported_symbols():
    """Names include/lili_hip.h declares (used by the CPU-side symbol test)."""
    return sorted(_SIGS)


def load_library():
    """Loads liblili_hip.so.  Raises LiliError if it has not been built — there is no other backend."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("LILI_HIP_LIBRARY", LIB_PATH)   # A/B builds of the SAME library (tools/); never another backend
    if not os.path.exists(path):
        raise LiliError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). The hot path has no CPU fallback.")
    # PyTorch wheels bundle their own libamdhip64 (same soname, different file name).  If this library pulled in the
    # system copy first, a later `import torch` would start a SECOND HIP runtime in the process and find no GPU.
    # Importing torch first makes both share one runtime.  (C/C++ hosts without torch are unaffected.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)      # AttributeError here = ABI mismatch between header and library
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class PinnedArray:
    """numpy view of page-locked host memory (lili_host_alloc): clouds passed from it are DMA'd, not staged.  Keep the object
    alive as long as the array is used; close() (or garbage collection) frees the memory."""

    def __init__(self, shape, dtype=np.float32):
        self.lib = load_library()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = self.lib.lili_host_alloc(max(n, 1))
        if not self.ptr:
            raise LiliError("lili_host_alloc failed")
        buf = (C.c_ubyte * max(n, 1)).from_address(self.ptr)
        buf._lili_owner = _PinnedBlock(self.lib, self.ptr)      # the ctypes buffer is the base object of every numpy view: the block lives as long as any view
        self._block = buf._lili_owner
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        """Drops this object's reference; the memory is released once no numpy view of it is left (never under a live view)."""
        self.array = None
        self._block = None
        self.ptr = None

    __del__ = close


class _PinnedBlock:
    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def __del__(self):
        if self.ptr:
            try:
                self.lib.lili_host_free(C.c_void_p(self.ptr))
            except Exception:   # noqa: BLE001  (interpreter shutdown)
                pass
            self.ptr = None


def _f64(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} doubles")
    return a


def cloud_from_numpy(arr, aux_col=None):
    """Describes a contiguous float32 (n, k>=3) host array as a lili_cloud (stride = 4k bytes)."""
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    if arr.ndim != 2 or arr.shape[1] < 3:
        raise ValueError("cloud array must be (n, >=3) float32")
    c = Cloud(arr.ctypes.data if arr.size else None, arr.shape[0], arr.shape[1] * 4,
              -1 if aux_col is None else int(aux_col) * 4, MEM_HOST)
    c._keep = arr
    return c


def cloud_from_device(ptr, n, stride, aux_offset=-1):
    return Cloud(ptr, n, stride, aux_offset, MEM_DEVICE)


class Context:
    """One HIP stream + device buffers (lili_ctx)."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.lili_ctx_create(C.byref(h), int(device), C.c_void_p(stream) if stream else None)
        if rc != OK:
            raise LiliError(f"lili_ctx_create failed ({rc}): no usable gfx950 device — the hot path has no CPU fallback")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lili_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc != OK:
            raise LiliError(f"lili error {rc}: {self.lib.lili_last_error(self.h).decode()}")

    def sync(self):
        self._chk(self.lib.lili_sync(self.h))

    def set_option(self, name, value):
        self._chk(self.lib.lili_set_option(self.h, name.encode(), int(value)))

    def set_debug(self, keep_neighbors=True):
        self._chk(self.lib.lili_set_debug(self.h, int(bool(keep_neighbors))))


class ScanToMapMatcher:
    """Host-side mirror of the reference's matcher calls (names follow BackendFusion.cpp):

        setInputCloud            -> set_input_cloud            (L/src/BackendFusion.cpp:839-840)
        findCorrespondingSurfFeatures   -> find_corresponding_surf_features     (L:1601)
        findCorrespondingCornerFeatures -> find_corresponding_corner_features   (L:1531)
        N x CostFunction::Evaluate + JtJ -> linearize                            (LidarKeyframeFactor.h, MarginalizationFactor.cpp:3-71)
    """

    def __init__(self, ctx, params):
        self.ctx = ctx
        self.lib = ctx.lib
        self.params = params

    # -- map ------------------------------------------------------------------------------------
    def set_input_cloud(self, kind, cloud, max_sq_radius=None):
        if not isinstance(cloud, Cloud):
            cloud = cloud_from_numpy(cloud, aux_col=3 if (np.ndim(cloud) == 2 and np.shape(cloud)[1] > 3) else None)
        if max_sq_radius is None:
            max_sq_radius = self.params.kd_max_radius if kind == KIND_SURF else self.params.edge_gate
        self.ctx._chk(self.lib.lili_map_set(self.ctx.h, kind, C.byref(cloud), float(max_sq_radius)))

    def set_input_cloud_begin(self, kind, cloud, max_sq_radius=None):
        """Starts building the NEXT index of `kind` on a side stream (work already enqueued keeps the current one); finish with
        set_input_cloud_end.  The cloud's memory must stay valid until then (a reference is kept here)."""
        if not isinstance(cloud, Cloud):
            cloud = cloud_from_numpy(cloud, aux_col=3 if (np.ndim(cloud) == 2 and np.shape(cloud)[1] > 3) else None)
        if max_sq_radius is None:
            max_sq_radius = self.params.kd_max_radius if kind == KIND_SURF else self.params.edge_gate
        self._pending_cloud = getattr(self, "_pending_cloud", {})
        self._pending_cloud[kind] = cloud
        self.ctx._chk(self.lib.lili_map_set_begin(self.ctx.h, kind, C.byref(cloud), float(max_sq_radius)))

    def set_input_cloud_end(self, kind):
        self.ctx._chk(self.lib.lili_map_set_end(self.ctx.h, kind))
        getattr(self, "_pending_cloud", {}).pop(kind, None)

    def map_info(self, kind):
        n, nc, ce = C.c_int64(), C.c_int64(), C.c_double()
        self.ctx._chk(self.lib.lili_map_info(self.ctx.h, kind, C.byref(n), C.byref(nc), C.byref(ce)))
        return n.value, nc.value, ce.value

    def map_build_stats(self):
        """(index builds started from a guessed box, those repeated with the true box, builds repeated with the three-kernel scan)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.ctx._chk(self.lib.lili_map_build_stats(self.ctx.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def map_focus(self, center=None, radius=0.0):
        """Hint for the following set_input_cloud calls: build the super-row copy only within `radius` of `center` (None / 0: everywhere)."""
        if center is None or not radius > 0:
            self.ctx._chk(self.lib.lili_map_focus(self.ctx.h, None, 0.0))
        else:
            c = (C.c_double * 3)(*[float(v) for v in center])
            self.ctx._chk(self.lib.lili_map_focus(self.ctx.h, c, float(radius)))

    def map_density(self, kind):
        """(mean points per gate-sized cell, fine cell edge or 0, squared radius covered by the fine index or 0)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.ctx._chk(self.lib.lili_map_density(self.ctx.h, kind, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def map_debug_index(self, kind, which=0):
        """The index itself (lili_map_debug_index; which: 0 = gate-sized, 1 = fine): dict(info=MapIndexInfo, cell_start, base (n, 4) float32 whose column 3
        holds the original index as int bits, aux or None, cell_start9 / super / super_aux or None).  Two calls: the sizes, then the arrays."""
        info = MapIndexInfo()
        self.ctx._chk(self.lib.lili_map_debug_index(self.ctx.h, kind, which, C.byref(info), *([None, 0] * 6)))
        n, n9, nc9 = info.n_points, info.n_super, info.bnx * info.bny * info.bnz
        cs = np.zeros(info.n_cells + 1, np.int32)
        base = np.zeros((n, 4), np.float32)
        aux = np.zeros(n, np.float32) if info.has_aux else None
        cs9 = np.zeros(nc9 + 1, np.int32) if info.has_super else None
        sup = np.zeros((n9, 4), np.float32) if info.has_super else None
        sup_aux = np.zeros(n9, np.float32) if info.has_super and info.has_aux else None
        args = []
        for a, cap in ((cs, cs.size), (base, n), (aux, n), (cs9, nc9 + 1), (sup, n9), (sup_aux, n9)):
            args += [_ptr(a), cap if a is not None else 0]
        self.ctx._chk(self.lib.lili_map_debug_index(self.ctx.h, kind, which, C.byref(info), *args))
        return dict(info=info, cell_start=cs, base=base, aux=aux, cell_start9=cs9, super=sup, super_aux=sup_aux)

    # -- queries --------------------------------------------------------------------------------
    def set_queries(self, slot, kind, cloud):
        if not isinstance(cloud, Cloud):
            cloud = cloud_from_numpy(cloud, aux_col=3 if (np.ndim(cloud) == 2 and np.shape(cloud)[1] > 3) else None)
        self.ctx._chk(self.lib.lili_s2m_set_queries(self.ctx.h, slot, kind, C.byref(cloud)))

    def _associate(self, slot, kind, q, t, want_count):
        t, q = _f64(t, 3), _f64(q, 4)
        n = C.c_int(0)
        self.ctx._chk(self.lib.lili_s2m_associate(self.ctx.h, slot, kind, _ptr(t), _ptr(q), C.byref(self.params),
                                                  C.byref(n) if want_count else None))
        return n.value if want_count else None

    def find_corresponding_surf_features(self, slot, q, t, want_count=True):
        return self._associate(slot, KIND_SURF, q, t, want_count)

    def find_corresponding_corner_features(self, slot, q, t, want_count=True):
        return self._associate(slot, KIND_EDGE, q, t, want_count)

    def linearize(self, slot, t, q, kind_mask=MASK_SURF | MASK_EDGE):
        t, q = _f64(t, 3), _f64(q, 4)
        gram = np.zeros(64)
        cost = C.c_double(0)
        counts = np.zeros(2, np.int32)
        self.ctx._chk(self.lib.lili_s2m_linearize(self.ctx.h, slot, kind_mask, _ptr(t), _ptr(q), C.byref(self.params),
                                                  _ptr(gram), C.byref(cost), _ptr(counts)))
        return gram.reshape(8, 8), cost.value, counts

    # -- copy-outs ------------------------------------------------------------------------------
    def surf_records(self, slot, capacity):
        qi = np.zeros(capacity, np.int32)
        cp = np.zeros((capacity, 3), np.float32)
        nn = np.zeros((capacity, 3), np.float32)
        d = np.zeros(capacity, np.float32)
        sc = np.zeros(capacity, np.float64)
        n = C.c_size_t(0)
        self.ctx._chk(self.lib.lili_s2m_get_surf_records(self.ctx.h, slot, capacity, _ptr(qi), _ptr(cp), _ptr(nn), _ptr(d), _ptr(sc), C.byref(n)))
        k = min(n.value, capacity)
        return dict(count=n.value, query_index=qi[:k], cp=cp[:k], n=nn[:k], d=d[:k], score=sc[:k])

    def edge_records(self, slot, capacity):
        qi = np.zeros(capacity, np.int32)
        cp = np.zeros((capacity, 3), np.float32)
        a = np.zeros((capacity, 3), np.float32)
        b = np.zeros((capacity, 3), np.float32)
        s = np.zeros(capacity, np.float32)
        n = C.c_size_t(0)
        self.ctx._chk(self.lib.lili_s2m_get_edge_records(self.ctx.h, slot, capacity, _ptr(qi), _ptr(cp), _ptr(a), _ptr(b), _ptr(s), C.byref(n)))
        k = min(n.value, capacity)
        return dict(count=n.value, query_index=qi[:k], cp=cp[:k], a=a[:k], b=b[:k], s=s[:k])

    def neighbors(self, slot, kind, n_q):
        idx = np.zeros((n_q, 5), np.int32)
        d2 = np.zeros((n_q, 5), np.float32)
        self.ctx._chk(self.lib.lili_s2m_get_neighbors(self.ctx.h, slot, kind, n_q, _ptr(idx), _ptr(d2)))
        return idx, d2

    # -- device-resident iterations -------------------------------------------------------------
    def pose_set(self, slot, t, q):
        t, q = _f64(t, 3), _f64(q, 4)
        self.ctx._chk(self.lib.lili_s2m_pose_set(self.ctx.h, slot, _ptr(t), _ptr(q)))

    def pose_get(self, slot):
        t, q = np.zeros(3), np.zeros(4)
        st = C.c_int(0)
        self.ctx._chk(self.lib.lili_s2m_pose_get(self.ctx.h, slot, _ptr(t), _ptr(q), C.byref(st)))
        return t, q, st.value

    def last_step(self, slot):
        """(delta[6] = dt, rotation vector; number of GN updates since pose_set; status of the last one)."""
        d = np.zeros(6)
        n, st = C.c_int(0), C.c_int(0)
        self.ctx._chk(self.lib.lili_s2m_last_step(self.ctx.h, slot, _ptr(d), C.byref(n), C.byref(st)))
        return d, n.value, st.value

    def accumulate(self, slot, d_gram_ptr, kind_mask=MASK_SURF):
        self.ctx._chk(self.lib.lili_s2m_accumulate(self.ctx.h, slot, kind_mask, C.byref(self.params), C.c_void_p(d_gram_ptr)))

    def associate_dev(self, slot, kind_mask=MASK_SURF):
        self.ctx._chk(self.lib.lili_s2m_associate_dev(self.ctx.h, slot, kind_mask, C.byref(self.params)))

    def counts_export(self, slot, d_counts_ptr):
        self.ctx._chk(self.lib.lili_s2m_counts_export(self.ctx.h, slot, C.c_void_p(d_counts_ptr)))

    def counts_import(self, slot, d_counts_ptr):
        self.ctx._chk(self.lib.lili_s2m_counts_import(self.ctx.h, slot, C.c_void_p(d_counts_ptr)))

    def linearize_dev(self, slot, d_gram_ptr, kind_mask=MASK_SURF):
        self.ctx._chk(self.lib.lili_s2m_linearize_dev(self.ctx.h, slot, kind_mask, C.byref(self.params), C.c_void_p(d_gram_ptr)))

    def gn_update(self, slot, d_gram_ptr):
        self.ctx._chk(self.lib.lili_s2m_gn_update(self.ctx.h, slot, C.c_void_p(d_gram_ptr)))

    def iterate_sharded(self, slot, n_iters, d_counts_ptr, d_gram_ptr, allreduce_fn=None, comm=None, restart_every=0, restart_slot=1,
                        kind_mask=MASK_SURF):
        """n_iters staged iterations with the two collectives enqueued from C (lili_s2m_iterate_sharded).  allreduce_fn: address
        of an ncclAllReduce-compatible function (int), comm: its communicator handle (int); None = single rank."""
        self.ctx._chk(self.lib.lili_s2m_iterate_sharded(self.ctx.h, slot, kind_mask, C.byref(self.params), int(n_iters), int(restart_every),
                                                        int(restart_slot), C.c_void_p(allreduce_fn), C.c_void_p(comm),
                                                        C.c_void_p(d_counts_ptr), C.c_void_p(d_gram_ptr)))

    def counts_window_sharded(self, slots, d_counts_ptr, allreduce_fn=None, comm=None, kind_mask=MASK_SURF | MASK_EDGE):
        arr = (C.c_int * len(slots))(*slots)
        self.ctx._chk(self.lib.lili_s2m_counts_window_sharded(self.ctx.h, arr, len(slots), kind_mask, C.c_void_p(allreduce_fn), C.c_void_p(comm), C.c_void_p(d_counts_ptr)))

    def linearize_window_sharded(self, slots, ts, qs, d_gram_ptr, allreduce_fn=None, comm=None, kind_mask=MASK_SURF | MASK_EDGE):
        """One evaluation of the joint window with the queries of every slot sharded over the ranks: [(gram 8x8, cost, counts)] per slot,
        the same bits on every rank."""
        n = len(slots)
        arr = (C.c_int * n)(*slots)
        t = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(n, 3)); q = np.ascontiguousarray(np.asarray(qs, np.float64).reshape(n, 4))
        G = np.zeros((n, 64)); cost = np.zeros(n); cnt = np.zeros((n, 2), np.int32)
        self.ctx._chk(self.lib.lili_s2m_linearize_window_sharded(self.ctx.h, arr, n, kind_mask, _ptr(t), _ptr(q), C.byref(self.params), C.c_void_p(allreduce_fn),
                                                                 C.c_void_p(comm), C.c_void_p(d_gram_ptr), _ptr(G), _ptr(cost), _ptr(cnt)))
        return [(G[i].reshape(8, 8), float(cost[i]), cnt[i].copy()) for i in range(n)]

    def iterate_window_sharded(self, slots, n_iters, d_counts_ptr, d_gram_ptr, allreduce_fn=None, comm=None, kind_mask=MASK_SURF | MASK_EDGE):
        arr = (C.c_int * len(slots))(*slots)
        self.ctx._chk(self.lib.lili_s2m_iterate_window_sharded(self.ctx.h, arr, len(slots), kind_mask, C.byref(self.params), int(n_iters), C.c_void_p(allreduce_fn),
                                                               C.c_void_p(comm), C.c_void_p(d_counts_ptr), C.c_void_p(d_gram_ptr)))

    def linearize_window_gather(self, slots, owner, rank, d_gram_ptr, allreduce_fn=None, comm=None, kind_mask=MASK_SURF | MASK_EDGE):
        """Slot-per-rank window: the records of one evaluation at the slots' device poses, gathered into d_gram (n x GRAM_DOUBLES, device)."""
        arr, own = (C.c_int * len(slots))(*slots), (C.c_int * len(slots))(*owner)
        self.ctx._chk(self.lib.lili_s2m_linearize_window_gather(self.ctx.h, arr, len(slots), kind_mask, C.byref(self.params), own, int(rank), allreduce_fn, comm, d_gram_ptr))

    def linearize_window_gather_at(self, slots, ts, qs, owner, rank, d_gram_ptr, allreduce_fn=None, comm=None, kind_mask=MASK_SURF | MASK_EDGE):
        """One solver evaluation of the slot-per-rank window at the body poses (ts[k], qs[k]): [(gram 8x8, cost, counts)] per slot, the same bits on every rank."""
        n = len(slots)
        arr, own = (C.c_int * n)(*slots), (C.c_int * n)(*owner)
        t = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(n, 3)); q = np.ascontiguousarray(np.asarray(qs, np.float64).reshape(n, 4))
        G = np.zeros((n, 64)); cost = np.zeros(n); cnt = np.zeros((n, 2), np.int32)
        self.ctx._chk(self.lib.lili_s2m_linearize_window_gather_at(self.ctx.h, arr, n, kind_mask, _ptr(t), _ptr(q), C.byref(self.params), own, int(rank), allreduce_fn, comm,
                                                                   d_gram_ptr, _ptr(G), _ptr(cost), _ptr(cnt)))
        return [(G[i].reshape(8, 8), float(cost[i]), cnt[i].copy()) for i in range(n)]

    def iterate_window_gather(self, slots, n_iters, owner, rank, d_gram_ptr, allreduce_fn=None, comm=None, kind_mask=MASK_SURF | MASK_EDGE):
        arr, own = (C.c_int * len(slots))(*slots), (C.c_int * len(slots))(*owner)
        self.ctx._chk(self.lib.lili_s2m_iterate_window_gather(self.ctx.h, arr, len(slots), kind_mask, C.byref(self.params), int(n_iters), own, int(rank), allreduce_fn, comm,
                                                              d_gram_ptr))

    def iterate_window(self, slots, n_iters, kind_mask=MASK_SURF):
        arr = (C.c_int * len(slots))(*[int(s) for s in slots])
        self.ctx._chk(self.lib.lili_s2m_iterate_window(self.ctx.h, arr, len(slots), kind_mask, C.byref(self.params), int(n_iters)))

    def debug_times(self, slot):
        out = (C.c_longlong * 16)()
        self.ctx._chk(self.lib.lili_s2m_debug_times(self.ctx.h, slot, out))
        return list(out)

    def pose_copy(self, dst_slot, src_slot):
        self.ctx._chk(self.lib.lili_s2m_pose_copy(self.ctx.h, dst_slot, src_slot))

    def iterate_restart(self, slot, n_iters, restart_every, restart_slot, kind_mask=MASK_SURF, time_association=False):
        """Returns the summed association-kernel time in ms when time_association (blocking), else None (async)."""
        ms = C.c_float(0)
        self.ctx._chk(self.lib.lili_s2m_iterate_restart(self.ctx.h, slot, kind_mask, C.byref(self.params), int(n_iters), int(restart_every),
                                                        int(restart_slot), C.byref(ms) if time_association else None))
        return ms.value if time_association else None

    def associate_window(self, slots, ts_assoc, qs_assoc, kind_mask=MASK_SURF | MASK_EDGE):
        """findCorresponding{Surf,Corner}Features of all keyframes of the window at the association poses; returns [(n_surf, n_edge)] per slot."""
        n = len(slots)
        arr = (C.c_int * n)(*[int(s) for s in slots])
        t = np.ascontiguousarray(np.asarray(ts_assoc, np.float64).reshape(n, 3))
        q = np.ascontiguousarray(np.asarray(qs_assoc, np.float64).reshape(n, 4))
        counts = np.zeros((n, 2), np.int32)
        self.ctx._chk(self.lib.lili_s2m_associate_window(self.ctx.h, arr, n, int(kind_mask), _ptr(t), _ptr(q), C.byref(self.params), _ptr(counts)))
        return [(int(counts[k, 0]), int(counts[k, 1])) for k in range(n)]

    def linearize_window(self, slots, ts, qs, kind_mask=MASK_SURF | MASK_EDGE):
        """One evaluation of the joint window: (Gram 8x8, cost, counts) per slot at the body poses (ts[k], qs[k]); one synchronisation for all."""
        n = len(slots)
        arr = (C.c_int * n)(*[int(s) for s in slots])
        t = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(n, 3))
        q = np.ascontiguousarray(np.asarray(qs, np.float64).reshape(n, 4))
        G = np.zeros((n, 64)); cost = np.zeros(n); counts = np.zeros((n, 2), np.int32)
        self.ctx._chk(self.lib.lili_s2m_linearize_window(self.ctx.h, arr, n, int(kind_mask), _ptr(t), _ptr(q), C.byref(self.params), _ptr(G), _ptr(cost), _ptr(counts)))
        return [(G[k].reshape(8, 8).copy(), float(cost[k]), (int(counts[k, 0]), int(counts[k, 1]))) for k in range(n)]

    def lm_options(self, **kw):
        """Ceres 2.0 defaults with max_iterations = 15 (what the reference's ceres::Solve runs with, L/src/BackendFusion.cpp:984-992), overridden by kw."""
        o = LmOptions()
        self.lib.lili_lm_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def solve_lm(self, slot, kind_mask=MASK_SURF | MASK_EDGE, options=None, want_summary=True, summary=None):
        """Levenberg-Marquardt on the records of the last association, one persistent launch (ceres::Solve's loop for the lidar blocks of one
        keyframe); returns the summary as a dict (blocking) or None (asynchronous).  summary: an LmSummary of the caller's to fill instead of a new one."""
        s = summary if summary is not None else LmSummary() if want_summary else None
        self.ctx._chk(self.lib.lili_s2m_solve_lm(self.ctx.h, slot, kind_mask, C.byref(self.params), C.byref(options) if options is not None else None,
                                                     C.byref(s) if s is not None else None))
        return s.as_dict() if s is not None else None

    def solve_lm_window(self, slots, kind_mask=MASK_SURF | MASK_EDGE, options=None, want_summary=True, summary=None):
        """summary: an (LmSummary * len(slots)) array of the caller's to fill instead of a new one"""
        arr = (C.c_int * len(slots))(*slots)
        s = summary if summary is not None else (LmSummary * len(slots))() if want_summary else None
        self.ctx._chk(self.lib.lili_s2m_solve_lm_window(self.ctx.h, arr, len(slots), kind_mask, C.byref(self.params),
                                                            C.byref(options) if options is not None else None, s))
        return [x.as_dict() for x in s] if s is not None else None

    def iterate(self, slot, n_iters, kind_mask=MASK_SURF):
        self.ctx._chk(self.lib.lili_s2m_iterate(self.ctx.h, slot, kind_mask, C.byref(self.params), int(n_iters)))

    def iterate_inner(self, slot, n_iters, kind_mask=MASK_SURF, want_cost=True):
        """n_iters x (linearise + reduce + GN update) on the records of the last association (ceres::Solve's inner loop)."""
        self.ctx._chk(self.lib.lili_s2m_iterate_inner(self.ctx.h, slot, kind_mask, C.byref(self.params), int(n_iters), 1 if want_cost else 0))


def extract_rot_device(ctx):
    """(full, edge, surf) device clouds of the last RotExtractor.extract on this context."""
    f, e, s = Cloud(), Cloud(), Cloud()
    ctx._chk(ctx.lib.lili_extract_rot_device(ctx.h, C.byref(f), C.byref(e), C.byref(s)))
    return f, e, s


def extract_livox_device(ctx):
    e, s = Cloud(), Cloud()
    ctx._chk(ctx.lib.lili_extract_livox_device(ctx.h, C.byref(e), C.byref(s)))
    return e, s


class KeyframeRule:
    """The odometry node's keyframe decision (L/src/LidarOdometry.cpp:565-585, 675-676; lili_kf_rule_step): one step() per frame with the pose it ended at.
    step() returns KF_NO, KF_YES or — the first frame of a sequence, whose clouds go out without deskew and without /odom — KF_FIRST; `flag` is the node's `kf`."""

    def __init__(self):
        self.lib = load_library()
        self.st = KfRuleState()
        self.reset()

    def reset(self):
        self.lib.lili_kf_rule_reset(C.byref(self.st))

    @property
    def flag(self):
        return bool(self.st.kf)

    def step(self, t, q, matched=True):
        t, q = _f64(t, 3), _f64(q, 4)
        rc = self.lib.lili_kf_rule_step(C.byref(self.st), _ptr(t), _ptr(q), 1 if matched else 0)
        if rc < 0:
            raise LiliError(f"lili_kf_rule_step failed ({rc})")
        return rc


def pose_relative(t_prev, q_prev, t_cur, q_cur):
    """computeRelative (L/src/LidarOdometry.cpp:444-480): (t_rel, q_rel) of the current pose in the previous one's frame, Eigen's order of operations."""
    a = [_f64(t_prev, 3), _f64(q_prev, 4), _f64(t_cur, 3), _f64(q_cur, 4)]
    t, q = np.zeros(3), np.zeros(4)
    if load_library().lili_pose_relative(*[_ptr(x) for x in a], _ptr(t), _ptr(q)) != OK:
        raise LiliError("lili_pose_relative failed")
    return t, q


def keyframe_undistort(ctx, clouds, time_offsets, t_rel, q_rel=None, out_ptrs=None):
    """undistortion(cloud, t_rel, q_rel) (L/src/LidarOdometry.cpp:178-199) of up to three clouds (Cloud or None each) in one launch; time_offsets: the byte
    offset of the time channel in each cloud's rows.  out_ptrs: device addresses of float4 buffers with room for each cloud (a cloud's own address: in place), or None
    — the rows then land in torch tensors the returned Clouds keep alive.  Returns three device Clouds (x', y', z', aux).  Asynchronous: ctx.sync() before reading."""
    arr = (C.POINTER(Cloud) * 3)()
    offs = (C.c_int * 3)(*[int(v) for v in time_offsets])
    outs = (FeatureOut * 3)()
    keep = []
    for k in range(3):
        c = clouds[k]
        n = 0 if c is None else int(c.n)
        if c is not None:
            arr[k] = C.pointer(c)
        if out_ptrs is not None and out_ptrs[k]:
            outs[k] = FeatureOut(out_ptrs[k], n, 16, MEM_DEVICE, 0)
            keep.append(None)
        else:
            import torch
            buf = torch.empty((max(n, 1), 4), dtype=torch.float32, device="cuda")
            outs[k] = FeatureOut(buf.data_ptr(), n, 16, MEM_DEVICE, 0)
            keep.append(buf)
    t = _f64(t_rel, 3)
    q = None if q_rel is None else _f64(q_rel, 4)
    ctx._chk(ctx.lib.lili_keyframe_undistort(ctx.h, arr, offs, _ptr(t), _ptr(q), outs))
    res = []
    for k in range(3):
        c = Cloud(outs[k].data, outs[k].count, 16, 12, MEM_DEVICE)
        c._keep = keep[k]
        res.append(c)
    return res


def frontend_keyframe(ctx, flavour, t_rel=None, q_rel=None, deskew=True):
    """publishCloudLast (L/src/LidarOdometry.cpp:624-650) for the last frame / extraction of `flavour` (VARIANT_LIVOX or VARIANT_ROT) on the context: (edge, surf, full) device
    Clouds of float4 rows, valid until the next extraction or keyframe call — usable as new_edge / new_surf of BackendKeyframes.prepare and as `full` of KeyframeArchive.push."""
    e, s, f = Cloud(), Cloud(), Cloud()
    t = None if t_rel is None else _f64(t_rel, 3)
    q = None if q_rel is None else _f64(q_rel, 4)
    ctx._chk(ctx.lib.lili_frontend_keyframe(ctx.h, int(flavour), _ptr(t), _ptr(q), 1 if deskew else 0, C.byref(e), C.byref(s), C.byref(f)))
    return e, s, f


def frontend_keyframe_get(ctx, kind):
    """One of the clouds of the last frontend_keyframe (0 edge, 1 surf, 2 full) as (n, 4) float32 rows on the host."""
    fo = FeatureOut(None, 0, 16, MEM_HOST, 0)
    ctx._chk(ctx.lib.lili_frontend_keyframe_get(ctx.h, int(kind), C.byref(fo)))
    out = np.zeros((max(fo.count, 1), 4), np.float32)
    fo = FeatureOut(out.ctypes.data, out.shape[0], 16, MEM_HOST, 0)
    ctx._chk(ctx.lib.lili_frontend_keyframe_get(ctx.h, int(kind), C.byref(fo)))
    return out[:fo.count]


def voxel_filter_device(ctx, cloud, leaf, d_out_ptr, capacity):
    """VoxelGrid of a device cloud into a caller-owned device float4 buffer; returns the output device cloud."""
    fo = FeatureOut(d_out_ptr, capacity, 16, MEM_DEVICE, 0)
    ctx._chk(ctx.lib.lili_voxel_filter(ctx.h, C.byref(cloud), float(leaf), C.byref(fo), None))
    return Cloud(d_out_ptr, min(fo.count, capacity), 16, 12, MEM_DEVICE)


def voxel_filter(ctx, pts_xyza, leaf):
    """pcl::VoxelGrid on (n,4) float32 rows (x, y, z, aux).  Returns (centroids (m,4), counts (m,))."""
    pts = np.ascontiguousarray(pts_xyza, dtype=np.float32)
    cloud = cloud_from_numpy(pts, aux_col=3)
    cap = max(pts.shape[0], 1)
    out = np.zeros((cap, 4), np.float32)
    cnt = np.zeros(cap, np.int32)
    fo = FeatureOut(out.ctypes.data, cap, 16, MEM_HOST, 0)
    ctx._chk(ctx.lib.lili_voxel_filter(ctx.h, C.byref(cloud), float(leaf), C.byref(fo), _ptr(cnt)))
    return out[:fo.count], cnt[:fo.count]


def voxel_filter_stats(ctx):
    """(filters served with guessed key bits — no host round trip for the bounding box —, guesses that did not hold) of this context so far."""
    a, b = C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx.lib.lili_voxel_filter_stats(ctx.h, C.byref(a), C.byref(b)))
    return a.value, b.value


class LocalMap:
    """Keyframe ring buffer + VoxelGrid + map index on the device (buildLocalMapWithLandMark / downSampleCloud /
    setInputCloud, L/src/BackendFusion.cpp:1387-1528, 839-840)."""

    def __init__(self, ctx, kind, width, leaf, max_sq_radius=1.0):
        self.ctx, self.kind, self.width, self.leaf, self.max_sq_radius = ctx, kind, int(width), float(leaf), float(max_sq_radius)
        ctx._chk(ctx.lib.lili_localmap_reset(ctx.h, kind))

    def push(self, feats_xyza, t, q):
        pts = np.ascontiguousarray(feats_xyza, dtype=np.float32)
        cloud = cloud_from_numpy(pts, aux_col=3 if pts.shape[1] > 3 else None)
        t, q = _f64(t, 3), _f64(q, 4)
        self.ctx._chk(self.ctx.lib.lili_localmap_push(self.ctx.h, self.kind, C.byref(cloud), _ptr(t), _ptr(q), self.width))

    def get(self, capacity):
        """The down-sampled local map of the last commit, (n, 4) float32 rows in map order."""
        out = np.zeros((max(int(capacity), 1), 4), np.float32)
        fo = FeatureOut(out.ctypes.data, out.shape[0], 16, MEM_HOST, 0)
        self.ctx._chk(self.ctx.lib.lili_localmap_get(self.ctx.h, C.byref(fo)))
        return out[:min(fo.count, out.shape[0])]

    def stats(self):
        """(incremental commits, full rebuilds) of this context so far."""
        a, b = C.c_int32(0), C.c_int32(0)
        self.ctx._chk(self.ctx.lib.lili_localmap_stats(self.ctx.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def commit(self):
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(self.ctx.lib.lili_localmap_commit(self.ctx.h, self.kind, self.leaf, self.max_sq_radius, C.byref(a), C.byref(b)))
        return a.value, b.value

    def repose(self, ts, qs):
        """The ring's keyframes (oldest first) take new map-frame poses (buildLocalMapWithLandMark's warm-up branch, L/src/BackendFusion.cpp:1407-1443);
        ts: (n, 3), qs: (n, 4) wxyz, n = ring size (keyframe_map_poses turns body poses into these).  Asynchronous; the next commit uses them."""
        _repose(self.ctx, 1 << self.kind, ts, qs)


def _repose(ctx, kind_mask, ts, qs):
    t = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(-1, 3))
    q = np.ascontiguousarray(np.asarray(qs, np.float64).reshape(-1, 4))
    if t.shape[0] != q.shape[0]:
        raise ValueError("repose: as many translations as rotations")
    ctx._chk(ctx.lib.lili_localmap_repose(ctx.h, int(kind_mask), t.shape[0], _ptr(t), _ptr(q)))


class RotExtractor:
    """Host-side mirror of LiLi-OM-ROT's Preprocessing::cloudHandler (R/src/Preprocessing.cpp:248-535)."""

    def __init__(self, ctx, n_scans=64, ds_rate=4, ds_v=0.6, near_range=3.0):
        self.ctx = ctx
        self.lib = ctx.lib
        self.params = RotParams(n_scans, ds_rate, ds_v, near_range)

    def extract_device(self, d_ptr, n, q_imu=(1.0, 0, 0, 0), q_lb=(1.0, 0, 0, 0)):
        """The scan is already in HBM as float4 rows (x, y, z, intensity) at device address d_ptr; the features stay in HBM
        (extract_rot_device() hands them on as device clouds).  Returns (n_full, n_edge, n_surf)."""
        cloud = Cloud(d_ptr, n, 16, 12, MEM_DEVICE)
        qi, ql = _f64(q_imu, 4), _f64(q_lb, 4)
        outs = [FeatureOut(None, 0, 16, MEM_DEVICE, 0) for _ in range(3)]
        self.ctx._chk(self.lib.lili_extract_rot(self.ctx.h, C.byref(cloud), _ptr(qi), _ptr(ql), C.byref(self.params),
                                                C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2])))
        return outs[0].count, outs[1].count, outs[2].count

    def _out_buffers(self, cap, reuse):
        """Three (cap, 4) float32 result buffers.  reuse: page-locked buffers owned by the extractor (DMA'd into, no per-call
        allocation; the returned arrays are VIEWS that the next call overwrites — what a ROS node's callback would do with one
        message in flight)."""
        if not reuse:
            return [np.zeros((cap, 4), np.float32) for _ in range(3)]
        if getattr(self, "_pin_cap", 0) < cap:
            # the old blocks are RETIRED, not freed: arrays handed out by earlier calls are views of them (freeing them here
            # left those views pointing at released page-locked memory); they go when the extractor does
            self._retired = getattr(self, "_retired", []) + list(getattr(self, "_pins", []))
            self._pins = [PinnedArray((cap, 4), np.float32) for _ in range(3)]
            self._pin_cap = cap
        return [p.array[:cap] for p in self._pins]

    def extract(self, pts_xyzi, q_imu=(1.0, 0, 0, 0), q_lb=(1.0, 0, 0, 0), debug=False, reuse=False):
        pts = np.ascontiguousarray(pts_xyzi, dtype=np.float32)
        n = pts.shape[0]
        cloud = cloud_from_numpy(pts, aux_col=3)
        cap = max(n, 1)
        bufs = self._out_buffers(cap, reuse)
        outs = [FeatureOut(b.ctypes.data, cap, 16, MEM_HOST, 0) for b in bufs]
        qi, ql = _f64(q_imu, 4), _f64(q_lb, 4)
        self.ctx._chk(self.lib.lili_extract_rot(self.ctx.h, C.byref(cloud), _ptr(qi), _ptr(ql), C.byref(self.params),
                                                C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2])))
        res = dict(full=bufs[0][:outs[0].count], edge=bufs[1][:outs[1].count], surf=bufs[2][:outs[2].count])
        if debug:
            counts = np.zeros(8, np.int32)
            rs, re_ = np.zeros(64, np.int32), np.zeros(64, np.int32)
            self.ctx._chk(self.lib.lili_extract_rot_debug(self.ctx.h, _ptr(counts), _ptr(rs), _ptr(re_), *([None] * 8)))
            nf, ne, ns, nfl, nlf, nsu = [int(v) for v in counts[:6]]
            arr = dict(full_src=np.zeros(nf, np.int32), curvature=np.zeros(nf, np.float32), label=np.zeros(nf, np.int32),
                       edge_idx=np.zeros(ne, np.int32), sharp_idx=np.zeros(ns, np.int32), flat_idx=np.zeros(nfl, np.int32),
                       lessflat_idx=np.zeros(nlf, np.int32), surf_cnt=np.zeros(nsu, np.int32))
            self.ctx._chk(self.lib.lili_extract_rot_debug(self.ctx.h, _ptr(counts), _ptr(rs), _ptr(re_), _ptr(arr["full_src"]),
                                                          _ptr(arr["curvature"]), _ptr(arr["label"]), _ptr(arr["edge_idx"]),
                                                          _ptr(arr["sharp_idx"]), _ptr(arr["flat_idx"]), _ptr(arr["lessflat_idx"]),
                                                          _ptr(arr["surf_cnt"])))
            res.update(arr)
            res.update(ring_start=rs[:self.params.n_scans], ring_end=re_[:self.params.n_scans], half_idx=int(counts[6]))
        return res


class LivoxExtractor:
    """Host-side mirror of LiLi-OM's Preprocessing::cloudHandler (L/src/Preprocessing.cpp:194-408)."""

    def __init__(self, ctx, surf_thres=0.28, edge_thres=4.0, near_range=0.1):
        self.ctx = ctx
        self.lib = ctx.lib
        self.params = LivoxParams(surf_thres, edge_thres, near_range)

    def extract(self, pts5, q_imu=(1.0, 0, 0, 0), debug=False, pcl_layout=False, reuse=False):
        """pts5: (n,5) float32 = x, y, z, intensity, curvature.  reuse: results land in page-locked buffers owned by the extractor
        (views that the next call overwrites), see RotExtractor._out_buffers."""
        pts = np.ascontiguousarray(pts5, dtype=np.float32)
        n = pts.shape[0]
        cloud = Cloud(pts.ctypes.data if n else None, n, 20, 12, MEM_HOST)
        cap = max(n, 24000)
        w = 12 if pcl_layout else 8
        if reuse:
            if getattr(self, "_pin_key", None) != (cap, w):
                for p_ in getattr(self, "_pins", []):
                    p_.close()
                self._pins = [PinnedArray((cap, w), np.float32) for _ in range(3)]
                self._pin_key = (cap, w)
            bufs = [p_.array for p_ in self._pins]
        else:
            bufs = [np.zeros((cap, w), np.float32) for _ in range(3)]
        outs = [FeatureOut(b.ctypes.data, cap, 4 * w, MEM_HOST, 0) for b in bufs]
        qi = _f64(q_imu, 4)
        self.ctx._chk(self.lib.lili_extract_livox(self.ctx.h, C.byref(cloud), 16, _ptr(qi), C.byref(self.params),
                                                  C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2])))
        res = dict(cutted=bufs[0][:outs[0].count], edge=bufs[1][:outs[1].count], surf=bufs[2][:outs[2].count])
        if debug:
            counts = np.zeros(3, np.int32)
            self.ctx._chk(self.lib.lili_extract_livox_debug(self.ctx.h, _ptr(counts), None, None, None, None))
            arr = dict(cut_src=np.zeros(counts[0], np.int32), cell_src=np.zeros(24000, np.int32),
                       edge_cell=np.zeros(counts[1], np.int32), surf_cell=np.zeros(counts[2], np.int32))
            self.ctx._chk(self.lib.lili_extract_livox_debug(self.ctx.h, _ptr(counts), _ptr(arr["cut_src"]), _ptr(arr["cell_src"]),
                                                            _ptr(arr["edge_cell"]), _ptr(arr["surf_cell"])))
            arr["cell_src"] = arr["cell_src"].reshape(6, 4000)
            res.update(arr)
        return res


class FrontendOdometry:
    """Host-side mirror of LidarOdometry::run (L/src/LidarOdometry.cpp:652-707) behind the extraction node (L/src/Preprocessing.cpp:219-401): one
    lili_frontend_frame call per Livox scan — extraction, down_size_filter_surf, the outer iterations against the local map of the last `width`
    frames, the ring push at the pose found and the next frame's local map, all device-resident.  The frame counter reproduces the node's start-up:
    frame 0 is only stored (system not initialised, L:659-663; its surf_frames entry is empty), frame 1 is matched against its own surf features with
    8 iterations (L:283-289, 501-502), later frames against the ring with `scan_match_cnt`.  The caller keeps poseInitialization's constant-velocity
    prediction (L:415-441)."""

    def __init__(self, ctx, params=None, surf_thres=0.28, edge_thres=4.0, near_range=0.1, leaf_query=0.4, leaf_map=0.4, width=20, slot=0,
                 scan_match_cnt=6, first_match_cnt=8, reference_startup=True, external_map=False, edges=False):
        """reference_startup = False: the replay tools' simpler start (frame 0 enters the ring with its features at the given pose, frame 1 is matched
        against it with `first_match_cnt` iterations) — same C call, other flags.  external_map = True (with edges: the edge features are queries too): every scan is
        matched with `scan_match_cnt` iterations against the indices the caller set with ScanToMapMatcher.set_input_cloud / lili_map_set, nothing joins the ring."""
        self.reference_startup = bool(reference_startup)
        self.base_flags = (FRAME_EXTERNAL_MAP if external_map else 0) | (FRAME_EDGES if edges else 0)
        self.ctx, self.lib = ctx, ctx.lib
        self.params = params if params is not None else make_params("frontend")
        self.livox = LivoxParams(surf_thres, edge_thres, near_range)
        self.opt = FrontendOptions(leaf_query, leaf_map, width, scan_match_cnt, slot, 0, 0)
        self.res = FrontendResult()
        self.scan_match_cnt, self.first_match_cnt = int(scan_match_cnt), int(first_match_cnt)
        self.n_frames = 0

    def reset(self):
        self.ctx._chk(self.lib.lili_frontend_reset(self.ctx.h))
        self.n_frames = 0

    def flush(self):
        """Builds the local map of everything pushed so far (the frame call leaves that to the next frame); returns (ring points, map points)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self.ctx._chk(self.lib.lili_frontend_flush(self.ctx.h, C.byref(self.params), C.byref(self.opt), C.byref(a), C.byref(b)))
        return a.value, b.value

    flavour = VARIANT_LIVOX

    def keyframe(self, t_rel=None, q_rel=None, deskew=True):
        """The last frame's three clouds as the node's publishCloudLast hands them to the back end (lili_frontend_keyframe): (edge, surf, full) device Clouds, moved by
        undistortion(cloud, t_rel, q_rel) when deskew is set (the node passes rel_pose's translation and no rotation).  Valid until the next frame."""
        return frontend_keyframe(self.ctx, self.flavour, t_rel, q_rel, deskew)

    def frame(self, scan, t_pred, q_pred, q_imu=(1.0, 0, 0, 0), timing=False):
        """scan: (n,5) float32 rows x, y, z, intensity, curvature (host; page-locked memory is read in place) or a Cloud.  Returns (t, q, info)."""
        if isinstance(scan, Cloud):
            cloud, curv_off = scan, 16
        else:
            n = scan.shape[0]
            cloud, curv_off = Cloud(scan.ctypes.data if n else None, n, 20, 12, MEM_HOST), 16
        k = self.n_frames
        if self.base_flags & FRAME_EXTERNAL_MAP:
            self.opt.n_iters, self.opt.flags = self.scan_match_cnt, self.base_flags
        else:
            self.opt.n_iters = 0 if k == 0 else (self.first_match_cnt if k == 1 else self.scan_match_cnt)
            self.opt.flags = (FRAME_PUSH_EMPTY if k == 0 else (FRAME_SELF_MAP if k == 1 else 0)) if self.reference_startup else 0
        self.opt.want_timing = 1 if timing else 0
        qi, tp, qp = _f64(q_imu, 4), _f64(t_pred, 3), _f64(q_pred, 4)
        r = self.res
        self.ctx._chk(self.lib.lili_frontend_frame(self.ctx.h, C.byref(cloud), curv_off, _ptr(qi), C.byref(self.livox), C.byref(self.params), C.byref(self.opt),
                                                   _ptr(tp), _ptr(qp), C.byref(r)))
        self.n_frames += 1
        info = dict(gn_status=r.gn_status, matched=bool(r.matched), n_edge=r.n_edge, n_surf=r.n_surf, n_query=r.n_query, n_map_raw=r.n_map_raw, n_map=r.n_map)
        if timing:
            info["stage_us"] = [r.stage_us[j] for j in range(4)]
        t, q = np.array(r.t[:], np.float64), np.array(r.q[:], np.float64)
        if q[0] < 0:
            q = -q                    # unifyQuaternion (L:538-548)
        return t, q, info


class RotFrontendOdometry(FrontendOdometry):
    """The same node behind the LOAM-style extractor of LiLi-OM-ROT (R/src/Preprocessing.cpp:248-535 + R/src/LidarOdometry.cpp:638-693): one lili_frontend_frame_rot call
    per spinning-LiDAR scan.  external_map = True: the call for a caller that keeps its own maps (the back end's matcher on one scan, BASELINE configs[0]) — the scan is
    matched against the indices set with ScanToMapMatcher.set_input_cloud, nothing joins the ring; edges = True: the edge features are queries too; leaf_query = 0: the
    surf features themselves are the queries."""

    flavour = VARIANT_ROT

    def __init__(self, ctx, params=None, n_scans=64, ds_rate=4, ds_v=0.6, near_range=3.0, q_lb=(1.0, 0, 0, 0), leaf_query=0.4, leaf_map=0.4, width=20, slot=0,
                 scan_match_cnt=6, first_match_cnt=8, reference_startup=True, external_map=False, edges=False):
        super().__init__(ctx, params, leaf_query=leaf_query, leaf_map=leaf_map, width=width, slot=slot, scan_match_cnt=scan_match_cnt, first_match_cnt=first_match_cnt,
                         reference_startup=reference_startup, external_map=external_map, edges=edges)
        self.rot = RotParams(n_scans, ds_rate, ds_v, near_range)
        self.q_lb = _f64(q_lb, 4)

    def frame(self, scan, t_pred, q_pred, q_imu=(1.0, 0, 0, 0), timing=False):
        """scan: (n,4) float32 rows x, y, z, intensity (host) or a Cloud (e.g. a device float4 array).  Returns (t, q, info)."""
        if isinstance(scan, Cloud):
            cloud = scan
        else:
            n = scan.shape[0]
            cloud = Cloud(scan.ctypes.data if n else None, n, 16, 12, MEM_HOST)
        k = self.n_frames
        if self.base_flags & FRAME_EXTERNAL_MAP:
            self.opt.n_iters, self.opt.flags = self.scan_match_cnt, self.base_flags
        else:
            self.opt.n_iters = 0 if k == 0 else (self.first_match_cnt if k == 1 else self.scan_match_cnt)
            self.opt.flags = (FRAME_PUSH_EMPTY if k == 0 else (FRAME_SELF_MAP if k == 1 else 0)) if self.reference_startup else 0
        self.opt.want_timing = 1 if timing else 0
        qi, tp, qp = _f64(q_imu, 4), _f64(t_pred, 3), _f64(q_pred, 4)
        r = self.res
        self.ctx._chk(self.lib.lili_frontend_frame_rot(self.ctx.h, C.byref(cloud), _ptr(qi), _ptr(self.q_lb), C.byref(self.rot), C.byref(self.params), C.byref(self.opt),
                                                       _ptr(tp), _ptr(qp), C.byref(r)))
        self.n_frames += 1
        info = dict(gn_status=r.gn_status, matched=bool(r.matched), n_edge=r.n_edge, n_surf=r.n_surf, n_query=r.n_query, n_map_raw=r.n_map_raw, n_map=r.n_map)
        if timing:
            info["stage_us"] = [r.stage_us[j] for j in range(4)]
        t, q = np.array(r.t[:], np.float64), np.array(r.q[:], np.float64)
        if q[0] < 0:
            q = -q                    # unifyQuaternion (R/src/LidarOdometry.cpp:524-534)
        return t, q, info


class BackendKeyframes:
    """Host-side mirror of what BackendFusion does per keyframe before ceres::Solve (L/src/BackendFusion.cpp:830-980, 1387-1528): ONE lili_backend_keyframe_prepare call —
    the keyframe of the previous solve joins both local-map rings, both maps are voxel-filtered and indexed, the new keyframe's features are down-sampled into the newest
    window slot, every keyframe of the window is associated.  Everything stays in HBM."""

    def __init__(self, ctx, params, leaf_surf=0.4, leaf_edge=0.2, width=40):
        self.ctx, self.lib, self.params = ctx, ctx.lib, params
        self.opt = BackendOptions(leaf_surf, leaf_edge, leaf_surf, leaf_edge, width, 0, -1)
        self.res = BackendResult()

    @staticmethod
    def _cloud(a):
        return a if isinstance(a, Cloud) else cloud_from_numpy(a, aux_col=3 if (np.ndim(a) == 2 and np.shape(a)[1] > 3) else None)

    def prepare(self, join, new_surf, new_edge, slots, ts_assoc, qs_assoc, timing=False):
        """join: None, (surf features, edge features, t, q) of the keyframe that joins the local map at its LiDAR pose, or (slot, t, q): the down-sampled features an earlier
        call left in that matcher slot (device to device); new_surf / new_edge: the new keyframe's features
        (numpy rows or Clouds); slots: the window, oldest first (the new keyframe takes slots[-1]).  Returns ([(n_surf, n_edge)] per slot, info)."""
        n = len(slots)
        arr = (C.c_int * n)(*[int(v) for v in slots])
        t = np.ascontiguousarray(np.asarray(ts_assoc, np.float64).reshape(n, 3)); q = np.ascontiguousarray(np.asarray(qs_assoc, np.float64).reshape(n, 4))
        counts = np.zeros((n, 2), np.int32)
        keep = [self._cloud(new_surf), self._cloud(new_edge)]
        js = je = tj = qj = None
        self.opt.join_slot = -1
        if join is not None and len(join) == 3:
            self.opt.join_slot = int(join[0])
            tj, qj = _f64(join[1], 3), _f64(join[2], 4)
        elif join is not None:
            keep += [self._cloud(join[0]), self._cloud(join[1])]
            js, je = C.byref(keep[2]), C.byref(keep[3])
            tj, qj = _f64(join[2], 3), _f64(join[3], 4)
        self.opt.want_timing = 1 if timing else 0
        r = self.res
        self.ctx._chk(self.lib.lili_backend_keyframe_prepare(self.ctx.h, js, je, _ptr(tj) if tj is not None else None, _ptr(qj) if qj is not None else None,
                                                             C.byref(keep[0]), C.byref(keep[1]), arr, n, _ptr(t), _ptr(q), C.byref(self.params), C.byref(self.opt), _ptr(counts),
                                                             C.byref(r)))
        info = dict(n_map_raw=tuple(r.n_map_raw), n_map=tuple(r.n_map), n_query=tuple(r.n_query), associated=bool(r.associated))
        if timing:
            info["stage_us"] = [r.stage_us[j] for j in range(3)]
        return [(int(counts[k, 0]), int(counts[k, 1])) for k in range(n)], info

    def repose(self, ts, qs):
        """Warm-up of the local map (while the reference's recent_surf_keyframes.size() < local_map_width, L/src/BackendFusion.cpp:1407-1443): the keyframes of both
        rings, oldest first, take the map-frame poses (keyframe_map_poses) the last solve gave them — before the next prepare, which pushes the joining keyframe at its own."""
        _repose(self.ctx, MASK_SURF | MASK_EDGE, ts, qs)


def window_sqrt_info(covariance):
    """sqrt_info = LLT(covariance^-1).matrixL()^T of an IMU factor as lili_window_evaluate / lili_window_solve compute it (host code, no GPU)."""
    cov = np.ascontiguousarray(np.asarray(covariance, np.float64).reshape(15, 15))
    out = np.zeros((15, 15))
    if load_library().lili_window_sqrt_info(_ptr(cov), _ptr(out)) != 0:
        raise LiliError("window_sqrt_info: the covariance is not positive definite")
    return out


def pack_preintegration(pre, g=None):
    """lili_window_imu from an object with a pre-integration's attributes: delta_p, delta_q (w x y z), delta_v, jacobian, covariance (15 x 15),
    linearized_ba, linearized_bg (or ba, bg), sum_dt; g: the gravity vector of the factor (default: pre.g_vec, else (0, 0, -9.805))."""
    w = WindowImu()
    w.sum_dt = float(pre.sum_dt)
    if g is None:
        g = getattr(pre, "g_vec", (0.0, 0.0, -9.805))
    ba = pre.linearized_ba if hasattr(pre, "linearized_ba") else pre.ba
    bg = pre.linearized_bg if hasattr(pre, "linearized_bg") else pre.bg
    for name, val, n in (("g", g, 3), ("delta_p", pre.delta_p, 3), ("delta_q", pre.delta_q, 4), ("delta_v", pre.delta_v, 3), ("lin_ba", ba, 3), ("lin_bg", bg, 3),
                         ("jacobian", pre.jacobian, 225), ("covariance", pre.covariance, 225)):
        a = np.asarray(val, np.float64).reshape(-1)
        if a.size != n:
            raise LiliError(f"pack_preintegration: {name} has {a.size} values, expected {n}")
        getattr(w, name)[:] = a.tolist()
    return w


def _pack_prior(prior):
    """(lili_window_prior, the arrays it points into) from the dict WindowSolver.set_problem(prior=...) takes"""
    wp = WindowPrior()
    kind = np.ascontiguousarray(prior["block_kind"], np.int32)
    kf = np.ascontiguousarray(prior["block_keyframe"], np.int32)
    x0 = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in prior["x0"]]) if isinstance(prior["x0"], (list, tuple)) else prior["x0"], np.float64)
    J0 = np.ascontiguousarray(prior["J0"], np.float64)
    r0 = np.ascontiguousarray(prior["r0"], np.float64)
    wp.n_rows, wp.n_cols, wp.n_blocks = J0.shape[0], int(prior.get("n_cols", J0.shape[1])), len(kind)
    wp.block_kind = kind.ctypes.data_as(C.POINTER(C.c_int32)); wp.block_keyframe = kf.ctypes.data_as(C.POINTER(C.c_int32))
    wp.x0 = x0.ctypes.data_as(C.POINTER(C.c_double)); wp.J0 = J0.ctypes.data_as(C.POINTER(C.c_double)); wp.r0 = r0.ctypes.data_as(C.POINTER(C.c_double))
    return wp, [kind, kf, x0, J0, r0]


def _prior_dict(st):
    """the dict set_problem(prior=...) takes, plus rank and sweeps, from a filled WindowPriorStorage"""
    rows, n, nb = st.prior.n_rows, st.prior.n_cols, st.prior.n_blocks
    kind = [int(st.block_kind[b]) for b in range(nb)]
    x0_all, x0, off = np.array(st.x0[:], np.float64), [], 0
    for k in kind:
        gs = (3, 4, 9)[k]
        x0.append(x0_all[off:off + gs].copy())
        off += gs
    return dict(block_kind=kind, block_keyframe=[int(st.block_keyframe[b]) for b in range(nb)], x0=x0,
                J0=np.array(st.J0[:rows * n], np.float64).reshape(rows, n), r0=np.array(st.r0[:rows], np.float64), rank=int(st.rank), sweeps=(int(st.sweeps_mm), int(st.sweeps_s)))


class WindowSolver:
    """The joint keyframe window on the device (lili_window_evaluate / lili_window_solve): lidar blocks of the matcher's slots + IMU factors + the
    marginalisation prior or the speed-bias priors.  A state is (n_kf, 16): t[3], q[4] (w x y z), speed-bias[9] per keyframe."""

    def __init__(self, ctx, matcher):
        self.ctx, self.lib, self.matcher = ctx, ctx.lib, matcher
        self._keep = []
        self.problem = None

    def set_problem(self, slots, kind_mask=MASK_SURF | MASK_EDGE, imu=None, prior=None, sb_prior=None, n_kf=None):
        """slots: matcher slot per keyframe (None with kind_mask 0); imu: n_kf - 1 WindowImu or pre-integration objects; prior: dict(block_kind,
        block_keyframe, x0, J0 (rows x cols), r0[, n_cols]); sb_prior: (n_kf, 9) means, a NaN row = no prior on that keyframe."""
        n_kf = int(n_kf if n_kf is not None else len(slots))
        pr = WindowProblem()
        keep = []
        pr.n_kf, pr.kind_mask = n_kf, int(kind_mask)
        if slots is not None:
            arr = (C.c_int32 * len(slots))(*[int(s) for s in slots])
            keep.append(arr)
            pr.slots = arr
        if imu is not None:
            arr = (WindowImu * len(imu))(*[f if isinstance(f, WindowImu) else pack_preintegration(f) for f in imu])
            if len(imu) != n_kf - 1:
                raise LiliError("WindowSolver: n_kf - 1 IMU factors expected")
            keep.append(arr)
            pr.imu = arr
        if prior is not None:
            wp, held = _pack_prior(prior)
            keep += [wp] + held
            pr.prior = C.pointer(wp)
        if sb_prior is not None:
            sb = np.ascontiguousarray(np.asarray(sb_prior, np.float64).reshape(n_kf, 9))
            keep.append(sb)
            pr.sb_prior = sb.ctypes.data_as(C.POINTER(C.c_double))
        self._keep, self.problem = keep, pr
        return self

    def _state(self, state):
        s = np.ascontiguousarray(np.asarray(state, np.float64).reshape(-1, 16)).copy()
        if self.problem is None or s.shape[0] != self.problem.n_kf:
            raise LiliError("WindowSolver: set_problem first, state must be (n_kf, 16)")
        return s

    def evaluate(self, state, want_jtj=True):
        """(cost, gradient[15 n_kf], JtJ[15 n_kf, 15 n_kf] or None) in local coordinates at `state`."""
        s = self._state(state)
        n = 15 * s.shape[0]
        cost, g = np.zeros(1), np.zeros(n)
        H = np.zeros((n, n)) if want_jtj else None
        self.ctx._chk(self.lib.lili_window_evaluate(self.ctx.h, C.byref(self.problem), C.byref(self.matcher.params), _ptr(s), _ptr(cost), _ptr(g), _ptr(H)))
        return float(cost[0]), g, H

    def solve(self, state, options=None, want_summary=True, summary=None):
        """ceres::Solve on the window, one persistent launch: (final state (n_kf, 16), summary dict) — or (None, None) asynchronously
        (want_summary=False; last_state() fetches the state later).  summary: an LmSummary of the caller's to fill instead of a new one."""
        s = self._state(state)
        sm = summary if summary is not None else LmSummary() if want_summary else None
        self.ctx._chk(self.lib.lili_window_solve(self.ctx.h, C.byref(self.problem), C.byref(self.matcher.params), C.byref(options) if options is not None else None,
                                                 _ptr(s), C.byref(sm) if sm is not None else None))
        return (s, sm.as_dict()) if sm is not None else (None, None)

    def last_state(self):
        s = np.zeros((self.problem.n_kf, 16))
        self.ctx._chk(self.lib.lili_window_state_get(self.ctx.h, self.problem.n_kf, _ptr(s)))
        return s

    def marginalize(self, state, storage=None):
        """The NEXT window's prior from this problem at the solved `state` (lili_window_marginalize: keyframe 0 marginalised, the reference's factor
        set): the dict set_problem(prior=...) takes — block_kind, block_keyframe (already in the next window's numbering), x0 (list per block), J0, r0 —
        plus rank and sweeps (of the two Jacobi decompositions).  storage: a WindowPriorStorage of the caller's to fill (its .prior is the C view); untouched when the call is refused."""
        s = self._state(state)
        st = storage if storage is not None else WindowPriorStorage()
        self.ctx._chk(self.lib.lili_window_marginalize(self.ctx.h, C.byref(self.problem), C.byref(self.matcher.params), _ptr(s), C.byref(st)))
        return _prior_dict(st)

    def cycle(self, state, options=None, gates=None, use_resident_prior=False, result=None):
        """One keyframe's solve, sign unification, next prior and write-back gates in one call (lili_window_cycle).  gates: a WindowCycleOptions or a dict of
        gate_p / gate_q / gate_v / gate_ba / gate_bg (default: the reference's 10, 10, 10, 22, 22); use_resident_prior: the problem's prior is the one the previous
        cycle left on the device (set_problem then carries none).  Returns dict(summary, solved, abs_state, next_state (each (n_kf, 16)), refused (n_kf bit masks:
        bit 0 p, 1 q, 2 v, 3..5 ba, 6..8 bg), prior_updated, prior_n, prior_blocks, rank, sweeps).  result: a WindowCycleResult of the caller's to fill; untouched
        when the call is refused."""
        s = self._state(state)
        co = gates if isinstance(gates, WindowCycleOptions) else WindowCycleOptions(**(gates or {}))
        co.use_resident_prior = 1 if use_resident_prior else 0
        res = result if result is not None else WindowCycleResult()
        self.ctx._chk(self.lib.lili_window_cycle(self.ctx.h, C.byref(self.problem), C.byref(self.matcher.params), C.byref(options) if options is not None else None,
                                                 C.byref(co), _ptr(s), C.byref(res)))
        n = s.shape[0]
        return dict(summary=res.summary.as_dict(), solved=np.array(res.solved[:16 * n], np.float64).reshape(n, 16), abs_state=np.array(res.abs_state[:16 * n], np.float64).reshape(n, 16),
                    next_state=np.array(res.next_state[:16 * n], np.float64).reshape(n, 16), refused=[int(res.refused[k]) for k in range(n)],
                    prior_updated=bool(res.prior_updated), prior_n=int(res.prior_n), prior_blocks=int(res.prior_blocks), rank=int(res.rank),
                    sweeps=(int(res.sweeps_mm), int(res.sweeps_s)))

    def reset_cycle(self):
        """drops the resident prior (after a loop closure the reference starts again without one)"""
        self.ctx._chk(self.lib.lili_window_cycle_reset(self.ctx.h))

    def resident_prior(self, storage=None):
        """a copy of the resident prior as marginalize() returns one; LiliError when there is none"""
        st = storage if storage is not None else WindowPriorStorage()
        self.ctx._chk(self.lib.lili_window_prior_get(self.ctx.h, C.byref(st)))
        return _prior_dict(st)

    def set_resident_prior(self, prior):
        """seeds the resident prior from a dict as set_problem(prior=...) takes (a restart from a saved prior)"""
        wp, held = _pack_prior(prior)
        self.ctx._chk(self.lib.lili_window_prior_set(self.ctx.h, C.byref(wp)))
        del held


def marg_schur(ctx, A, b, m):
    """(J0 (n, n), r0 (n), rank) of lili_marg_schur: the first m dimensions of the symmetric system A (pos, pos), b are marginalised on the device, n = pos - m
    (MarginalizationFactor.cpp:176-201).  Only J0^T J0, J0^T r0, r0^T r0 and the rank are independent of the eigenvector basis."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or b.shape[0] != A.shape[0]:
        raise LiliError("marg_schur: A must be square and b as long")
    pos, m = A.shape[0], int(m)
    n = max(pos - m, 0) if m >= 0 else 0
    J0, r0, rank = np.full((n, n), np.nan), np.full(n, np.nan), C.c_int(-1)
    ctx._chk(ctx.lib.lili_marg_schur(ctx.h, _ptr(A), pos, _ptr(b), pos, m, _ptr(J0) if n else None, _ptr(r0) if n else None, C.byref(rank)))
    return J0, r0, rank.value


def gn_step_host(gram, t, q):
    lib = load_library()
    g = _f64(gram, 64)
    t = _f64(t, 3).copy()
    q = _f64(q, 4).copy()
    d = np.zeros(6)
    st = lib.lili_gn_step_host(_ptr(g), _ptr(t), _ptr(q), _ptr(d))
    return st, t, q, d


def gram_to_factor(gram, cost):
    """(residuals[9], jacobian[9,7]) of the ceres adapter block (include/lili_ceres_adapter.h)."""
    lib = load_library()
    g = _f64(gram, 64)
    res = np.zeros(9)
    jac = np.zeros(63)
    rc = lib.lili_gram_to_factor(_ptr(g), float(cost), _ptr(res), _ptr(jac))
    if rc != OK:
        raise LiliError(f"lili_gram_to_factor failed ({rc})")
    return res, jac.reshape(9, 7)


def assoc_transform(t, q, params):
    """(Q2, T2) = (Q * q_lb^-1, T - Q2 * t_lb): L/src/BackendFusion.cpp:929-930 (host-side pose algebra)."""
    q = np.asarray(q, np.float64)
    qlb = np.array(list(params.q_lb))
    tlb = np.array(list(params.t_lb))
    n2 = float((qlb * qlb).sum())
    qi = np.array([qlb[0], -qlb[1], -qlb[2], -qlb[3]]) / n2
    a, b = q, qi
    Q2 = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                   a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                   a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                   a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])
    u = Q2[1:4]
    uv = 2 * np.cross(u, tlb)
    rot = tlb + Q2[0] * uv + np.cross(u, uv)
    return Q2, np.asarray(t, np.float64) - rot


def keyframe_map_pose(t_po, q_po, t_bl, q_bl):
    """Pose a stored keyframe's features are moved by when they enter the local map: (q_po * q_bl, q_po * t_bl + t_po),
    L/src/BackendFusion.cpp:1425-1426, 1462-1463 (host-side pose algebra, f64).  Returns (t, q) as LocalMap.push takes them."""
    a, b = np.asarray(q_po, np.float64), np.asarray(q_bl, np.float64)
    q = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                  a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                  a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                  a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])
    u, v = a[1:4], np.asarray(t_bl, np.float64)
    uv = np.cross(u, v)
    uv = uv + uv
    return (v + uv * a[0]) + np.cross(u, uv) + np.asarray(t_po, np.float64), q


def keyframe_map_poses(ts_po, qs_po, t_bl, q_bl):
    """keyframe_map_pose of every keyframe of a ring (body poses (n, 3) / (n, 4) wxyz, oldest first): the (n, 3), (n, 4) arrays LocalMap.repose and
    BackendKeyframes.repose take — Ttmp of the warm-up branch, L/src/BackendFusion.cpp:1413-1436."""
    out = [keyframe_map_pose(t, q, t_bl, q_bl) for t, q in zip(np.asarray(ts_po, np.float64).reshape(-1, 3), np.asarray(qs_po, np.float64).reshape(-1, 4))]
    return np.array([o[0] for o in out]).reshape(-1, 3), np.array([o[1] for o in out]).reshape(-1, 4)


def body_pose_from_lidar(t_lidar, q_lidar, params):
    """Body pose (T, Q) whose association transform (Q*q_lb^-1, T - Q2*t_lb) equals the given LiDAR pose
    (up to the non-unit norm of the configured q_lb, which the reference does not normalise either)."""
    qlb = np.array(list(params.q_lb))
    qn = qlb / np.linalg.norm(qlb)
    a, b = np.asarray(q_lidar, np.float64), qn
    Q = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                  a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                  a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                  a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])
    _, T2 = assoc_transform([0.0, 0.0, 0.0], Q, params)
    return np.asarray(t_lidar, np.float64) - T2, Q


# ------------------------------------------------------------------------------------------------
# callers / data formats either side of the path
# ------------------------------------------------------------------------------------------------
CUSTOM_POINT = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                         ("reflectivity", "u1"), ("tag", "u1"), ("line", "u1")])   # livox_ros_driver/CustomPoint, 19 B


def livox_custom_to_cloud(ctx, points):
    """Livox CustomMsg points (CUSTOM_POINT array or raw bytes, 19 B each) -> (n, 12) float32 PointXYZINormal rows
    (L/src/FormatConvert.cpp:11-35), converted on the device."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=CUSTOM_POINT))
    n = pts.shape[0]
    out = np.zeros((n, 12), np.float32)
    ctx._chk(ctx.lib.lili_livox_custom_to_cloud(ctx.h, pts.ctypes.data if n else None, n, CUSTOM_POINT.itemsize, MEM_HOST,
                                                out.ctypes.data if n else None, MEM_HOST))
    return out


class ImuState(C.Structure):
    _fields_ = [("idx", C.c_int64), ("t_cur", C.c_double), ("gyr0", C.c_double * 3), ("first", C.c_int32), ("reserved", C.c_int32)]


class ImuIntegrator:
    """Host-side gyro integration over one scan (L/src/Preprocessing.cpp:129-171); returns q_imu (w,x,y,z)."""

    def __init__(self):
        self.lib = load_library()
        self.state = ImuState()
        self.lib.lili_imu_reset(C.byref(self.state))

    def integrate(self, stamps, gyr, t_scan_next):
        st = np.ascontiguousarray(stamps, dtype=np.float64)
        g = np.ascontiguousarray(gyr, dtype=np.float64).reshape(-1, 3)
        q = np.zeros(4, np.float64)
        rc = self.lib.lili_imu_integrate(C.byref(self.state), st.ctypes.data if st.size else None, g.ctypes.data if g.size else None,
                                         st.shape[0], float(t_scan_next), q.ctypes.data)
        if rc != 0:
            raise LiliError(f"lili_imu_integrate failed ({rc})")
        return q


IMU_MAX_SAMPLES, IMU_MAX_SEGMENTS = 4096, 64


class ImuPreintegrator:
    """IMU pre-integration on the device (lili_imu_preintegrate) and the keyframe sample slicing in front of it (lili_imu_keyframe_samples, host code).
    A segment is a dict: dt (n), acc (n, 3), gyr (n, 3) — push_back's arguments —, acc0, gyr0, ba, bg — the constructor's —, optionally g (default
    (0, 0, -9.805)) and, for a prediction, P0 (3), R0 (3, 3), V0 (3).  ctx may be None for keyframe_samples alone."""

    def __init__(self, ctx=None):
        self.ctx, self.lib = ctx, ctx.lib if ctx is not None else load_library()
        self.state = ImuKfState()
        self.lib.lili_imu_kf_reset(C.byref(self.state))

    def reset(self):
        self.lib.lili_imu_kf_reset(C.byref(self.state))

    def keyframe_samples(self, stamps, acc, gyr, t_kf, cap=None):
        """The segment of the keyframe stamped t_kf from the sample buffer (stamps (n), acc / gyr (n, 3); the running state remembers what is consumed):
        dict(dt, acc, gyr, acc0, gyr0) — preintegrate's segment once ba / bg are added.  cap: rows the outputs may hold (default: enough)."""
        st = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        a = np.ascontiguousarray(acc, np.float64).reshape(-1, 3)
        g = np.ascontiguousarray(gyr, np.float64).reshape(-1, 3)
        if not (st.shape[0] == a.shape[0] == g.shape[0]):
            raise LiliError("keyframe_samples: stamps, acc and gyr differ in length")
        cap = int(cap if cap is not None else max(st.shape[0] - int(self.state.idx), 0) + 1)
        dt_o, a_o, g_o = np.zeros(cap), np.zeros((cap, 3)), np.zeros((cap, 3))
        n_out = C.c_size_t(0)
        was_first = bool(self.state.first)
        acc0, gyr0 = np.array(self.state.acc0[:]), np.array(self.state.gyr0[:])
        rc = self.lib.lili_imu_keyframe_samples(C.byref(self.state), _ptr(st) if st.size else None, _ptr(a) if a.size else None, _ptr(g) if g.size else None, st.shape[0],
                                                float(t_kf), _ptr(dt_o), _ptr(a_o), _ptr(g_o), cap, C.byref(n_out))
        if rc != 0:
            raise LiliError(f"lili_imu_keyframe_samples failed ({rc})")
        if not was_first and st.size:      # a fresh state took the constructor's pair from the first sample
            acc0, gyr0 = a[0].copy(), g[0].copy()
        n = int(n_out.value)
        return dict(dt=dt_o[:n].copy(), acc=a_o[:n].copy(), gyr=g_o[:n].copy(), acc0=acc0, gyr0=gyr0)

    def _pack(self, segments, predict=False):
        """(ctypes array of lili_imu_segment, the arrays it points into, per-segment predict flags); a segment's own "predict" key overrides the argument"""
        n_seg = len(segments)
        segs = (ImuSegment * max(n_seg, 1))()
        keep, flags = [], []
        for s, d in zip(segs, segments):
            dt = np.ascontiguousarray(d["dt"], np.float64).reshape(-1)
            a = np.ascontiguousarray(d["acc"], np.float64).reshape(-1, 3)
            g = np.ascontiguousarray(d["gyr"], np.float64).reshape(-1, 3)
            if not (dt.shape[0] == a.shape[0] == g.shape[0]):
                raise LiliError("preintegrate: dt, acc and gyr differ in length")
            keep += [dt, a, g]
            flags.append(bool(d.get("predict", predict)))
            s.n, s.predict = dt.shape[0], 1 if flags[-1] else 0
            if dt.size:
                s.dt, s.acc, s.gyr = (x.ctypes.data_as(C.POINTER(C.c_double)) for x in (dt, a, g))
            for name, key, size, default in (("acc0", "acc0", 3, None), ("gyr0", "gyr0", 3, None), ("lin_ba", "ba", 3, None), ("lin_bg", "bg", 3, None), ("g", "g", 3, (0.0, 0.0, -9.805)),
                                             ("P0", "P0", 3, (0.0,) * 3), ("R0", "R0", 9, (1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)), ("V0", "V0", 3, (0.0,) * 3)):
                v = np.asarray(d[key] if default is None else d.get(key, default), np.float64).reshape(-1)
                if v.size != size:
                    raise LiliError(f"preintegrate: {key} has {v.size} values, expected {size}")
                getattr(s, name)[:] = v.tolist()
        return segs, keep, flags

    def preintegrate(self, segments, predict=False):
        """WindowImu array (one per segment, what WindowSolver.set_problem(imu=...) takes) — and, if any segment predicts, the list of
        (P1 (3), R1 (3, 3), V1 (3)) per segment (None where a segment does not)."""
        if self.ctx is None:
            raise LiliError("ImuPreintegrator: preintegrate needs a context")
        n_seg = len(segments)
        segs, keep, flags = self._pack(segments, predict)
        out = (WindowImu * max(n_seg, 1))()
        pred = (ImuPrediction * max(n_seg, 1))() if any(flags) else None
        self.ctx._chk(self.lib.lili_imu_preintegrate(self.ctx.h, segs, n_seg, out, pred))
        if pred is None:
            return out
        return out, [(np.array(p.P1[:]), np.array(p.R1[:]).reshape(3, 3), np.array(p.V1[:])) if f else None for p, f in zip(pred, flags)]

    def kernel_ms(self):
        ms = C.c_float(0)
        self.ctx._chk(self.lib.lili_imu_kernel_ms(self.ctx.h, C.byref(ms)))
        return float(ms.value)


def marg_add_lidar(gram, A, b, idx_t, idx_q):
    """Adds the lidar blocks of one keyframe's Gram record into MarginalizationInfo's dense A (pos x pos, C order), b."""
    lib = load_library()
    G = np.ascontiguousarray(gram, dtype=np.float64).reshape(64)
    assert A.flags.c_contiguous and A.dtype == np.float64 and b.dtype == np.float64 and A.shape[0] == A.shape[1] == b.shape[0]
    rc = lib.lili_marg_add_lidar(G.ctypes.data, A.ctypes.data, A.shape[1], b.ctypes.data, A.shape[0], int(idx_t), int(idx_q))
    if rc != 0:
        raise LiliError(f"lili_marg_add_lidar failed ({rc})")
    return A, b
