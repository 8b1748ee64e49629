"""Pins against the REFERENCE'S OWN code: tests/golden/ref_*.npz were produced by oracle/_ref — the reference's
Preprocessing.cpp (both flavours) and LidarKeyframeFactor.h compiled unmodified from /root/reference against the stand-in
third-party headers of oracle/refshim/ (generator: tests/golden/make_ref_golden.py).

  * where oracle/_ref is present (the build container) it must still reproduce the committed fixtures bit for bit;
  * the oracle restatement (oracle/lo_extract.cpp, lo_s2m.cpp, oracle.ImuIntegrator) must reproduce them bit for bit in
    its literal mode — this is what turns "parity unpinned" into "pinned to the reference's own statements" for the
    extractors and the factor functors (third-party arithmetic — Eigen quaternions / eigen-solver, PCL VoxelGrid, Ceres Jets —
    is shared between shim and oracle and stays an App. B assumption);
  * the product's host-side gyro integration (lili_imu_integrate) feeds the same chain.
"""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(G, "make_ref_golden.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_npz(d, g):
    assert set(d) == set(g.files)
    for k in g.files:
        a, b = np.asarray(d[k]), g[k]
        if a.dtype.kind == "f":
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
        else:
            assert np.array_equal(a, b), k


# ------------------------------------------------------------------ the reference build itself
@pytest.mark.parametrize("which", ["rot", "rot_cases", "livox", "factors", "frontend", "frontend_R", "backend", "format", "marg", "localmap"])
def test_reference_build_reproduces_fixtures(which):
    if not M.R.available():
        pytest.skip("oracle/_ref not built (needs /root/reference; build container only)")
    d = {"rot": M.run_rot, "rot_cases": M.run_rot_cases, "livox": M.run_livox, "factors": M.run_factors, "frontend": M.run_frontend, "frontend_R": M.run_frontend_rot, "backend": M.run_backend, "format": M.run_format,
         "marg": M.run_marg, "localmap": M.run_localmap}[which]()
    _same_npz(d, np.load(os.path.join(G, f"ref_{which}.npz")))


# ------------------------------------------------------------------ oracle vs reference
def _q_imu_per_scan(integrator, stamps, imu_t, gyr, k):
    # scan k is processed when cloud k+2 arrives: the node has seen every IMU sample up to that stamp and
    # integrates up to the stamp of cloud k+1 (time_scan_next)
    m = imu_t <= stamps[k + 2]
    return integrator.integrate(imu_t[m], gyr[m], stamps[k + 1])


def test_oracle_equals_reference_rot(oracle):
    g = np.load(os.path.join(G, "ref_rot.npz"))
    scans, stamps, imu_t, gyr = M.rot_inputs()
    integ = oracle.ImuIntegrator()
    assert int(g["n_processed"]) == 2
    for k in range(2):
        q_imu = _q_imu_per_scan(integ, stamps, imu_t, gyr, k)
        assert abs(np.linalg.norm(q_imu[1:])) > 1e-3            # the deskew is exercised
        r = oracle.extract_rot(scans[k], q_imu, M.ROT_QLB, oracle.rot_params(ds_rate=4, atan_mode=0, stable_sort=0))
        assert float(g[f"stamp{k}"]) == stamps[k]
        assert np.array_equal(_bits(r["full"]), _bits(g[f"cutted{k}"]))                      # /lidar_cloud_cutted
        assert np.array_equal(_bits(r["full"][r["edge_idx"]]), _bits(g[f"edge{k}"]))         # /edge_features
        assert np.array_equal(_bits(r["surf"]), _bits(g[f"surf{k}"]))                        # /surf_features
        assert len(r["edge_idx"]) > 100 and len(r["surf"]) > 500
        # the GPU path's definition (f64 atan rounded to f32, index tie-break, in-order centroids) picks the same
        # features on this data and differs from the literal one only in centroid rounding
        d = oracle.extract_rot(scans[k], q_imu, M.ROT_QLB, oracle.rot_params(ds_rate=4, atan_mode=1, stable_sort=1))
        assert np.array_equal(d["full_src"], r["full_src"]) and np.array_equal(d["edge_idx"], r["edge_idx"])
        assert np.array_equal(d["surf_cnt"], r["surf_cnt"])
        np.testing.assert_allclose(d["surf"], g[f"surf{k}"], rtol=2e-6, atol=2e-5)
        # the feature indices the reference run pushed (row match of /edge_features in /lidar_cloud_cutted, make_ref_golden.py)
        assert np.array_equal(r["edge_idx"], g[f"edge_src{k}"])
        # glibc's float atan / atan2 restated (lo_math.h fd_atanf / fd_atan2f — what the HIP extractor runs by default): the SAME bits
        # as the libm the reference build called, in every published cloud
        f = oracle.extract_rot(scans[k], q_imu, M.ROT_QLB, oracle.rot_params(ds_rate=4, atan_mode=2, stable_sort=0))
        for key in ("full", "surf"):
            assert np.array_equal(_bits(f[key]), _bits(r[key])), key
        assert np.array_equal(f["edge_idx"], r["edge_idx"]) and np.array_equal(f["label"], r["label"])


def test_oracle_equals_reference_rot_cases(oracle):
    """The designed scans of tests/rot_cases.py — both endOri corrections, the four wrap branches, early and missing latches, relTime outside [0, 1], the three ring
    tables at every id boundary, rings of 0 .. 24 600 points, picks at their caps and across segment borders, voxels, the slerp's branches — as the reference's own
    Preprocessing.cpp published them (tests/golden/ref_rot_cases.npz): the oracle's literal mode gives every cloud bit for bit, and where no two curvatures of a
    segment are equal, the definition the HIP extractor follows (glibc's float atan / atan2 restated, index tie-break, in-order centroids) picks the same features."""
    g = np.load(os.path.join(G, "ref_rot_cases.npz"))
    cases = M.rot_cases()
    assert len(cases) >= 50 and {k.split("/")[0] for k in g.files} == {c["name"] for c in cases}
    n_src = 0
    for c in cases:
        _, stamps, imu_t, gyr = M.rot_case_inputs(c)
        q_imu = _q_imu_per_scan(oracle.ImuIntegrator(), stamps, imu_t, gyr, 0)      # every case is a run of its own
        assert abs(np.linalg.norm(q_imu[1:])) > 1e-3            # the deskew is exercised
        P = dict(n_scans=c["n_scans"], ds_rate=c["ds_rate"])
        r = oracle.extract_rot(c["raw"], q_imu, c["q_lb"], oracle.rot_params(atan_mode=0, stable_sort=0, **P))
        k = c["name"]
        for name, a in (("cutted", r["full"]), ("edge", r["full"][r["edge_idx"]]), ("surf", r["surf"])):     # /lidar_cloud_cutted, /edge_features, /surf_features
            assert a.shape[0] == int(g[f"{k}/{name}_n"]), (k, name)
            assert np.array_equal(_bits(a[::M.cloud_stride(a.shape[0])]), _bits(g[f"{k}/{name}_rows"])), (k, name)
            assert _sha(np.ascontiguousarray(a, np.float32)) == str(g[f"{k}/{name}_sha"]), (k, name)
        if f"{k}/edge_src" in g.files:                           # the indices the reference run pushed
            assert np.array_equal(r["edge_idx"], g[f"{k}/edge_src"]), k
            n_src += 1
        if r["n_ties"] == 0:
            d = oracle.extract_rot(c["raw"], q_imu, c["q_lb"], oracle.rot_params(atan_mode=2, stable_sort=1, **P))
            assert np.array_equal(_bits(d["full"]), _bits(r["full"])) and np.array_equal(d["full_src"], r["full_src"]), k
            assert np.array_equal(d["edge_idx"], r["edge_idx"]) and np.array_equal(d["label"], r["label"]) and np.array_equal(d["surf_cnt"], r["surf_cnt"]), k
            np.testing.assert_allclose(d["surf"], r["surf"], rtol=2e-6, atol=2e-5)
    assert n_src >= 50


def test_oracle_equals_reference_livox(oracle):
    g = np.load(os.path.join(G, "ref_livox.npz"))
    scans, stamps, imu_t, gyr = M.livox_inputs()
    integ = oracle.ImuIntegrator()
    for k in range(2):
        q_imu = _q_imu_per_scan(integ, stamps, imu_t, gyr, k)
        r = oracle.extract_livox(scans[k], q_imu)
        for name in ("cutted", "surf"):
            a = r[name]
            assert a.shape[0] == int(g[f"{name}{k}_n"])
            assert _sha(a[:, [0, 1, 2, 6, 7]]) == str(g[f"{name}{k}_sha_payload"])
            assert _sha(np.abs(a[:, 3:6])) == str(g[f"{name}{k}_sha_absn"])
            s = g[f"{name}{k}_every8"]
            assert np.array_equal(_bits(np.abs(a[::8])), _bits(np.abs(s)))
        e, ge = r["edge"], g[f"edge{k}"]
        assert e.shape == ge.shape and e.shape[0] > 10
        assert np.array_equal(_bits(e[:, [0, 1, 2, 6, 7]]), _bits(ge[:, [0, 1, 2, 6, 7]]))
        assert np.array_equal(_bits(np.abs(e[:, 3:6])), _bits(np.abs(ge[:, 3:6])))


def test_oracle_equals_reference_factors(oracle):
    """LidarEdgeFactor / LidarPlaneNormFactor / LidarPlaneNormIncreFactor through Create()->Evaluate() vs the oracle's
    dual-number evaluation (lo_eval_edge / lo_eval_plane)."""
    g = np.load(os.path.join(G, "ref_factors.npz"))
    f = M.factor_inputs()
    P = oracle.params("rot", q_lb=f["qlb"], t_lb=f["tlb"])
    n = f["cp"].shape[0]
    worst = 0.0
    for i in range(n):
        e = oracle.eval_edge(f["t"][i], f["q"][i], f["cp"][i], f["a"][i], f["b"][i], f["s"][i])       # J(7), r
        p = oracle.eval_plane(f["t"][i], f["q"][i], f["cp"][i], f["n"][i], f["d"][i], f["s"][i], P)
        pi = oracle.eval_plane(f["t"][i], f["q"][i], f["cp"][i], f["n"][i], f["d"][i], 1.0, P, frontend=True)
        ref_e, ref_p, ref_pi = g["edge"][i], g["plane"][i], g["plane_incre"][i]
        for mine, ref in ((np.r_[e[7], e[0:7]], ref_e), (np.r_[p[7], p[0:7]], ref_p),
                          (np.r_[pi[7], pi[3:7], pi[0:3]], ref_pi)):             # Incre: parameter order (q, t)
            worst = max(worst, np.abs(mine - ref).max())
    assert worst == 0.0, worst          # bit-exact, incl. the Jet-style q_lb inverse of the plane factor


# ------------------------------------------------------------------ front-end node (LidarOdometry.cpp) vs oracle
def _frontend_surf_features(oracle):
    frames, stamps, imu_t, gyr = M.frontend_inputs()
    integ = oracle.ImuIntegrator()
    return [oracle.extract_livox(frames[k], _q_imu_per_scan(integ, stamps, imu_t, gyr, k))["surf"][:, [0, 1, 2, 7]]
            for k in range(M.FRONTEND_FRAMES)]


def test_oracle_association_equals_reference_frontend(oracle):
    """findCorrespondingSurfFeatures + LidarPlaneNormIncreFactor + HuberLoss as the reference's node ran them (three solves
    stored completely): the oracle builds the same correspondence records (cp, weight*n, weight*d: bit-exact), the same raw
    residual/Jacobian rows, and the same Gauss-Newton step."""
    g = np.load(os.path.join(G, "ref_frontend.npz"))
    PO = oracle.params("frontend")
    for i in M.FRONTEND_FULL_SOLVES:
        mp, qs, rec, rows = (g[f"solve{i}_{k}"] for k in ("map", "queries", "records", "rows"))
        assert _sha(mp) == str(g["map_sha"][i]) and _sha(rec) == str(g["records_sha"][i])
        q, t = g["pose_in"][i][:4], g["pose_in"][i][4:]
        rs = oracle.associate_surf(oracle.KdTree(np.ascontiguousarray(mp[:, :3])), None, np.ascontiguousarray(qs[:, :3]), None, q, t, PO)
        v = rs["valid"].astype(bool)
        mine = np.c_[rs["cp"][v], rs["n"][v], rs["d"][v]].astype(np.float64)
        assert mine.shape == rec.shape and np.array_equal(mine, rec) and rec.shape[0] > 1000
        for k in range(0, rec.shape[0], 37):          # raw rows: reference (r, dq4, dt3) vs oracle (J: t3 q4, r)
            o = oracle.eval_plane(t, q, rec[k, 0:3], rec[k, 3:6], rec[k, 6], 1.0, PO, frontend=True)
            assert np.array_equal(np.r_[o[7], o[3:7], o[0:3]], rows[k]), k
        Gm, _, _ = oracle.linearize_surf(rs, t, q, PO)
        st, t2, q2, _ = oracle.gn_step(Gm, t, q)
        assert st == 0 and np.array_equal(np.r_[q2, t2], g["pose_out"][i])


def test_frontend_chain_on_oracle_equals_reference_node(oracle):
    """The whole front-end loop (tests/frontend_chain.py on oracle primitives, literal PCL mode) reproduces the poses of the
    reference's LidarOdometry node bit for bit over the sequence, and every solve's pose and residual-block count;
    the GPU path's definition (in-order voxel centroids) stays within 1e-5."""
    from tests import frontend_chain as F
    g = np.load(os.path.join(G, "ref_frontend.npz"))
    surf = _frontend_surf_features(oracle)
    be = F.OracleBackend(oracle, stable=False)
    a, r = F.run_frontend_chain(be, surf, scan_match_cnt=int(M.FRONTEND_PARAMS["/lidar_odometry/scan_match_cnt"]))
    assert np.array_equal(a, g["abs_pose"]) and np.array_equal(r, g["rel_pose"])
    assert len(be.log) == int(g["n_solves"])
    assert [l["n_blocks"] for l in be.log] == list(g["n_blocks"]) and [l["n_map"] for l in be.log] == list(g["n_map"])
    assert all(np.array_equal(l["pose_out"], g["pose_out"][i]) for i, l in enumerate(be.log))
    assert np.linalg.norm(a[-1][4:] - a[1][4:]) > 1.5           # the sensor really moved (0.5 m per frame)
    a2, _ = F.run_frontend_chain(F.OracleBackend(oracle, stable=True), surf, scan_match_cnt=6)
    assert np.abs(a2 - g["abs_pose"]).max() < 1e-5


def test_frontend_chain_on_oracle_equals_reference_rot_node(oracle):
    """Round 6 (VERDICT r5 #3b): the ROT package's odometry node — LiLi-OM-ROT/src/LidarOdometry.cpp compiled as is behind its own Preprocessing node, 64-ring scans
    of a moving sensor (tests/golden/ref_frontend_R.npz) — is reproduced by the oracle's ROT extractor + the same front-end loop bit for bit: poses, every solve's pose and
    residual-block count.  The ROT node had been pinned by analogy with the Livox package's file only."""
    from tests import frontend_chain as F
    g = np.load(os.path.join(G, "ref_frontend_R.npz"))
    scans, stamps, imu_t, gyr = M.frontend_rot_inputs()
    rp = oracle.rot_params(ds_rate=4, atan_mode=2, stable_sort=0)
    feats = [oracle.extract_rot(scans[k], (1.0, 0, 0, 0), M.ROT_QLB, rp) for k in range(M.FRONTEND_R_FRAMES)]
    assert [f["surf"].shape[0] for f in feats] == list(g["n_surf"]) and [len(f["edge_idx"]) for f in feats] == list(g["n_edge"])
    surf = [np.ascontiguousarray(f["surf"][:, :4]) for f in feats]
    be = F.OracleBackend(oracle, stable=False)
    a, r = F.run_frontend_chain(be, surf, scan_match_cnt=int(M.FRONTEND_R_PARAMS["/lidar_odometry/scan_match_cnt"]))
    assert np.array_equal(a, g["abs_pose"]) and np.array_equal(r, g["rel_pose"])
    assert len(be.log) == int(g["n_solves"])
    assert [l["n_blocks"] for l in be.log] == list(g["n_blocks"]) and [l["n_map"] for l in be.log] == list(g["n_map"])
    assert all(np.array_equal(l["pose_out"], g["pose_out"][i]) for i, l in enumerate(be.log))
    assert np.linalg.norm(a[-1][4:] - a[1][4:]) > 1.5


# ------------------------------------------------------------------ back-end matcher (BackendFusion.cpp slices) vs oracle
def _sorted_ab(e):
    """edge records with (A, B) in a canonical order: A = c + 0.1 v, B = c - 0.1 v and the sign of an eigenvector is arbitrary"""
    a, b = e[:, 3:6].copy(), e[:, 6:9].copy()
    swap = np.array([tuple(x) > tuple(y) for x, y in zip(a, b)])
    a[swap], b[swap] = e[swap, 6:9], e[swap, 3:6]
    return np.c_[e[:, 0:3], a, b, e[:, 9:10]]


@pytest.mark.parametrize("flavour", ["livox", "rot"])
def test_oracle_association_equals_reference_backend(oracle, flavour):
    """transformPoint + findCorrespondingSurfFeatures + findCorrespondingCornerFeatures of the reference's back-end (both
    flavours: reflectivity-weighted LS and score for Livox, point-to-line gate for ROT) and the residual blocks built from
    them (count scaling with the reference's float / double promotions for ROT): records and raw rows bit-exact."""
    g = np.load(os.path.join(G, "ref_backend.npz"))
    i = M.backend_inputs(flavour)
    PO = oracle.params(flavour)
    B = M.BACKEND_PARAMS[flavour]
    assert (PO.kd_max_radius, PO.surf_dist_thres, PO.lidar_const, PO.reflect_thres) == (B["kd_max_radius"], B["surf_dist_thres"], B["lidar_const"], B["reflect_thres"])
    assert list(PO.q_lb) == B["q_lb"] and list(PO.t_lb) == B["t_lb"]
    assert np.array_equal(i["Q2"], g[f"{flavour}_Q2"]) and np.array_equal(i["t0"], g[f"{flavour}_t0"])
    refl = flavour == "livox"
    rs = oracle.associate_surf(oracle.KdTree(np.ascontiguousarray(i["surf_map"][:, :3])), np.ascontiguousarray(i["surf_map"][:, 3]) if refl else None,
                               np.ascontiguousarray(i["surf_q"][:, :3]), np.ascontiguousarray(i["surf_q"][:, 3]) if refl else None, i["Q2"], i["T2"], PO)
    re_ = oracle.associate_edge(oracle.KdTree(np.ascontiguousarray(i["edge_map"][:, :3])), np.ascontiguousarray(i["edge_q"][:, :3]), i["Q2"], i["T2"], PO)
    v, ve = rs["valid"].astype(bool), re_["valid"].astype(bool)
    assert v.sum() > 1000 and ve.sum() > 100
    assert np.array_equal(np.c_[rs["cp"][v], rs["n"][v], rs["d"][v]], g[f"{flavour}_surf_rec"])
    assert np.array_equal(rs["score"][v], g[f"{flavour}_surf_score"])
    mine_e = np.c_[re_["cp"][ve], re_["a"][ve], re_["b"][ve], re_["s"][ve]]
    assert np.array_equal(_sorted_ab(mine_e), _sorted_ab(g[f"{flavour}_edge_rec"]))
    ss = (1000.0, int(v.sum())) if flavour == "rot" else 1.0
    se = (200.0, int(ve.sum())) if flavour == "rot" else 1.0
    raw = oracle.params(flavour, loss=0)
    rows_s = oracle.linearize_rows(rs, i["t0"], i["q0"], raw, ss, "surf")
    rows_e = oracle.linearize_rows(re_, i["t0"], i["q0"], raw, se, "edge")
    assert np.array_equal(np.c_[rows_s[:, 7], rows_s[:, :7]], g[f"{flavour}_surf_rows"])
    assert np.array_equal(np.c_[rows_e[:, 7], rows_e[:, :7]], g[f"{flavour}_edge_rows"])


# ------------------------------------------------------------------ local-map assembly
def test_oracle_local_map_equals_reference_backend(oracle):
    """transformCloud / buildLocalMapWithLandMark / downSampleCloud compiled from the reference text (7 keyframes through a ring of 3,
    tilted extrinsic) vs the numpy restatement: the down-sampled surf / edge maps and keyframe features of every keyframe, bit for bit —
    the first-keyframe special case (own raw features moved by T_bl), the rebuild-while-short branch, the pop/push branch, the
    q_po * q_bl composition and the f64 -> f32 rounding of the moved points."""
    g = np.load(os.path.join(G, "ref_localmap.npz"))
    i = M.localmap_inputs()
    os_ = oracle.LocalMapAssembly(M.LM_WIDTH, M.LM_SURF_MAP_LEAF, M.LM_SURF_LEAF, i["q_bl"], i["t_bl"])
    oe = oracle.LocalMapAssembly(M.LM_WIDTH, M.LM_EDGE_MAP_LEAF, M.LM_EDGE_LEAF, i["q_bl"], i["t_bl"])
    sizes = []
    for k, (s, e, p) in enumerate(zip(i["surf"], i["edge"], i["poses"])):
        ms, ds = os_.keyframe(s)
        me, de = oe.keyframe(e)
        for name, a in (("surf_map", ms), ("edge_map", me), ("surf_ds", ds), ("edge_ds", de)):
            b = g[f"kf{k}_{name}"]
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (k, name)
        sizes.append(os_.raw.shape[0])
        os_.commit(p)
        oe.commit(p)
    # before the filter: the first keyframe's own raw features, then the down-sampled features of the newest <= width earlier keyframes
    ds_n = [g[f"kf{k}_surf_ds"].shape[0] for k in range(len(sizes))]
    assert sizes == [900] + [sum(ds_n[max(0, k - M.LM_WIDTH):k]) for k in range(1, len(sizes))]
    assert len(os_.recent) == M.LM_WIDTH


# ------------------------------------------------------------------ wire format and marginalisation feed vs oracle / product
def test_oracle_equals_reference_format_convert(oracle):
    """livoxLidarHandler (FormatConvert.cpp compiled unmodified) vs the numpy restatement: every published row bit for bit,
    including the 0/0 and x/0 rows of an all-zero offset_time."""
    g = np.load(os.path.join(G, "ref_format.npz"))
    pts, zero = M.format_inputs()
    a = oracle.livox_custom_to_cloud(pts)
    assert a.shape[0] == int(g["n"]) and _sha(a) == str(g["sha"])
    assert np.array_equal(_bits(a[::16]), _bits(g["every16"]))
    assert np.array_equal(_bits(oracle.livox_custom_to_cloud(zero)), _bits(g["zero_case"]))


def _rec_dicts(srec, erec):
    rs = dict(valid=np.ones(len(srec), np.uint8), cp=srec[:, 0:3].astype(np.float32), n=srec[:, 3:6].astype(np.float32),
              d=srec[:, 6].astype(np.float32), score=srec[:, 7].copy())
    re_ = dict(valid=np.ones(len(erec), np.uint8), cp=erec[:, 0:3].astype(np.float32), a=erec[:, 3:6].astype(np.float32),
               b=erec[:, 6:9].astype(np.float32), s=erec[:, 9].astype(np.float32))
    return rs, re_


def test_oracle_and_product_equal_reference_marginalisation_feed(oracle):
    """ResidualBlockInfo::Evaluate (the loss corrector every lidar block goes through) and ThreadsConstructA (A += J_i^T J_j with
    rightCols(3) of the quaternion block, b += J_i^T r), compiled from the reference text, vs (1) the oracle's robustified rows
    and per-residual accumulation: bit for bit; (2) the product's lili_marg_add_lidar fed with the Gram of the same rows: 1e-12."""
    import lili_om_amd as L
    g = np.load(os.path.join(G, "ref_marg.npz"))
    i, srec, erec = M.marg_inputs()
    PO = oracle.params("livox")
    rs, re_ = _rec_dicts(srec, erec)
    rows = np.r_[oracle.linearize_rows(re_, i["t0"], i["q0"], PO, 1.0, "edge"), oracle.linearize_rows(rs, i["t0"], i["q0"], PO, 1.0, "surf")]
    mine = np.c_[rows[:, 7], rows[:, :7]]                       # r, J_t, J_q like the reference's ResidualBlockInfo
    assert mine.shape[0] == int(g["n_rows"]) and _sha(mine) == str(g["rows_sha"])
    assert np.array_equal(mine[::8], g["rows_every8"])
    A, b = oracle.marg_accumulate(rows[:, :7], rows[:, 7], M.MARG_POS, M.MARG_IDX_T, M.MARG_IDX_Q)
    assert np.array_equal(A, g["A"]) and np.array_equal(b, g["b"])
    # product: one Gram record -> A, b
    Jr = np.c_[rows[:, :7], rows[:, 7]]
    Gm = Jr.T @ Jr
    A2, b2 = np.zeros((M.MARG_POS, M.MARG_POS)), np.zeros(M.MARG_POS)
    L.api.marg_add_lidar(Gm, A2, b2, M.MARG_IDX_T, M.MARG_IDX_Q)
    assert np.abs(A2 - g["A"]).max() <= 1e-12 * np.abs(g["A"]).max()
    assert np.abs(b2 - g["b"]).max() <= 1e-12 * np.abs(g["b"]).max()


# ------------------------------------------------------------------ product host logic vs reference
def test_product_gyro_integration_feeds_reference_identically(oracle):
    """lili_imu_integrate (the product's host-side processIMU) -> q_imu -> deskewed cloud: bit-identical to what the
    reference node published, i.e. the q_imu it integrated internally has the same bits."""
    import lili_om_amd as L
    g = np.load(os.path.join(G, "ref_rot.npz"))
    scans, stamps, imu_t, gyr = M.rot_inputs()
    integ = L.api.ImuIntegrator()
    for k in range(2):
        q_imu = _q_imu_per_scan(integ, stamps, imu_t, gyr, k)
        r = oracle.extract_rot(scans[k], q_imu, M.ROT_QLB, oracle.rot_params(ds_rate=4, atan_mode=0, stable_sort=0))
        assert np.array_equal(_bits(r["full"]), _bits(g[f"cutted{k}"]))


# ------------------------------------------------------------------ live differential tests against oracle/_ref (build container only)
needs_ref = pytest.mark.skipif(not M.R.available(), reason="oracle/_ref not built (needs /root/reference; build container only)")


def _rot_params(line_num, ds_rate, qlb):
    p = dict(M.ROT_PARAMS)
    p.update({"/preprocessing/line_num": line_num, "/preprocessing/ds_rate": ds_rate, "/backend_fusion/ql2b_w": qlb[0],
              "/backend_fusion/ql2b_x": qlb[1], "/backend_fusion/ql2b_y": qlb[2], "/backend_fusion/ql2b_z": qlb[3]})
    return p


@needs_ref
@pytest.mark.parametrize("line_num,ds_rate", [(16, 1), (32, 2), (64, 1)])
def test_reference_rot_node_ring_tables_and_bad_points(oracle, line_num, ds_rate):
    """The reference's ROT Preprocessing node with the 16- / 32- / 64-ring tables, every ring kept (ds_rate 1) or every second,
    a unit and a non-unit extrinsic, and scans that contain NaN points, points closer than 3 m and points outside the ring
    table: every published cloud equals the oracle's literal mode bit for bit."""
    from lili_om_amd import synth
    rng = np.random.default_rng(100 + line_num)
    scans = []
    for s_ in range(3):
        w = synth.make_workload(n_map=50_000, n_az=150, half_extent=(120.0, 120.0), seed=synth.SEED_SCENE + 70 + s_)
        raw = np.concatenate([w["scan_xyz"], rng.integers(1, 255, (w["scan_xyz"].shape[0], 1)).astype(np.float32)], 1).astype(np.float32)
        bad = rng.choice(raw.shape[0], 90, replace=False)
        raw[bad[:30], rng.integers(0, 3, 30)] = np.nan                      # removeNaNFromPointCloud
        raw[bad[30:60], :3] *= 0.01                                          # closer than 3 m: removeClosedPointCloud
        raw[bad[60:], 2] = np.abs(raw[bad[60:], 2]) + 60.0                   # far above the ring table
        scans.append(raw)
    stamps = 20.0 + 0.1 * np.arange(3)
    imu_t = 19.96 + 0.005 * np.arange(70)
    gyr = 0.3 * rng.standard_normal((70, 3))
    qlb = [1.0, 0.0, 0.0, 0.0] if line_num == 32 else [0.7071, 0.0, 0.0, 0.7071]
    out = M.R.run_scans("rot", _rot_params(line_num, ds_rate, qlb), scans, stamps, imu_t, gyr)
    assert len(out) == 1
    q_imu = oracle.ImuIntegrator().integrate(imu_t[imu_t <= stamps[2]], gyr[imu_t <= stamps[2]], stamps[1])
    r = oracle.extract_rot(scans[0], q_imu, qlb, oracle.rot_params(n_scans=line_num, ds_rate=ds_rate, atan_mode=0, stable_sort=0))
    o = out[0]
    assert np.array_equal(_bits(r["full"]), _bits(o["cutted"][:, M.PAYLOAD_ROT]))
    assert np.array_equal(_bits(r["full"][r["edge_idx"]]), _bits(o["edge"][:, M.PAYLOAD_ROT]))
    assert np.array_equal(_bits(r["surf"]), _bits(o["surf"][:, M.PAYLOAD_ROT]))
    assert r["full"].shape[0] > 3000 and len(r["edge_idx"]) > 20 and r["surf"].shape[0] > 100


@needs_ref
def test_reference_livox_node_bad_points(oracle):
    """The Livox node on scans with NaNs, near points (< 0.1 m), far points (> 200 m), zero / saturated reflectivity and
    duplicate time slots (synth.make_livox_scan(inject_bad=True) plus extra NaNs)."""
    from lili_om_amd import synth
    rng = np.random.default_rng(7)
    scans = [synth.make_livox_scan(60 + s_, inject_bad=True) for s_ in range(3)]
    for sc in scans:
        bad = rng.choice(sc.shape[0], 40, replace=False)
        sc[bad[:20], rng.integers(0, 3, 20)] = np.nan
        sc[bad[20:], :3] *= 0.001
    stamps = 30.0 + 0.1 * np.arange(3)
    imu_t = 29.96 + 0.005 * np.arange(70)
    gyr = 0.3 * rng.standard_normal((70, 3))
    out = M.R.run_scans("livox", M.LIVOX_PARAMS, scans, stamps, imu_t, gyr)
    assert len(out) == 1
    q_imu = oracle.ImuIntegrator().integrate(imu_t[imu_t <= stamps[2]], gyr[imu_t <= stamps[2]], stamps[1])
    r = oracle.extract_livox(scans[0], q_imu)
    pay = [0, 1, 2, 6, 7]
    for name in ("cutted", "edge", "surf"):
        a, b = r[name], out[0][name][:, M.PAYLOAD_LIVOX]
        assert a.shape == b.shape, name
        assert np.array_equal(_bits(a[:, pay]), _bits(b[:, pay])), name
        assert np.array_equal(_bits(np.abs(a[:, 3:6])), _bits(np.abs(b[:, 3:6]))), name


@needs_ref
@pytest.mark.parametrize("flavour", ["livox", "rot"])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_reference_backend_association_random_scenes(oracle, flavour, seed):
    """Randomised differential test of the back-end association against the reference's functions: different rooms, noise levels,
    pose errors (so that gates, plane-validity and weight thresholds are all exercised on both sides of their limits)."""
    from lili_om_amd import synth
    from tests import frontend_chain as F
    rng = np.random.default_rng(1000 + seed)
    room = synth.make_room(seed=200 + seed, size=(10.0 + 6 * seed, 8.0 + 3 * seed, 4.0 + seed), leaf=0.3 + 0.1 * (seed % 3),
                           n_query=900, n_edge_query=150, noise=0.005 * seed * seed)
    B = M.BACKEND_PARAMS[flavour]
    PO = oracle.params(flavour)
    qlb, tlb = np.array(B["q_lb"]), np.array(B["t_lb"])
    qb, tb = F.eigen_qmul(room["q_true"], qlb), room["t_true"] + F.eigen_qrot(room["q_true"], tlb[None, :])[0]
    t0, q0 = synth.perturbed_pose(tb, qb, rng, 0.02 * seed * seed, 0.3 * seed)
    Q2 = F.eigen_qmul(q0, F.eigen_qinv(qlb))
    T2 = t0 - F.eigen_qrot(Q2, tlb[None, :])[0]
    z = lambda a: np.zeros((a.shape[0], 1), np.float32)                                 # noqa: E731
    smap, sq = np.c_[room["map_xyz"], room["map_refl"]].astype(np.float32), np.c_[room["q_xyz"], room["q_refl"]].astype(np.float32)
    emap, eq = np.c_[room["edge_map_xyz"], z(room["edge_map_xyz"])].astype(np.float32), np.c_[room["eq_xyz"], z(room["eq_xyz"])].astype(np.float32)
    srec, erec = M.R.backend_associate(flavour, smap, emap, sq, eq, Q2, T2, B["kd_max_radius"], B["surf_dist_thres"], B["lidar_const"], B["reflect_thres"])
    refl = flavour == "livox"
    rs = oracle.associate_surf(oracle.KdTree(room["map_xyz"]), room["map_refl"] if refl else None, room["q_xyz"], room["q_refl"] if refl else None, Q2, T2, PO)
    re_ = oracle.associate_edge(oracle.KdTree(room["edge_map_xyz"]), room["eq_xyz"], Q2, T2, PO)
    v, ve = rs["valid"].astype(bool), re_["valid"].astype(bool)
    mine_s = np.c_[rs["cp"][v], rs["n"][v], rs["d"][v], rs["score"][v]].astype(np.float64)
    assert mine_s.shape == srec.shape and np.array_equal(mine_s, srec)
    mine_e = np.c_[re_["cp"][ve], re_["a"][ve], re_["b"][ve], re_["s"][ve]].astype(np.float64)
    assert mine_e.shape == erec.shape and np.array_equal(_sorted_ab(mine_e), _sorted_ab(erec))
    assert 0 < v.sum() < v.size                                          # some queries accepted, some rejected
    srows, erows = M.R.backend_rows(flavour, srec, erec, qlb, tlb, t0, q0)
    raw = oracle.params(flavour, loss=0)
    ss = (1000.0, int(v.sum())) if flavour == "rot" else 1.0
    se = (200.0, max(int(ve.sum()), 1)) if flavour == "rot" else 1.0
    rows_s = oracle.linearize_rows(rs, t0, q0, raw, ss, "surf")
    assert np.array_equal(np.c_[rows_s[:, 7], rows_s[:, :7]], srows)
    if ve.sum():
        rows_e = oracle.linearize_rows(re_, t0, q0, raw, se, "edge")
        # the reference builds the edge factor from ITS (A, B) order; the residual is symmetric in A <-> B, bit for bit
        assert np.array_equal(np.c_[rows_e[:, 7], rows_e[:, :7]], erows)


@needs_ref
@pytest.mark.parametrize("seed,match_cnt", [(300, 3), (400, 5)])
def test_reference_frontend_node_other_sequences(oracle, seed, match_cnt):
    """The front-end loop on oracle primitives against the reference's LidarOdometry node, live, on other sequences and
    scan_match_cnt settings than the committed fixture: poses, residual-block counts and every solve's step bit for bit."""
    from tests import frontend_chain as F
    from tests import seq_harness as H
    n = 5
    frames = H.make_frames(n + 2, seed=seed)
    stamps = 40.0 + 0.1 * np.arange(n + 2)
    imu_t = 39.97 + 0.005 * np.arange(20 * (n + 2) + 20)
    gyr = np.zeros((imu_t.shape[0], 3))
    pre = M.R.run_scans("livox", M.LIVOX_PARAMS, frames, stamps, imu_t, gyr)
    params = dict(M.FRONTEND_PARAMS)
    params["/lidar_odometry/scan_match_cnt"] = match_cnt
    lo = M.R.LidarOdometry(params)
    ref_abs = np.array([lo.frame(o["stamp"], o["edge"], o["surf"], o["cutted"])[0] for o in pre])
    S = lo.solves()
    lo.close()
    surf = [o["surf"][:, [0, 1, 2, 9]] for o in pre]                      # x y z curvature of the 48-byte rows the Livox node published
    be = F.OracleBackend(oracle, stable=False)
    a, _ = F.run_frontend_chain(be, surf, scan_match_cnt=match_cnt)
    assert np.array_equal(a, ref_abs)
    assert len(be.log) == len(S) and [l["n_blocks"] for l in be.log] == [len(s["records"]) for s in S]
    assert all(np.array_equal(l["pose_out"], s["pose_out"]) for l, s in zip(be.log, S))


@needs_ref
@pytest.mark.parametrize("width,seed", [(1, 5), (2, 6), (5, 7)])
def test_reference_local_map_other_widths(oracle, width, seed):
    """Live differential run of the local-map slice at other ring widths (1 = always the previous keyframe only), random poses,
    keyframes of different sizes including an empty edge cloud."""
    rng = np.random.default_rng(seed)
    q_bl = rng.normal(size=4); q_bl /= np.linalg.norm(q_bl)
    t_bl = rng.uniform(-0.2, 0.2, 3)
    lm = M.R.LocalMapSlice(width, 0.4, 0.2, 0.4, 0.2, q_bl, t_bl)
    os_ = oracle.LocalMapAssembly(width, 0.4, 0.4, q_bl, t_bl)
    oe = oracle.LocalMapAssembly(width, 0.2, 0.2, q_bl, t_bl)
    for k in range(width + 4):
        ns, ne = int(rng.integers(200, 1500)), (0 if k == 2 else int(rng.integers(20, 200)))
        s = np.concatenate([rng.uniform(-4, 4, (ns, 3)), rng.uniform(0, 25, (ns, 1))], 1).astype(np.float32)
        e = np.concatenate([rng.uniform(-4, 4, (ne, 3)), rng.uniform(0, 25, (ne, 1))], 1).astype(np.float32)
        r = lm.keyframe(s, e)
        ms, ds = os_.keyframe(s)
        me, de = oe.keyframe(e)
        for a, b in ((r["surf_map"], ms), (r["edge_map"], me), (r["surf_ds"], ds), (r["edge_ds"], de)):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        pose = np.concatenate([q, rng.uniform(-2, 2, 3)])
        lm.commit(pose); os_.commit(pose); oe.commit(pose)
    lm.close()


def test_functor_row_fixture_is_the_reference_functors_output():
    """tests/golden/ref_functor_rows.npz (the rows tests/test_reference_gpu.py::test_gpu_linearize_vs_reference_functors falls back on where the
    git-ignored oracle/_ref did not travel): re-evaluated here through LidarPlaneNormFactor / LidarEdgeFactor of the reference's header
    (oracle/_ref/libref_factors.so) on the records stored beside them — the committed rows are the reference's, bit for bit."""
    from oracle import ref as R
    if not R.available():
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    import lili_om_amd as L
    from lili_om_amd import synth
    d = np.load(os.path.join(G, "ref_functor_rows.npz"))
    for variant in ("livox", "rot"):
        P = L.make_params(variant)
        room = synth.make_room(seed=12, n_query=1500, n_edge_query=200)
        tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
        t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(3), 0.05, 0.5)
        rs = {k: d[f"{variant}_s_{k}"] for k in ("cp", "n", "d", "score")}
        re_ = {k: d[f"{variant}_e_{k}"] for k in ("cp", "a", "b", "s")}
        ns, ne = len(rs["d"]), len(re_["s"])
        ss = P.scale_surf_num / ns if P.scale_surf_num else 1.0
        se = P.scale_edge_num / ne if P.scale_edge_num else 1.0
        rows_s, rows_e = M.functor_rows(R, rs, re_, np.array(list(P.q_lb)), np.array(list(P.t_lb)), ss, se, np.asarray(t0, np.float64), np.asarray(q0, np.float64))
        assert np.array_equal(rows_s, d[f"{variant}_rows_s"]) and np.array_equal(rows_e, d[f"{variant}_rows_e"])
