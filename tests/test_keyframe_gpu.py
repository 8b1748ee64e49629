"""The keyframe hand-over on the device: lili_keyframe_undistort against what the reference's own odometry nodes published with if_to_deskew = 1
(tests/golden/ref_keyframe.npz) and against the numpy model (tests/keyframe_model.py); lili_frontend_keyframe behind the frame calls against the kernel on the features the
extraction calls return; the seam run on the reference's sequences; the hand-over into lili_backend_keyframe_prepare / lili_archive_push; replay(keyframes=True)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from tests import keyframe_model as M

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLD, "make_ref_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

A = L.api
E_ARG, E_STATE = -1, -3


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ref_keyframe.npz"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


def host_cloud(rows, aux_col):
    c = A.cloud_from_numpy(rows, aux_col=aux_col)
    return c


def undistort_host(ctx, clouds, offs, t, q=None, out_ptrs=None):
    """lili_keyframe_undistort, the three results on the host as (n, 4) arrays"""
    import torch
    res = A.keyframe_undistort(ctx, clouds, offs, t, q, out_ptrs)
    ctx.sync()
    out = []
    for c in res:
        if c._keep is not None:
            out.append(c._keep[:int(c.n)].cpu().numpy())
        else:
            out.append(None)
    torch.cuda.synchronize()
    return out


def fixture_rows(gold, flavour, fr):
    """per cloud: (n, 4) input rows x y z intensity, aux column, published xyz"""
    out = []
    for name in M.CLOUDS:
        k = f"{flavour}/{fr}/{name}"
        out.append((gold[f"{k}/in"], gold[f"{k}/wrong"], gold[f"{k}/out"]))
    return out


@pytest.mark.parametrize("flavour", ["livox", "rot"])
def test_kernel_equals_the_reference_node(gpu_ctx, gold, flavour):
    """host rows in the node's own point layout (48 / 32 bytes) and device float4 rows; the three clouds of a keyframe in one call; frames 1 and 4"""
    import torch
    floats, tcol = M.ROW_FLOATS[flavour], M.TIME_COL[flavour]
    auxcol = 9 if flavour == "livox" else 4
    for fr in (1, 4):
        t_rel = gold[f"{flavour}/rel_pose"][fr, 4:]
        sets = fixture_rows(gold, flavour, fr)
        hosts = []
        for rows, aux, _ in sets:
            h = np.full((rows.shape[0], floats), 7.5, np.float32)
            h[:, :3] = rows[:, :3]; h[:, tcol] = rows[:, 3]
            if flavour == "livox":
                h[:, auxcol] = aux
            hosts.append(h)
        got = undistort_host(gpu_ctx, [host_cloud(h, auxcol) for h in hosts], [4 * tcol] * 3, t_rel)
        for (rows, aux, want), h, g in zip(sets, hosts, got):
            assert same_bits(g[:, :3], want), (flavour, fr)
            assert same_bits(g[:, 3], h[:, auxcol])
        # page-locked host rows (read where they lie) and an explicit identity quaternion
        pins = [A.PinnedArray(h.shape, np.float32) for h in hosts]
        for p, h in zip(pins, hosts):
            p.array[...] = h
        clouds = [A.Cloud(p.ptr, h.shape[0], 4 * floats, 4 * auxcol, A.MEM_HOST) for p, h in zip(pins, hosts)]
        got = undistort_host(gpu_ctx, clouds, [4 * tcol] * 3, t_rel, [1.0, 0, 0, 0])
        for (rows, aux, want), g in zip(sets, got):
            assert same_bits(g[:, :3], want), (flavour, fr, "pinned")
        # device rows of stride 16: x y z intensity, the intensity also the aux
        dev = [torch.from_numpy(np.ascontiguousarray(rows)).cuda() for rows, _, _ in sets]
        clouds = [A.cloud_from_device(d.data_ptr(), d.shape[0], 16, 12) for d in dev]
        got = undistort_host(gpu_ctx, clouds, [12] * 3, t_rel)
        for (rows, aux, want), g in zip(sets, got):
            assert same_bits(g[:, :3], want) and same_bits(g[:, 3], rows[:, 3]), (flavour, fr, "device")


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]


def designed_rows(rng, n):
    """x y z and a designed time channel: exactly k, k + 0.1f, just above, negative, k + 0.05f, and ordinary ones"""
    rows = rng.uniform(-80, 80, (n, 4)).astype(np.float32)
    k = rng.integers(0, 6, n).astype(np.float32)
    kind = np.arange(n) % 7
    f01 = np.float32(0.1)
    t = np.where(kind == 0, k, 0).astype(np.float32)
    t = np.where(kind == 1, k + f01, t).astype(np.float32)
    t = np.where(kind == 2, np.nextafter((k + f01).astype(np.float32), np.float32(100)), t).astype(np.float32)
    t = np.where(kind == 3, -rng.uniform(0.01, 3.0, n).astype(np.float32), t).astype(np.float32)
    t = np.where(kind == 4, k + np.float32(0.05), t).astype(np.float32)
    t = np.where(kind == 5, k + rng.uniform(0, 0.1, n).astype(np.float32), t).astype(np.float32)
    t = np.where(kind == 6, k + rng.uniform(0.1, 0.9, n).astype(np.float32), t).astype(np.float32)      # beyond the sweep: clamped
    rows[:, 3] = t
    return rows


def test_tile_edges_and_segment_lookup(gpu_ctx):
    import torch
    rng = np.random.default_rng(11)
    combos = []
    for a in SIZES:
        combos += [(a, 0, 0), (0, a, 0), (0, 0, a)]
    combos += [(1, 63, 64), (63, 64, 65), (65, 255, 256), (255, 256, 257), (257, 1000, 1), (1000, 65, 0), (64, 0, 257), (256, 1, 1000)]
    t_rel = np.array([0.4371, -0.0213, 0.0077])
    n_checked = 0
    for combo in combos:
        rows = [designed_rows(rng, n) for n in combo]
        want = [np.c_[M.undistort(r[:, :3], r[:, 3], t_rel), r[:, 3]].astype(np.float32) for r in rows]
        dev = [torch.from_numpy(r).cuda() for r in rows]
        clouds = [A.cloud_from_device(d.data_ptr(), d.shape[0], 16, 12) if d.shape[0] else None for d in dev]
        got = undistort_host(gpu_ctx, clouds, [12] * 3, t_rel)
        for g, w in zip(got, want):
            assert same_bits(g, w), combo
            n_checked += g.shape[0]
        # in place equals out of place
        A.keyframe_undistort(gpu_ctx, clouds, [12] * 3, t_rel, None, [d.data_ptr() if d.shape[0] else None for d in dev])
        gpu_ctx.sync()
        for d, w in zip(dev, want):
            if d.shape[0]:
                assert same_bits(d.cpu().numpy(), w), (combo, "in place")
    assert n_checked > 10000


def _axis_angle(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.r_[np.cos(angle / 2), np.sin(angle / 2) * axis]


def test_general_rotation(gpu_ctx):
    """A caller's q_rel (pinned to the model only).  Bound, derived: both sides evaluate the same f64 expression with relative errors of a few 1e-16 (the sines differ
    by an ulp of f64 between libraries), far below half an f32 ulp, so the two f32 roundings can differ only when the exact value lies next to a rounding boundary — by
    one f32 ulp at the magnitude of the result, which is at most |p|_inf * sqrt(3) + |t_rel|_inf; the issue's bound, one ulp at |p|_inf + |t_rel|_inf, is what is asserted."""
    import torch
    rng = np.random.default_rng(12)
    rows = designed_rows(rng, 1000)
    t_rel = np.array([0.51, -0.07, 0.02])
    q = _axis_angle([0.3, -0.5, 0.8], 0.3)
    cases = {"skew_0.3rad": q, "all_signs_flipped": -q, "linear_branch": np.array([1.0, 1e-18, -2e-18, 0.5e-18])}
    dev = torch.from_numpy(rows).cuda()
    cloud = A.cloud_from_device(dev.data_ptr(), rows.shape[0], 16, 12)
    for name, qq in cases.items():
        got = undistort_host(gpu_ctx, [cloud, None, None], [12] * 3, t_rel, qq)[0]
        want = M.undistort(rows[:, :3], rows[:, 3], t_rel, qq)
        mag = np.abs(rows[:, :3]).max(1) + np.abs(t_rel).max()
        ulp = np.spacing(mag.astype(np.float32)).astype(np.float64)
        d = np.abs(got[:, :3].astype(np.float64) - want.astype(np.float64))
        share = float((bits(got[:, :3]) != bits(want)).mean())
        print(f"general q_rel {name}: max |d| / ulp = {(d / ulp[:, None]).max():.3g}, coordinates not bit-identical: {100 * share:.3f} %")
        assert (d <= ulp[:, None]).all(), name
        assert same_bits(got[:, 3], rows[:, 3])
    # the flipped quaternion is the same rotation; the linear branch at 1e-18 moves nothing but the translation
    ident = undistort_host(gpu_ctx, [cloud, None, None], [12] * 3, t_rel)[0]
    lin = undistort_host(gpu_ctx, [cloud, None, None], [12] * 3, t_rel, cases["linear_branch"])[0]
    assert np.abs(lin[:, :3] - ident[:, :3]).max() <= np.spacing(np.float32(160.0))


def test_non_finite_rows_and_bad_arguments(gpu_ctx):
    import torch
    rng = np.random.default_rng(13)
    rows = designed_rows(rng, 300)
    t_rel = np.array([0.3, 0.1, -0.2])
    clean = M.undistort(rows[:, :3], rows[:, 3], t_rel)
    bad = rows.copy()
    bad[10, 0] = np.nan; bad[70, 2] = np.inf; bad[130, 3] = np.nan; bad[200, :3] = np.nan; bad[255, 3] = np.inf; bad[256, 3] = -np.inf
    dev = torch.from_numpy(bad).cuda()
    got = undistort_host(gpu_ctx, [None, A.cloud_from_device(dev.data_ptr(), 300, 16, 12), None], [0, 12, 0], t_rel)[1]
    for r in (10, 70, 130, 200, 256):      # (-inf: the slerp's weights are inf and -inf)
        assert np.isnan(got[r, :3]).all(), r
    assert same_bits(got[255, :3], (bad[255, :3].astype(np.float64) + t_rel).astype(np.float32))          # +inf: ratio clamps to 1
    keep = np.ones(300, bool); keep[[10, 70, 130, 200, 255, 256]] = False
    assert same_bits(got[keep, :3], clean[keep])                                                           # no neighbour disturbed
    model = M.undistort(bad[:, :3], bad[:, 3], t_rel)                                                      # the same NaN pattern as Eigen's arithmetic gives, the same bits elsewhere
    assert np.array_equal(np.isnan(got[:, :3]), np.isnan(model)) and same_bits(np.nan_to_num(got[:, :3], nan=0.0), np.nan_to_num(model, nan=0.0))
    # bad strides and offsets: LILI_E_ARG, the output untouched
    out = torch.full((300, 4), -5.0, dtype=torch.float32, device="cuda")
    good = dict(stride=16, aux=12, toff=12)
    for change in (dict(stride=18), dict(stride=8), dict(aux=14), dict(aux=16), dict(toff=13), dict(toff=16), dict(toff=-1)):
        a = dict(good, **change)
        cloud = A.Cloud(dev.data_ptr(), 300, a["stride"], a["aux"], A.MEM_DEVICE)
        with pytest.raises(L.LiliError, match=f"lili error {E_ARG}"):
            A.keyframe_undistort(gpu_ctx, [cloud, None, None], [a["toff"], 0, 0], t_rel, None, [out.data_ptr(), None, None])
    gpu_ctx.sync()
    assert bool((out == -5.0).all())
    # the frame-bound call before any extraction
    ctx = L.Context(0)
    try:
        for flavour in (A.VARIANT_LIVOX, A.VARIANT_ROT):
            with pytest.raises(L.LiliError, match=f"lili error {E_STATE}"):
                A.frontend_keyframe(ctx, flavour, t_rel, None, True)
        with pytest.raises(L.LiliError, match=f"lili error {E_STATE}"):
            A.frontend_keyframe_get(ctx, 0)
        with pytest.raises(L.LiliError, match=f"lili error {E_ARG}"):
            A.frontend_keyframe(ctx, A.VARIANT_FRONTEND, t_rel, None, True)
    finally:
        ctx.close()


# ---- the seam behind the frame calls -------------------------------------------------------------------------------------------------------------------------------

def _q_imu(integ, stamps, imu_t, gyr, k):
    m = imu_t <= stamps[k + 2]
    return integ.integrate(imu_t[m], gyr[m], stamps[k + 1])


def run_sequence(flavour, hook=None, deskew=True):
    """The reference's six-frame sequence through the frame call, the rule, computeRelative and lili_frontend_keyframe; hook(ctx, odo, rec, device clouds) at keyframes."""
    from tests import frontend_chain as F
    if flavour == "livox":
        scans, stamps, imu_t, gyr = G.frontend_inputs()
        n = G.FRONTEND_FRAMES
    else:
        scans, stamps, imu_t, gyr = G.frontend_rot_inputs()
        n = G.FRONTEND_R_FRAMES
    ctx = L.Context(0)
    try:
        integ = A.ImuIntegrator()
        if flavour == "livox":
            odo = L.FrontendOdometry(ctx, scan_match_cnt=6, first_match_cnt=8, reference_startup=True)
        else:
            odo = L.RotFrontendOdometry(ctx, n_scans=64, ds_rate=4, q_lb=G.ROT_QLB, scan_match_cnt=6, first_match_cnt=8, reference_startup=True)
        odo.reset()
        rule = L.KeyframeRule()
        t_abs, q_abs = np.zeros(3), np.array([1.0, 0, 0, 0])
        t_rel, q_rel = np.zeros(3), np.array([1.0, 0, 0, 0])
        recs = []
        for k in range(n):
            q_imu = _q_imu(integ, stamps, imu_t, gyr, k)
            scan = np.ascontiguousarray(scans[k], np.float32)
            if k == 0:
                _, _, info = odo.frame(scan, t_abs, q_abs, q_imu)
            else:
                t0 = F.eigen_qrot(q_abs, t_rel[None, :])[0] + t_abs      # poseInitialization
                q0 = F.eigen_qmul(q_abs, q_rel)
                t, q, info = odo.frame(scan, t0, q0, q_imu)
                t_rel, q_rel = L.pose_relative(t_abs, q_abs, t, q)
                t_abs, q_abs = t, q
            verdict = rule.step(t_abs, q_abs, info["matched"])
            rec = dict(k=k, t=t_abs.copy(), q=q_abs.copy(), t_rel=t_rel.copy(), q_rel=q_rel.copy(), verdict=verdict, info=info, scan=scan, q_imu=np.array(q_imu), stamp=stamps[k])
            if verdict != M.KF_NO:
                views = odo.keyframe(t_rel, None, deskew and verdict == M.KF_YES)
                rec["clouds"] = [A.frontend_keyframe_get(ctx, kind) for kind in range(3)]
                assert [int(v.n) for v in views] == [c.shape[0] for c in rec["clouds"]]
                if hook:
                    hook(ctx, odo, rec, views)
            recs.append(rec)
        return recs
    finally:
        ctx.close()


def features_by_extraction(ctx2, flavour, scan, q_imu):
    """the frame's three lists as the existing extraction calls return them on the host, with where their time channel and their published aux lie:
    -> [(rows, time column, aux column)] for edge, surf, full"""
    if flavour == "livox":
        f = A.LivoxExtractor(ctx2).extract(scan, q_imu)
        return [(np.ascontiguousarray(f["edge"]), 6, 7), (np.ascontiguousarray(f["surf"]), 6, 7), (np.ascontiguousarray(f["cutted"]), 6, 6)]
    f = A.RotExtractor(ctx2, n_scans=64, ds_rate=4).extract(scan, q_imu, G.ROT_QLB)
    return [(np.ascontiguousarray(f[k]), 3, 3) for k in ("edge", "surf", "full")]


def undistort_features(ctx2, feats, t_rel):
    clouds = [A.cloud_from_numpy(r, aux_col=a) if r.shape[0] else None for r, _, a in feats]
    return undistort_host(ctx2, clouds, [4 * tc for _, tc, _ in feats], t_rel)


def test_frontend_keyframe_after_a_livox_frame():
    ctx2 = L.Context(0)
    seen = []

    def hook(ctx, odo, rec, views):
        if rec["k"] != 4:
            return
        feats = features_by_extraction(ctx2, "livox", rec["scan"], rec["q_imu"])
        want = undistort_features(ctx2, feats, rec["t_rel"])
        assert (feats[0][0].shape[0], feats[1][0].shape[0]) == (rec["info"]["n_edge"], rec["info"]["n_surf"])
        assert rec["info"]["n_edge"] > 20 and rec["info"]["n_surf"] > 3000 and feats[2][0].shape[0] > 20000
        for kind in range(3):
            assert same_bits(rec["clouds"][kind], want[kind]), kind
        # deskew = 0: the extractor's clouds in the same layout
        odo.keyframe(None, None, False)
        for kind in range(3):
            rows, _, a = feats[kind]
            assert same_bits(A.frontend_keyframe_get(ctx, kind), rows[:, [0, 1, 2, a]]), kind
        # and a caller's rotation goes through the same kernel
        q = _axis_angle([0.1, 0.2, -0.4], 0.05)
        odo.keyframe(rec["t_rel"], q, True)
        clouds = [A.cloud_from_numpy(r, aux_col=a) if r.shape[0] else None for r, _, a in feats]
        want_q = undistort_host(ctx2, clouds, [4 * tc for _, tc, _ in feats], rec["t_rel"], q)
        for kind in range(3):
            assert same_bits(A.frontend_keyframe_get(ctx, kind), want_q[kind]), kind
        seen.append(rec["k"])

    try:
        run_sequence("livox", hook)
    finally:
        ctx2.close()
    assert seen == [4]


def test_frontend_keyframe_after_a_rot_frame_with_guessed_counts():
    """lili_frontend_frame_rot on the caller's maps with frame_guess_counts on: the second frame of the same scan is matched with guessed counts; the keyframe clouds have
    the true ones."""
    import torch
    w = synth.make_workload(n_map=200_000, n_az=400, half_extent=(150.0, 150.0), verbose=False)
    raw = np.concatenate([w["scan_xyz"], np.full((w["scan_xyz"].shape[0], 1), 50.0, np.float32)], 1).astype(np.float32)
    P = L.make_params("rot")
    q_lb = np.array(list(P.q_lb))
    tb, qb = A.body_pose_from_lidar(w["lidar_t"], w["lidar_q"], P)
    d_raw = torch.from_numpy(raw).cuda()
    cloud = A.cloud_from_device(d_raw.data_ptr(), raw.shape[0], 16, 12)
    t_rel = np.array([0.45, 0.02, -0.01])
    ctx, ctx2 = L.Context(0), L.Context(0)
    try:
        ctx.set_option("frame_guess_counts", 1)
        m = L.ScanToMapMatcher(ctx, P)
        m.set_input_cloud(L.KIND_SURF, w["map_xyz"]); m.set_input_cloud(L.KIND_EDGE, w["edge_map_xyz"])
        odo = L.RotFrontendOdometry(ctx, params=P, n_scans=64, ds_rate=4, q_lb=q_lb, leaf_query=0.0, scan_match_cnt=2, external_map=True, edges=True, slot=1)
        for _ in range(2):
            _, _, info = odo.frame(cloud, tb, qb)
        assert info["matched"] and info["n_surf"] > 500 and info["n_edge"] > 50
        views = odo.keyframe(t_rel, None, True)
        got = [A.frontend_keyframe_get(ctx, kind) for kind in range(3)]
        assert (int(views[0].n), int(views[1].n)) == (info["n_edge"], info["n_surf"])
        f = A.RotExtractor(ctx2, n_scans=64, ds_rate=4).extract(raw, (1.0, 0, 0, 0), q_lb)
        feats = [(np.ascontiguousarray(f[k]), 3, 3) for k in ("edge", "surf", "full")]
        want = undistort_features(ctx2, feats, t_rel)
        for kind in range(3):
            assert same_bits(got[kind], want[kind]), kind
        odo.keyframe(None, None, False)
        for kind in range(3):
            assert same_bits(A.frontend_keyframe_get(ctx, kind), feats[kind][0]), kind
        # ... and behind a plain extraction call
        views2 = A.frontend_keyframe(ctx2, A.VARIANT_ROT, t_rel, None, True)
        assert [int(v.n) for v in views2] == [x.shape[0] for x in want]
        for kind in range(3):
            assert same_bits(A.frontend_keyframe_get(ctx2, kind), want[kind]), kind
    finally:
        ctx.close(); ctx2.close()


@pytest.mark.parametrize("flavour", ["livox", "rot"])
def test_seam_follows_the_reference_node(gold, flavour):
    recs = run_sequence(flavour)
    kf = list(gold[f"{flavour}/kf"])
    assert [int(r["verdict"] != M.KF_NO) for r in recs] == kf and recs[0]["verdict"] == M.KF_FIRST
    for r in recs:
        if r["verdict"] == M.KF_NO:
            continue
        fr = r["k"]
        dt = float(np.abs(r["t_rel"] - gold[f"{flavour}/rel_pose"][fr, 4:]).max()) if fr > 0 else 0.0
        for kind, name in enumerate(M.CLOUDS):
            k = f"{flavour}/{fr}/{name}"
            got = r["clouds"][kind]
            assert got.shape[0] == int(gold[f"{k}/n"]), (k, got.shape[0])
            if flavour == "rot" and name == "surf":
                continue            # count only: the ROT surf centroids are themselves allowed 4 ulp against the reference
            idx, want = gold[f"{k}/idx"], gold[f"{k}/out"]
            d = np.abs(got[idx, :3].astype(np.float64) - want.astype(np.float64))
            bound = dt + np.spacing(np.abs(want)).astype(np.float64)
            print(f"{k}: max |d| = {d.max():.3g}, |d t_rel| = {dt:.3g}, rows beyond the bound: {int((d > bound).any(1).sum())}")
            assert (d <= bound).all(), (k, float(d.max()), dt)


def test_hand_over_to_the_back_end_and_the_archive():
    """the keyframe's device clouds into lili_backend_keyframe_prepare and lili_archive_push against the same clouds through host copies"""
    P = L.make_params("rot")
    P.q_lb = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)      # the odometry poses are the LiDAR's: no extrinsic between them and the keyframes' map poses
    P.t_lb = (C.c_double * 3)(0.0, 0.0, 0.0)
    ca, cb = L.Context(0), L.Context(0)
    state = dict(n=0, prev=None, assoc=0)
    try:
        ma, mb = L.ScanToMapMatcher(ca, P), L.ScanToMapMatcher(cb, P)
        ba, bb = L.BackendKeyframes(ca, P, width=3), L.BackendKeyframes(cb, P, width=3)
        t_bl, q_bl = np.array(list(P.t_lb)), np.array(list(P.q_lb))
        ara, arb = L.KeyframeArchive(ca, q_bl, t_bl), L.KeyframeArchive(cb, q_bl, t_bl)

        def hook(ctx, odo, rec, views):
            ctx.sync()
            j = state["n"]
            win = list(range(max(0, j - 1), j + 1))
            slots = [w % 2 for w in win]
            poses = ([state["prev"]] if j > 0 else []) + [(rec["t"], rec["q"])]
            tq = [A.assoc_transform(t, q, P) for t, q in poses]
            ts, qs = [a[1] for a in tq], [a[0] for a in tq]
            join = None
            if j > 0:
                tj, qj = A.keyframe_map_pose(state["prev"][0], state["prev"][1], t_bl, q_bl)
                join = ((j - 1) % 2, tj, qj)
            edge, surf, full = views
            he, hs, hf = rec["clouds"]
            counts_a, info_a = ba.prepare(join, surf, edge, slots, ts, qs)
            counts_b, info_b = bb.prepare(join, hs, he, slots, ts, qs)
            assert info_a["n_query"] == info_b["n_query"] and info_a["n_query"][0] > 100 and info_a["n_map"] == info_b["n_map"]
            assert counts_a == counts_b and info_a["associated"] == info_b["associated"] == (j > 0)
            if j > 0:
                state["assoc"] += sum(a + b for a, b in counts_a)
                for s in slots:
                    ra, rb = ma.surf_records(s, 8192), mb.surf_records(s, 8192)
                    for key in ("query_index", "cp", "n", "d", "score"):
                        assert np.array_equal(ra[key], rb[key]), (j, s, key)
                    ea, eb = ma.edge_records(s, 8192), mb.edge_records(s, 8192)
                    for key in ("query_index", "cp", "a", "b", "s"):
                        assert np.array_equal(ea[key], eb[key]), (j, s, key)
            ka = ara.push(edge, surf, full, rec["stamp"], rec["t"], rec["q"])
            kb = arb.push(he, hs, hf, rec["stamp"], rec["t"], rec["q"])
            assert ka == kb == j
            for kind, host in ((L.ARCHIVE_EDGE, he), (L.ARCHIVE_SURF, hs), (L.ARCHIVE_FULL, hf)):
                assert same_bits(ara.get(ka, kind), host) and same_bits(arb.get(kb, kind), host), (j, kind)
            state["prev"] = (rec["t"], rec["q"])
            state["n"] += 1

        run_sequence("rot", hook)
        assert state["n"] == 3 and state["assoc"] > 200
    finally:
        ca.close(); cb.close()


def test_replay_with_keyframes(gpu_ctx, tmp_path):
    from lili_om_amd import replay, rosbag
    from tests import seq_harness as H
    from tests.test_replay_gpu import _custom
    n = 7
    frames = H.make_frames(n + 2)
    msgs = []
    for k, scan in enumerate(frames):
        t = 50.0 + 0.1 * k
        for j in range(20):
            ti = t + 0.005 * j
            msgs.append(("/livox/imu", "sensor_msgs/Imu", ti, rosbag.encode_imu(ti, (0.0, 0.0, 0.0), seq=20 * k + j)))
        msgs.append(("/livox/lidar", "livox_ros_driver/CustomMsg", t + 0.1, rosbag.encode_livox_custom(_custom(scan), t, seq=k)))
    path = str(tmp_path / "synthetic.bag")
    rosbag.write_bag(path, msgs, compression="bz2", chunk_messages=16)
    t0, q0, _ = H.gt_pose(0)
    plain = replay.replay(path, gpu_ctx, "/livox/lidar", "/livox/imu", first_pose=(t0, q0))
    handed = []

    def on_keyframe(rec, edge, surf, full):
        handed.append((len(handed), rec["stamp"], [int(c.n) for c in (edge, surf, full)], [A.frontend_keyframe_get(gpu_ctx, kind) for kind in range(3)]))

    out = replay.replay(path, gpu_ctx, "/livox/lidar", "/livox/imu", first_pose=(t0, q0), keyframes=True, deskew=True, on_keyframe=on_keyframe)
    assert len(out) == len(plain) == n
    for a, b in zip(plain, out):
        assert set(b) == set(a) | {"is_kf", "rel"}
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    rule = L.KeyframeRule()
    flags = [rule.step(r["t"], r["q"], True) for r in out]
    assert [r["is_kf"] for r in out] == [f != M.KF_NO for f in flags] and sum(r["is_kf"] for r in out) == len(handed) >= 3
    # the default call's records, once more: nothing of the keyframe run leaks into it
    again = replay.replay(path, gpu_ctx, "/livox/lidar", "/livox/imu", first_pose=(t0, q0))
    for a, b in zip(plain, again):
        assert set(a) == set(b) and all(np.array_equal(a[key], b[key]) for key in a)
    # the clouds on_keyframe received = the kernel on the features the extraction call returns for that scan
    ctx2 = L.Context(0)
    try:
        kf_recs = [(f, r) for f, r in enumerate(out) if r["is_kf"]]
        for (f, r), (_, stamp, counts, clouds), flag in zip(kf_recs, handed, [fl for fl in flags if fl != M.KF_NO]):
            assert stamp == r["stamp"]
            if f > 0:
                t_rel, q_rel = L.pose_relative(out[f - 1]["t"], out[f - 1]["q"], r["t"], r["q"])
                assert np.array_equal(t_rel, r["rel"][0]) and np.array_equal(q_rel, r["rel"][1])
            scan = np.ascontiguousarray(A.livox_custom_to_cloud(ctx2, _custom(frames[f]))[:, [0, 1, 2, 8, 9]], np.float32)
            feats = features_by_extraction(ctx2, "livox", scan, r["q_imu"])
            assert counts == [x[0].shape[0] for x in feats] and counts[:2] == [r["n_edge"], r["n_surf"]]
            if flag == M.KF_FIRST:
                want = [rows[:, [0, 1, 2, a]] for rows, _, a in feats]
            else:
                want = undistort_features(ctx2, feats, r["rel"][0])
            for kind in range(3):
                assert same_bits(clouds[kind], want[kind]), (f, kind)
    finally:
        ctx2.close()
