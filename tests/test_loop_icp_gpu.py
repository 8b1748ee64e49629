"""Loop-closure registration on the MI355X (lili_loop_cloud / lili_icp_*) against the numpy restatement (tests/icp_model.py)."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from lili_om_amd.loop import LOOP_SOURCE, LOOP_TARGET, default_icp_params
from tests import icp_model as M

pytestmark = pytest.mark.gpu


def _rot(axis, deg):
    a = np.deg2rad(deg)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _quat(R):
    return L.loop.quat_from_matrix(R)


@pytest.fixture(scope="module")
def world():
    """jittered samples of the synthetic outdoor scene (two independent samplings: a revisit never sees the same points)"""
    sc = synth.OutdoorScene()
    a = sc.sample_surfaces(45.0, 45.0, 0.5, np.random.default_rng(11)).astype(np.float32)
    b = sc.sample_surfaces(45.0, 45.0, 0.5, np.random.default_rng(12)).astype(np.float32)
    return a, b


def _keyframe(W, t, R, radius=22.0, seed=0):
    """the points of W within `radius` of t in the keyframe's frame, with an aux column; split into (edge, surf)"""
    sel = W[np.linalg.norm(W[:, :2] - t[:2], axis=1) < radius]
    loc = ((sel.astype(np.float64) - t) @ R).astype(np.float32)
    aux = np.random.default_rng(seed).uniform(0, 1, (loc.shape[0], 1)).astype(np.float32)
    rows = np.concatenate([loc, aux], 1)
    return rows[::9].copy(), np.delete(rows, np.s_[::9], 0).copy()


def _path(n):
    """keyframe poses on a loop that returns to its start"""
    ts, Rs = [], []
    for k in range(n):
        a = 2 * np.pi * k / n
        ts.append(np.array([20 * np.cos(a), 20 * np.sin(a), 1.8]))
        Rs.append(_rot([0, 0, 1], np.rad2deg(a) + 90))
    return ts, Rs


def _tree(O, tgt):
    return O.KdTree(np.ascontiguousarray(tgt[:, :3]))


def test_assembly_bit_exact_host_and_device(oracle, gpu_ctx, world):
    import torch
    ts, Rs = _path(12)
    kfs = [_keyframe(world[0], ts[k], Rs[k], radius=12.0, seed=k) for k in range(12)]
    q_bl, t_bl = np.array([0.999, 0.01, -0.02, 0.03]), np.array([0.1, -0.05, 0.2])
    q_bl /= np.linalg.norm(q_bl)
    for variant in ("livox", "rot"):
        lc = L.LoopClosure(gpu_ctx, variant=variant, lc_map_width=3, q_bl=q_bl, t_bl=t_bl)
        latest, his = 9, 2
        qs = [_quat(R) for R in Rs]
        edge = [k[0] for k in kfs]
        surf = [k[1] for k in kfs]
        dev = [[torch.from_numpy(a).cuda() for a in k] for k in kfs]
        dedge = [L.api.cloud_from_device(d[0].data_ptr(), d[0].shape[0], 16, 12) for d in dev]
        dsurf = [L.api.cloud_from_device(d[1].data_ptr(), d[1].shape[0], 16, 12) for d in dev]
        for which, kf in ((LOOP_SOURCE, lc.source_keyframes(latest)), (LOOP_TARGET, lc.target_keyframes(latest, his))):
            clouds, tt, qq = [], [], []
            for k in kf:
                t, q = L.api.keyframe_map_pose(ts[k], qs[k], t_bl, q_bl)
                clouds += [edge[k], surf[k]]
                tt += [t, t]
                qq += [q, q]
            want = M.assemble(oracle, clouds, tt, qq, 0.4)
            for e_, s_ in ((edge, surf), (dedge, dsurf)):
                lc.assemble(latest, his, np.array(ts), np.array(qs), e_, s_)
                got = lc.get_cloud(which)
                assert got.shape == want.shape, (variant, which, got.shape, want.shape)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (variant, which)
        assert len(lc.source_keyframes(latest)) == (1 if variant == "livox" else 6)
        torch.cuda.synchronize()


def _pair(world, drift_t=(0.4, -0.3, 0.05), drift_deg=3.0):
    """target: keyframes around the start of the loop at their true poses; source: the revisit's keyframe from the second sampling, placed at a drifted pose.
    Returns (source rows, target rows, D) with source = D applied to true world points."""
    ts, Rs = _path(24)
    sel = np.zeros(world[0].shape[0], bool)
    for k in (22, 23, 0, 1, 2):
        sel |= np.linalg.norm(world[0][:, :2] - ts[k][:2], axis=1) < 22.0
    tgt = world[0][sel]
    D = np.eye(4)
    D[:3, :3] = _rot([0.2, 0.3, 1.0], drift_deg)
    D[:3, 3] = drift_t
    src_w = world[1][np.linalg.norm(world[1][:, :2] - ts[0][:2], axis=1) < 22.0]
    src = ((src_w.astype(np.float64) @ D[:3, :3].T) + D[:3, 3]).astype(np.float32)
    return src, tgt, D


def test_one_step_bit_identical_correspondences(oracle, gpu_ctx, world):
    src, tgt, D = _pair(world)
    lc = L.LoopClosure(gpu_ctx)
    lc.set_cloud(LOOP_SOURCE, src)
    lc.set_cloud(LOOP_TARGET, tgt)
    tree = _tree(oracle, tgt)
    guess = np.eye(4)
    guess[:3, 3] = (0.05, 0.02, -0.01)
    for gate in (30.0, 0.3):      # the small gate rejects a share
        p = default_icp_params()
        p.max_iterations, p.max_corr_dist = 1, gate
        res = lc.align(guess.reshape(-1), p)
        idx, d2 = lc.correspondences(src.shape[0])
        widx, wd2, inc, mse, n = M.step(tree, tgt, src, guess, gate)
        q = M.apply(guess, src)
        _, d5 = tree.knn5(q)
        unique = d5[:, 0] < d5[:, 1]
        assert np.array_equal(d2.view(np.uint32), wd2.view(np.uint32)), gate
        assert np.array_equal(idx[unique], widx[unique]), gate
        if gate < 1:
            assert 0 < (idx < 0).sum() < src.shape[0]
        assert res["iterations"] == 1 and res["state"] == M.ITERATIONS and res["log"][0]["n_corr"] == n
        assert abs(res["log"][0]["mse"] - mse) <= 1e-12 * max(mse, 1e-30)
        Tg = np.asarray(res["transform"]) @ np.linalg.inv(guess)
        assert np.abs(Tg - inc).max() < 1e-9, np.abs(Tg - inc).max()


def test_planar_and_collinear_sources(oracle, gpu_ctx):
    rng = np.random.default_rng(5)
    tgt = np.concatenate([rng.uniform(-5, 5, (3000, 2)), rng.normal(0, 0.02, (3000, 1))], 1).astype(np.float32)      # a plane
    src = tgt[::3] + np.float32([0.05, -0.03, 0.0])
    lc = L.LoopClosure(gpu_ctx)
    lc.set_cloud(LOOP_TARGET, tgt)
    lc.set_cloud(LOOP_SOURCE, np.concatenate([src[:, :2], np.zeros((src.shape[0], 1), np.float32)], 1))      # exactly planar source: rank-2 H
    p = default_icp_params()
    p.max_iterations = 1
    res = lc.align(None, p)
    _, _, inc, _, _ = M.step(_tree(oracle, tgt), tgt, np.concatenate([src[:, :2], np.zeros((src.shape[0], 1), np.float32)], 1), np.eye(4), 30.0)
    assert np.abs(res["transform"] - inc).max() < 1e-9
    line = np.stack([np.linspace(-4, 4, 200), np.zeros(200), np.zeros(200)], 1).astype(np.float32)       # collinear source: any valid rotation
    lc.set_cloud(LOOP_SOURCE, line)
    res = lc.align(None, p)
    R = res["transform"][:3, :3]
    assert np.all(np.isfinite(res["transform"]))
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9


def test_full_run_equals_chained_steps_and_the_model(oracle, gpu_ctx, world):
    src, tgt, D = _pair(world)
    lc = L.LoopClosure(gpu_ctx, lc_icp_thres=0.2)
    lc.set_cloud(LOOP_SOURCE, src)
    lc.set_cloud(LOOP_TARGET, tgt)
    full = lc.align()
    assert full["converged"]
    states, it = M.replay_states(full["log"], 100)
    assert states == [e["state"] for e in full["log"]] and it == full["iterations"]
    # chained single iterations: bit for bit per iteration
    p1 = default_icp_params()
    p1.max_iterations = 1
    T = np.eye(4)
    for k in range(min(full["iterations"], 5)):
        one = lc.align(T.reshape(-1), p1)
        pk = default_icp_params()
        pk.max_iterations = k + 1
        part = lc.align(None, pk)
        assert np.array_equal(part["transform"], one["transform"]), k
        assert part["log"][k]["mse"] == one["log"][0]["mse"] == full["log"][k]["mse"], k
        T = one["transform"]
    # the independent model
    tree = _tree(oracle, tgt)
    want = M.align(tree, tgt, src)
    dT = full["transform"] @ np.linalg.inv(want["transform"])
    assert np.abs(dT[:3, 3]).max() < 1e-5 and np.arccos(np.clip((np.trace(dT[:3, :3]) - 1) / 2, -1, 1)) < 1e-5
    fm, _ = M.fitness(tree, tgt, src, full["transform"])
    assert abs(full["fitness"] - fm) <= 1e-5 * fm
    # the recovered correction undoes the injected drift
    E = full["transform"] @ D
    assert np.linalg.norm(E[:3, 3]) < 0.02
    assert np.rad2deg(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))) < 0.2
    assert full["fitness"] <= 0.2
    assert full["host_syncs"] <= 4      # batches of 8, 16, 32, 64 cover 100 iterations


def test_fitness_is_exact_and_ungated(oracle, gpu_ctx, world):
    src, tgt, D = _pair(world)
    far = np.float32([[200.0, 10.0, 3.0], [-80.0, 150.0, -20.0], [0.0, 0.0, 90.0]])
    src = np.concatenate([src[::4], far], 0)
    lc = L.LoopClosure(gpu_ctx)
    lc.set_cloud(LOOP_SOURCE, src)
    lc.set_cloud(LOOP_TARGET, tgt)
    tree = _tree(oracle, tgt)
    T = np.linalg.inv(D)
    for rng_max in (np.finfo(np.float64).max, 1.0):
        f, n = lc.fitness(T.reshape(-1), rng_max)
        fm, nm = M.fitness(tree, tgt, src, T, rng_max)
        assert n == nm and abs(f - fm) <= 1e-12 * fm, (f, fm)
    assert n < src.shape[0]


def test_edge_cases(gpu_ctx):
    ctx = L.Context(0)
    try:
        lc = L.LoopClosure(ctx)
        r = L.api.IcpResult()
        rc = ctx.lib.lili_icp_align(ctx.h, C.byref(default_icp_params()), None, C.byref(r))
        assert rc == -3      # LILI_E_STATE: no cloud yet
        tgt = np.random.default_rng(1).uniform(-1, 1, (500, 3)).astype(np.float32)
        lc.set_cloud(LOOP_TARGET, tgt)
        lc.set_cloud(LOOP_SOURCE, tgt[:50] + np.float32([100.0, 0, 0]))
        guess = np.eye(4)
        guess[0, 3] = 0.5
        res = lc.align(guess.reshape(-1))
        assert not res["converged"] and res["state"] == M.NO_CORRESPONDENCES and res["iterations"] == 0
        assert np.array_equal(res["transform"], guess)
    finally:
        ctx.close()


def test_loop_calls_leave_the_rest_of_the_context_alone(gpu_ctx, world):
    """the same local-map / voxel-filter / matcher sequence with and without loop calls interleaved on the same context, and with a second context
    registering at the same time: identical maps, statistics and association counts"""
    src, tgt, _ = _pair(world)
    room = synth.make_room(seed=3, n_query=2000, n_edge_query=200)
    P = L.make_params("rot")
    ts, Rs = _path(24)
    kfs = [_keyframe(world[0], ts[k], Rs[k], seed=k) for k in range(6)]

    def run(with_loop, other=None):
        ctx = L.Context(0)
        try:
            lc = L.LoopClosure(ctx)
            lm = L.LocalMap(ctx, L.KIND_SURF, width=4, leaf=0.4)
            m = L.ScanToMapMatcher(ctx, P)
            out = []
            for k in range(6):
                if with_loop:
                    lc.set_cloud(LOOP_TARGET, tgt)
                    lc.set_cloud(LOOP_SOURCE, src)
                    lc.align()
                if other is not None:
                    other.align()
                t, q = ts[k], _quat(Rs[k])
                lm.push(kfs[k][1], t, q)
                if with_loop:
                    lc.assemble(5, 1, np.array(ts), np.array([_quat(R) for R in Rs]), [a[0] for a in kfs] * 4, [a[1] for a in kfs] * 4)
                out.append(lm.commit())
                out.append(lm.get(400000).tobytes())
                out.append(L.api.voxel_filter(ctx, kfs[k][1], 0.4)[0].tobytes())
                m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
                m.set_queries(0, L.KIND_SURF, room["q_xyz"])
                t_body, q_body = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
                Q2, T2 = L.api.assoc_transform(t_body, q_body, P)
                out.append(m.find_corresponding_surf_features(0, Q2, T2))
            out.append(lm.stats())
            out.append(L.api.voxel_filter_stats(ctx))
            return out
        finally:
            ctx.close()

    base = run(False)
    assert run(True) == base
    ctx2 = L.Context(0)
    try:
        lc2 = L.LoopClosure(ctx2)
        lc2.set_cloud(LOOP_TARGET, tgt)
        lc2.set_cloud(LOOP_SOURCE, src)
        assert run(False, other=lc2) == base
    finally:
        ctx2.close()
