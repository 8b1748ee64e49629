"""Loop-closure registration on the MI355X (lili_loop.hip) held to the exact models of tests/icp_cases.py: the nearest neighbour on hard grids
(ties, duplicates, queries outside the box, cell faces, degenerate grids, both cell clamps, the max_cells growth, the full-scan branch, non-finite points,
hints beyond the gate, the gate at equality), the rotation on hard H (reflection, turns up to 180 degrees, zero row / column, ranks 2, 1, 0, equal
singular values, a needle, three scales, an origin 4.9 km away) and every exit of the convergence rule, at the batch edges and past the log.

Measured (K: the CPU's numpy restatement against the 60-digit model, tests/test_icp_cases_cpu.py; the device is allowed 8 K):
  K = 5.11 (in use 5.5), made by cube_turned, where S / g = 1 / 2 and the figure is the SVD's own few ulps; every other case stays below 2.4.
  MI355X, worst |R - R_model| / (2^-52 S / g) over the unique-R cases: 5.11 (kilo/cube_turned, 5.6e-16 absolute; 2.04 at scale 1 and 1e-3; 1.24 with the
  origin 4.9 km away, decoy/rot_z_90).  Translation: at most 1.21 of its allowance at K = 1.
  Cases beyond the 1e-3 cap: 1 of 116 (decoy/needle: g = 2.4e-4 under sums of 8e8), on the CPU and on the device alike.
  Non-unique cases (rank 1; reflected with s2 = s3): tr(R H) deficit 0 at the resolution of f64 on every one (allowed 44 x 2^-52 S).
Fault found: three, five or seven identical accepted source points (rank 0) left H = S - n pm qm^T as the rounding of its sums (1.3 ulp of S), of which
icp_rotation made a rotation of 90 degrees and more (unit/rank0_3, milli/rank0_3, decoy/rank0_3 on the parent; four points cancel exactly).  k_icp_step now
takes an H below 64 ulp of the sums for zero: R = I.  Everything else passed on the code as it stood.
"""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from lili_om_amd.api import ICP_MAX_LOG
from lili_om_amd.loop import LOOP_SOURCE, LOOP_TARGET, default_icp_params
from tests import icp_cases as Cs
from tests import icp_model as M
from tests.test_loop_icp_gpu import _pair

pytestmark = pytest.mark.gpu


def _params(gate=30.0, iters=1, teps=1e-6, feps=1e-6):
    p = default_icp_params()
    p.max_corr_dist, p.max_iterations, p.transformation_epsilon, p.euclidean_fitness_epsilon = gate, iters, teps, feps
    return p


def _set(ctx, tgt, src):
    lc = L.LoopClosure(ctx)
    lc.set_cloud(LOOP_TARGET, np.ascontiguousarray(tgt, np.float32))
    lc.set_cloud(LOOP_SOURCE, np.ascontiguousarray(src, np.float32))
    return lc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the rotation ----
@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_rotation_on_a_forced_H(gpu_ctx, variant):
    worst_R, worst_t, worst_tr, capped, unique = 0.0, 0.0, 0.0, 0, 0
    K = Cs.DEVICE_FACTOR * Cs.K_IN_USE
    for c in Cs.h_cases(variant):
        name = c["name"]
        idx0, _, mult = Cs.nn_brute(c["tgt"], c["src"], multiplicity=True)
        assert np.array_equal(idx0, c["partner"]) and np.all(mult == 1), name      # the precondition: H is the chosen one
        lc = _set(gpu_ctx, c["tgt"], c["src"])
        res = lc.align(None, _params(gate=c["gate"]))
        idx, _ = lc.correspondences(c["src"].shape[0])
        assert np.array_equal(idx, c["partner"]), name
        assert res["iterations"] == 1 and res["state"] == M.ITERATIONS and res["log"][0]["n_corr"] == c["src"].shape[0], name
        T = res["transform"]
        R, t = T[:3, :3], T[:3, 3]
        assert np.array_equal(T[3], [0, 0, 0, 1]) and np.all(np.isfinite(T)), name
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12, name
        P, Q = c["src"], c["tgt"][c["partner"]]
        m = Cs.exact_rotation(P, Q)
        o = Cs.target_origin(c["tgt"])
        aR, at, S = Cs.allowance(P, Q, o, m, 1.0)
        if m["rank"] == 0:
            pm, qm = np.array([float(x) for x in m["pm"]]), np.array([float(x) for x in m["qm"]])
            assert np.array_equal(R, np.eye(3)), (name, R)
            # the means are formed about o and o is added back: four roundings at the size of the largest of the three
            assert np.abs(t - m["t"]).max() <= Cs.DEVICE_FACTOR * np.spacing(max(np.abs(pm).max(), np.abs(qm).max(), np.abs(o).max())), (name, t, m["t"])
            continue
        if not m["unique"]:
            d = m["opt"] - Cs.trace_RH(R, m["H"])
            worst_tr = max(worst_tr, abs(d) / (Cs.U52 * S))
            print(f"{name}: tr(R H) deficit {d:.3e} = {d / (Cs.U52 * S):.3f} u S")
            assert abs(d) <= K * Cs.U52 * S, (name, d)
            if m["rank"] == 1:
                assert np.abs(R @ m["u1"] - m["v1"]).max() <= K * Cs.U52 * S / m["sigma"][0], name
            continue
        unique += 1
        if Cs.K_IN_USE * aR > Cs.CAP:      # not evidence (the same cases as on the CPU)
            capped += 1
            continue
        eR, et = np.abs(R - m["R"]).max(), np.abs(t - m["t"]).max()
        worst_R = max(worst_R, eR / aR)
        worst_t = max(worst_t, et / at) if at > 0 else worst_t
        print(f"{name}: R {eR:.3e} = {eR / aR:.3f} of 2^-52 S / g ({aR:.2e}), t {et:.3e} of {at:.2e}")
        assert eR <= K * aR, (name, eR, aR)
        assert et <= K * at, (name, et, at)
    print(f"[{variant}] device worst R ratio {worst_R:.3f}, t ratio {worst_t:.3f} (allowed {K}), tr deficit {worst_tr:.3f} u S, {capped} of {unique} beyond the cap")
    assert capped <= 0.05 * unique + 1


# ---- the nearest neighbour ----
NN = {c["name"]: c for c in Cs.nn_cases()}


@pytest.mark.parametrize("name", list(NN))
def test_nearest_neighbour_for_every_query(gpu_ctx, name):
    c = NN[name]
    ctx = L.Context(0) if "max_cells" in c else gpu_ctx
    try:
        if "max_cells" in c:
            ctx.set_option("max_cells", c["max_cells"])
        tgt, src = c["tgt"], c["src"]
        lc = _set(ctx, tgt, src)
        G = np.eye(4) if c["guess"] is None else c["guess"]
        tree = Cs.BruteTree(tgt)
        for gate in c["gates"]:
            res = lc.align(None if c["guess"] is None else G.reshape(-1), _params(gate=gate))
            idx, d2 = lc.correspondences(src.shape[0])
            widx, wd2, _, mse, n = M.step(tree, tgt, src, G, gate)
            assert np.array_equal(idx, widx), (name, gate, np.nonzero(idx != widx)[0][:10])
            assert np.array_equal(_bits(d2), _bits(wd2)), (name, gate)
            e = res["log"][0]
            assert e["n_corr"] == n and abs(e["mse"] - mse) <= 1e-12 * mse, (name, gate, e, mse, n)
            assert (res["state"], res["iterations"]) == ((M.ITERATIONS, 1) if n >= 3 else (M.NO_CORRESPONDENCES, 0)), (name, gate)
            assert np.all(np.isfinite(res["transform"])) and np.isfinite(e["mse"]) and np.isfinite(res["fitness"]), (name, gate)
        for max_range in c["fit"]:
            f, nf = lc.fitness(G.reshape(-1), max_range)
            fm, nm = M.fitness(tree, tgt, src, G, max_range)
            assert nf == nm and nm > 0 and abs(f - fm) <= 1e-12 * fm, (name, max_range, f, fm, nf, nm)
        if name == "gate_boundary":      # d2 = 25 exactly: accepted at 5, rejected at the next double below
            acc = []
            for g in c["gates"]:
                lc.align(None, _params(gate=g))
                acc.append(int((lc.correspondences(src.shape[0])[0] >= 0).sum()))
            exact = int((Cs.nn_brute(tgt, src)[1] == 25.0).sum())
            assert acc[0] == src.shape[0] and acc[1] == src.shape[0] - exact and exact >= 10
        if name == "non_finite":
            idx, _ = lc.correspondences(src.shape[0])
            assert np.all(idx[~np.isfinite(src).all(1)] == -1) and not np.isin(idx, np.nonzero(~np.isfinite(tgt).all(1))[0]).any()
            assert lc.fitness(np.eye(4).reshape(-1))[1] == src.shape[0] - 4
    finally:
        if ctx is not gpu_ctx:
            ctx.close()


@pytest.mark.parametrize("name,gate", [("lattice_ties", 30.0), ("lattice_ties", 0.45), ("blob_halo", 30.0), ("blob_halo", 5.0)])
def test_hinted_search_equals_a_fresh_one(gpu_ctx, name, gate):
    """the second iteration starts every walk at the first one's match: its correspondences equal those of a fresh align started from the first transform,
    bit for bit, and both equal the brute-force neighbour — also where the hinted point lies beyond the gate"""
    c = NN[name]
    tgt = c["tgt"]
    src = c["src"]      # the lattice's queries as they are: exact ties in the first iteration, their winners the hints of the second
    if name == "blob_halo":
        src = (src.astype(np.float64) @ Cs.rot((1, -2, 3), 2.0).T + [0.11, -0.07, 0.05]).astype(np.float32)
    lc = _set(gpu_ctx, tgt, src)
    one = lc.align(None, _params(gate=gate, iters=1, teps=-1.0, feps=-1.0))
    two = lc.align(None, _params(gate=gate, iters=2, teps=-1.0, feps=-1.0))
    assert two["iterations"] == 2 and one["iterations"] == 1
    idx2, d22 = lc.correspondences(src.shape[0])
    fresh = lc.align(one["transform"].reshape(-1), _params(gate=gate, iters=1, teps=-1.0, feps=-1.0))
    idxf, d2f = lc.correspondences(src.shape[0])
    assert np.array_equal(idx2, idxf) and np.array_equal(_bits(d22), _bits(d2f))
    assert np.array_equal(two["transform"], fresh["transform"])
    widx, wd2, _, mse, n = M.step(Cs.BruteTree(tgt), tgt, src, one["transform"], gate)
    assert np.array_equal(idx2, widx) and np.array_equal(_bits(d22), _bits(wd2))
    assert two["log"][1]["n_corr"] == n >= 3
    if gate < 30.0:      # some hinted points lie beyond the gate in the second iteration
        hint, _ = Cs.nn_brute(tgt, M.apply(np.eye(4), src))
        dh = M.d2_f32(tgt[hint], M.apply(one["transform"], src)).astype(np.float64)
        assert (dh > gate * gate).sum() >= 3 and (idx2 < 0).sum() >= 3


# ---- the exits ----
EXITS = {c["name"]: c for c in Cs.exit_cases()}


def _same_run(res, want, name):
    assert res["state"] == want["state"] and res["iterations"] == want["iterations"] and res["converged"] == want["converged"], (name, res["state"], res["iterations"])
    n = min(len(want["log"]), ICP_MAX_LOG)
    assert len(res["log"]) == n, name
    assert [e["n_corr"] for e in res["log"]] == [e["n_corr"] for e in want["log"][:n]], name
    assert [e["state"] for e in res["log"]] == [e["state"] for e in want["log"][:n]], name


@pytest.mark.parametrize("name", list(EXITS))
def test_every_exit(gpu_ctx, name):
    c = EXITS[name]
    kw = dict(max_corr_dist=30.0, max_iterations=100, teps=1e-6, feps=1e-6)
    kw.update(c["kw"])
    want = M.align(Cs.BruteTree(c["tgt"]), c["tgt"], c["src"], **kw)
    assert want["state"] == c["want"][0] and (c["want"][1] is None or want["iterations"] == c["want"][1])
    lc = _set(gpu_ctx, c["tgt"], c["src"])
    res = lc.align(None, _params(kw["max_corr_dist"], kw["max_iterations"], kw["teps"], kw["feps"]))
    _same_run(res, want, name)
    assert np.abs(res["transform"] - want["transform"]).max() <= 1e-9, name
    if want["state"] == M.NO_CORRESPONDENCES:      # iterations counts the completed ones, and the transform is the last completed one's
        if want["iterations"] == 0:
            assert np.array_equal(res["transform"], np.eye(4))
        else:
            cut = lc.align(None, _params(kw["max_corr_dist"], want["iterations"], kw["teps"], kw["feps"]))
            assert cut["state"] == M.ITERATIONS and np.array_equal(cut["transform"], res["transform"])


@pytest.fixture(scope="module")
def long_run():
    """the `world` pair of tests/test_loop_icp_gpu.py cut to 400 source points, and the model's run past the log (both epsilons -1), computed once"""
    sc = synth.OutdoorScene()
    a = sc.sample_surfaces(45.0, 45.0, 0.5, np.random.default_rng(11)).astype(np.float32)
    b = sc.sample_surfaces(45.0, 45.0, 0.5, np.random.default_rng(12)).astype(np.float32)
    src, tgt, _ = _pair((a, b))
    src = np.ascontiguousarray(src[::src.shape[0] // 400][:400])
    want = M.align(Cs.BruteTree(tgt), tgt, src, max_iterations=ICP_MAX_LOG + 5, teps=-1.0, feps=-1.0)
    return src, tgt, want


def _batches(launches, max_iterations):
    """read-backs of lili_icp_align: batches of 8, 16, 32, ... cut to max_iterations, until the one that holds launch number `launches`"""
    done, batch, syncs = 0, 8, 0
    while True:
        done += min(batch, max_iterations - done)
        syncs += 1
        if done >= launches:
            return syncs, done
        batch *= 2


def test_iterations_at_batch_edges_and_past_the_log(gpu_ctx, long_run):
    src, tgt, want = long_run
    lc = _set(gpu_ctx, tgt, src)
    runs = {}
    for k in (8, 9, 24, 25, 56, 57, ICP_MAX_LOG + 5):
        res = lc.align(None, _params(30.0, k, -1.0, -1.0))
        runs[k] = res
        # the model's run with max_iterations = k is the prefix of its longest one: the count is asked first
        if want["iterations"] >= k:
            exp = dict(state=M.ITERATIONS, iterations=k, converged=True, log=[dict(e) for e in want["log"][:k]])
            exp["log"][-1]["state"] = M.ITERATIONS
        else:
            exp = want      # ABS_MSE ended the longest run early: the device must say the same
        _same_run(res, exp, k)
        assert len(res["log"]) == min(res["iterations"], ICP_MAX_LOG)
        syncs, enq = _batches(res["iterations"], k)
        assert res["host_syncs"] == syncs and res["iterations_enqueued"] == enq, (k, res["host_syncs"], res["iterations_enqueued"])
        for a, b in zip(res["log"], want["log"]):
            assert abs(a["mse"] - b["mse"]) <= 1e-9 * b["mse"], k
    longest = runs[ICP_MAX_LOG + 5]
    for k, res in runs.items():      # every run is the prefix of the longest one, bit for bit
        n = min(len(res["log"]), len(longest["log"]))
        for a, b in zip(res["log"][:n], longest["log"][:n]):
            assert (a["mse"], a["cos_angle"], a["translation_sqr"], a["n_corr"]) == (b["mse"], b["cos_angle"], b["translation_sqr"], b["n_corr"]), k
    for k in (8, 24, 56):            # and its transform continues into the next: one more iteration from T_k is T_(k+1)
        if runs[k + 1]["iterations"] == k + 1:
            nxt = lc.align(runs[k]["transform"].reshape(-1), _params(30.0, 1, -1.0, -1.0))
            assert np.array_equal(nxt["transform"], runs[k + 1]["transform"]), k
    dT = longest["transform"] @ np.linalg.inv(want["transform"])
    assert np.abs(dT - np.eye(4)).max() < 1e-6
