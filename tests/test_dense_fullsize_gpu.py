"""configs[2] variant B at full size: the 5 M-point map of bench_configs.make_variant_b (~170 points per gate-sized cell, ~84 M fine cells) read in place
from device memory, as bench_configs.config2b builds it.  The dense-map association (k_associate_fine) is held to an f32 brute force bit for bit at the
true pose (almost every query settles in its inner 27 fine cells) and at the 0.1 m / 0.5 deg start pose (a third of the first launch goes to the rings of
super-rows), in random and in scan order, with queries off the surfaces and outside the map; to the oracle's kd-tree; to the gate-sized index alone and to
the exact selector bit for bit; and one registration to the oracle's.  The map is built once, in a context of its own."""
import os

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from tests import dense_grid_model as M
from tests.knn_brute import BruteKnn5

pytestmark = pytest.mark.gpu

IPS = 10


def _world(q_local, Q2, T2):
    from oracle import oracle as O
    return O.transform_cloud(np.c_[q_local, np.zeros(q_local.shape[0], np.float32)], Q2, T2)[:, :3]      # transformPoint, f32 out


@pytest.fixture(scope="module")
def vb(oracle):
    import torch
    import bench_configs
    mp, q_local, t_true, q_true = bench_configs.make_variant_b()
    q_plain = q_local.copy()
    _, q_scan, _, _ = bench_configs.make_variant_b(scan_order=True)
    assert mp.shape[0] == 5_000_000 and q_local.shape[0] == 200_000
    rng = np.random.default_rng(0xB5)
    n_q = q_local.shape[0]
    # ~2 % of the queries 0.2-0.9 m off the surfaces (several ring levels), a few outside the map box, some of them beyond the gate
    q_conj = q_true * np.array([1, -1, -1, -1])
    qw = synth.quat_rot(q_true, q_local.astype(np.float64)) + t_true
    off = rng.choice(n_q, n_q // 50, replace=False)
    d = rng.normal(size=(off.size, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    qw[off] += d * rng.uniform(0.2, 0.9, (off.size, 1))
    out = rng.choice(np.setdiff1d(np.arange(n_q), off), 60, replace=False)
    qw[out[:30], 2] = -rng.uniform(0.1, 0.9, 30)                  # below the floor: outside the box, inside the gate
    qw[out[30:], 2] = -rng.uniform(1.2, 3.0, 30)                  # beyond the gate
    q_local = synth.quat_rot(q_conj, qw - t_true).astype(np.float32)
    perm = _row_permutation(q_plain, q_scan)           # q_scan == q_plain[perm]: the generator's scan order, applied to the displaced set
    q_scan = np.ascontiguousarray(q_local[perm])
    ctx = L.Context(0)
    try:
        P = L.make_params("rot")
        m = L.ScanToMapMatcher(ctx, P)
        m.map_focus(None)
        d_map = torch.from_numpy(mp).cuda()
        cloud = L.api.cloud_from_device(d_map.data_ptr(), mp.shape[0], 12, -1)
        stats0 = m.map_build_stats()
        m.set_input_cloud(L.KIND_SURF, cloud)                      # a fresh context: the box is measured
        stats1 = m.map_build_stats()
        ctx.set_debug(True)
        tb, qb = L.api.body_pose_from_lidar(t_true, q_true, P)
        t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(synth.SEED_POSE), 0.1, 0.5)
        sel3k = np.sort(np.r_[rng.choice(np.setdiff1d(np.arange(n_q), out), 2970, replace=False), out[30:]])     # with the 30 beyond the gate
        v = dict(mp=mp, q_local=q_local, q_scan=q_scan, perm=perm, off=off, out=out, t_true=t_true, q_true=q_true, tb=tb, qb=qb, t0=t0, q0=q0,
                 ctx=ctx, m=m, P=P, cloud=cloud, d_map=d_map, stats=(stats0, stats1), sel3k=sel3k, density=m.map_density(L.KIND_SURF))
        v["first"] = _assoc_3k(v)                                  # the records of the first build (the second build below must reproduce them)
        v["brute"], v["tree"] = BruteKnn5(mp), oracle.KdTree(mp)
        yield v
    finally:
        ctx.close()


def _row_permutation(a, b):
    """perm with b == a[perm] (the rows of b are those of a, reordered)."""
    ka, kb = a.view(np.dtype((np.void, a.dtype.itemsize * a.shape[1]))).ravel(), b.view(np.dtype((np.void, b.dtype.itemsize * b.shape[1]))).ravel()
    oa, ob = np.argsort(ka, kind="stable"), np.argsort(kb, kind="stable")
    perm = np.empty(a.shape[0], np.int64)
    perm[ob] = oa
    assert np.array_equal(a[perm], b)
    return perm


def _assoc_3k(v):
    """the 3 000-query sample at the start pose through slot 3: (count, neighbours, records, Gram, cost)."""
    m, P = v["m"], v["P"]
    q = np.ascontiguousarray(v["q_local"][v["sel3k"]])
    Q2, T2 = L.api.assoc_transform(v["t0"], v["q0"], P)
    m.set_queries(3, L.KIND_SURF, q)
    n = m.find_corresponding_surf_features(3, Q2, T2)
    idx, d2 = m.neighbors(3, L.KIND_SURF, q.shape[0])
    rec = m.surf_records(3, q.shape[0])
    G, cost, counts = m.linearize(3, v["t0"], v["q0"], L.MASK_SURF)
    return n, idx, d2, rec, G, cost


def _same(a, b, inside):
    na, ia, da, ra, Ga, ca = a
    nb, ib, db, rb, Gb, cb = b
    assert na == nb
    assert np.array_equal(ia[inside], ib[inside]) and np.array_equal(da[inside].view(np.uint32), db[inside].view(np.uint32))
    for k in ("query_index", "cp", "n", "d", "score"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(Ga, Gb) and ca == cb


def _angle(qa, qb):
    dq = synth.quat_mul(np.asarray(qa) * np.array([1, -1, -1, -1]), np.asarray(qb) / np.linalg.norm(qb))
    return 2 * np.arcsin(min(1.0, np.linalg.norm(dq[1:])))


def test_fullsize_fine_index_matches_the_model(vb):
    """lili_map_density of the first build (its box measured: a fresh context) equals tests/dense_grid_model.py bit for bit."""
    assert vb["stats"][0] == (0, 0, 0) and vb["stats"][1][0] == 0
    occ, fcell, fr2 = vb["density"]
    mn, mx = M.box_of(vb["mp"])
    fg, fc_model, fb_model = M.fine_index(mn, mx, 1.0, occ)
    assert occ > 100 and fg is not None
    assert fcell == fc_model and fr2 == fb_model, (fcell, fc_model, fr2, fb_model)
    assert fg.n_cells > 50_000_000                                 # the full-size fine index (~84 M cells)


def test_fullsize_bruteforce_at_true_and_start_pose_in_both_orders(vb):
    """96 queries — on the surfaces, 0.2-0.9 m off them, outside the map box — of the 200 k-query launch, random and scan order, at the true pose
    and at the 0.1 m / 0.5 deg start pose: neighbours and f32 distances equal the brute force bit for bit."""
    m, P = vb["m"], vb["P"]
    rng = np.random.default_rng(96)
    plain = np.setdiff1d(np.arange(vb["q_local"].shape[0]), np.r_[vb["off"], vb["out"]])
    sample = np.r_[rng.choice(plain, 64, replace=False), rng.choice(vb["off"], 24, replace=False),
                   rng.choice(vb["out"][:30], 4, replace=False), rng.choice(vb["out"][30:], 4, replace=False)]
    inv = np.empty_like(vb["perm"]); inv[vb["perm"]] = np.arange(vb["perm"].size)
    fr2 = vb["density"][2]
    poses = {"true": (vb["q_true"], vb["t_true"]), "start": L.api.assoc_transform(vb["t0"], vb["q0"], P)}
    for name, (Q2, T2) in poses.items():
        want_i, want_d = vb["brute"].query(_world(vb["q_local"][sample], Q2, T2))
        inside = want_d[:, 4] < 1.0
        assert inside.sum() > 80 and (~inside).sum() >= 3, (name, inside.sum())
        # the sample straddles the radius the fine index covers completely (settled in the inner block / rings of super-rows)
        assert (want_d[inside, 4] < fr2).sum() > 30 and (want_d[inside, 4] > fr2).sum() > 5, name
        for order, q, rows in (("random", vb["q_local"], sample), ("scan", vb["q_scan"], inv[sample])):
            m.set_queries(0, L.KIND_SURF, q)
            m.find_corresponding_surf_features(0, Q2, T2)
            idx, d2 = m.neighbors(0, L.KIND_SURF, q.shape[0])
            gi, gd = idx[rows], d2[rows]
            bad = np.nonzero(((gi != want_i) | (gd.view(np.uint32) != want_d.view(np.uint32))).any(1) & inside)[0]
            assert bad.size == 0, (name, order, sample[bad][:5], gi[bad][:2], want_i[bad][:2], gd[bad][:2], want_d[bad][:2])
            assert np.all(~(gd[~inside][:, 4] < 1.0))             # never a false accept


def test_fullsize_second_build_guesses_the_box_and_keeps_the_records(vb):
    """A second lili_map_set of the same device cloud with the default options starts from the guessed box with the dense hint (its gate-sized
    index without super-rows): one more guess, no miss, and the records of the first build bit for bit."""
    m = vb["m"]
    g0, miss0, fb0 = m.map_build_stats()
    m.set_input_cloud(L.KIND_SURF, vb["cloud"])
    g1, miss1, fb1 = m.map_build_stats()
    assert (g1 - g0, miss1 - miss0, fb1 - fb0) == (1, 0, 0)
    assert m.map_density(L.KIND_SURF)[1] > 0
    again = _assoc_3k(vb)
    inside = vb["first"][2][:, 4] < 1.0
    assert inside.sum() > 2800
    _same(vb["first"], again, inside)


def test_fullsize_oracle_gate_sized_index_and_exact_selector(vb, oracle):
    """3 000 queries at the start pose: counts, query_index and cp equal the oracle's kd-tree; the gate-sized index alone (fine_grid = 0) and every
    query through the exact selector (LILI_DEBUG bit 32768) give the same neighbours, records and Gram bit for bit."""
    m, P, ctx = vb["m"], vb["P"], vb["ctx"]
    PO = oracle.params("rot")
    q = np.ascontiguousarray(vb["q_local"][vb["sel3k"]])
    Q2, T2 = L.api.assoc_transform(vb["t0"], vb["q0"], P)
    base = _assoc_3k(vb)
    o = oracle.associate_surf(vb["tree"], None, q, None, Q2, T2, PO)
    inside = o["nn_d2"][:, 4] < 1.0
    assert base[0] == o["count"] > 2000 and (~inside).sum() > 0
    assert np.array_equal(base[1][inside], o["nn_idx"][inside]) and np.array_equal(base[2][inside], o["nn_d2"][inside])
    rec, v = base[3], np.nonzero(o["valid"])[0]
    assert np.array_equal(rec["query_index"], v) and np.array_equal(rec["cp"], o["cp"][v])
    np.testing.assert_allclose(rec["n"], o["n"][v], rtol=3e-7, atol=1e-9)
    np.testing.assert_allclose(rec["d"], o["d"][v], rtol=3e-7, atol=1e-9)
    np.testing.assert_allclose(rec["score"], o["score"][v], rtol=3e-7)
    try:
        os.environ["LILI_DEBUG"] = "32768"
        exact = _assoc_3k(vb)
    finally:
        os.environ.pop("LILI_DEBUG", None)
    _same(base, exact, inside)
    try:
        ctx.set_option("fine_grid", 0)
        m.set_input_cloud(L.KIND_SURF, vb["cloud"])
        assert m.map_density(L.KIND_SURF)[1] == 0.0
        coarse = _assoc_3k(vb)
    finally:
        ctx.set_option("fine_grid", 1)
        m.set_input_cloud(L.KIND_SURF, vb["cloud"])
    assert m.map_density(L.KIND_SURF)[1] > 0
    _same(base, coarse, inside)


def test_fullsize_registration_and_iterate_restart(vb, oracle):
    """One registration of 10 outer iterations on a fixed 20 k-query subset from the start pose equals the oracle's within 1e-4 m / 1e-4 rad; and
    iterate_restart(2 x 10, restart every 10) equals two rounds of pose_copy + iterate(10) bit for bit."""
    import bench_configs
    m, P = vb["m"], vb["P"]
    PO = oracle.params("rot")
    sub = np.ascontiguousarray(vb["q_local"][np.sort(np.random.default_rng(20).choice(vb["q_local"].shape[0], 20_000, replace=False))])
    m.set_queries(4, L.KIND_SURF, sub)
    m.pose_set(1, vb["t0"], vb["q0"])
    m.pose_copy(4, 1)
    m.iterate(4, IPS, L.MASK_SURF)
    t1, q1, st1 = m.pose_get(4)
    to, qo, applied, counts = oracle.register_surf(vb["tree"], sub, vb["t0"], vb["q0"], PO, 1000.0, IPS, min(16, bench_configs.usable_threads()))
    assert st1 == 0 and applied == IPS and counts[-1] > 10_000
    assert np.abs(t1 - to).max() < 1e-4 and _angle(q1, qo) < 1e-4, (np.abs(t1 - to).max(), _angle(q1, qo))
    assert np.abs(t1 - vb["tb"]).max() < 0.05                     # and it moved towards the true pose from 0.1 m off
    m.pose_copy(4, 1)
    m.iterate(4, IPS, L.MASK_SURF)
    m.pose_copy(4, 1)
    m.iterate(4, IPS, L.MASK_SURF)
    t2, q2, st2 = m.pose_get(4)
    m.pose_set(4, vb["tb"], vb["qb"])                               # (a different pose in the slot: the restart must replace it)
    m.iterate_restart(4, 2 * IPS, IPS, 1, L.MASK_SURF)
    t3, q3, st3 = m.pose_get(4)
    assert st2 == st3 == 0
    assert np.array_equal(t2, t3) and np.array_equal(q2, q3) and np.array_equal(t1, t3) and np.array_equal(q1, q3)
