"""The conditions on the inputs of tests/test_edge_fit_gpu.py, on the oracle alone (cases, model and margin rule: tests/edge_fit_cases.py).

For every case, at both offsets and for both parameter sets: the oracle's five neighbours are the query's own cluster; every kind is where it claims
to be; the oracle's valid flags equal the model's gates on every decided cluster; its A and B equal the model's within one f32 ulp per component (on
tied clusters as an unordered pair); the undecided clusters, the deliberately rotated exact-3 ones aside, are at most 1 % of a case — so the GPU test
cannot hide behind exclusions; and each case holds at least 20 accepted and 20 rejected decided clusters."""
import numpy as np
import pytest

from tests import edge_fit_cases as E

GRID = [(c, o, v) for c in E.CASES for o in E.OFFSETS for v in E.VARIANTS]


@pytest.mark.parametrize("case,offset,variant", GRID)
def test_oracle_meets_the_model_on_every_case(oracle, case, offset, variant):
    s, rec, m = E.reference(case, offset, variant)
    n, kind = s["n"], s["kind"]
    print(case, offset, variant, E.summary(case, offset, variant))
    # the neighbours: the query's own cluster, in the order of the f32 distances (ties by index), the distances bit for bit
    own = 5 * np.arange(n)[:, None] + np.arange(5)[None, :]
    assert np.array_equal(np.sort(rec["nn_idx"], axis=1), own)
    assert np.array_equal(rec["nn_d2"].view(np.uint32), m["d2"].view(np.uint32))
    d = rec["nn_d2"]
    assert (np.diff(d, axis=1) >= 0).all() and ((np.diff(d, axis=1) > 0) | (np.diff(rec["nn_idx"], axis=1) > 0)).all()
    bi, bd = oracle.knn5_brute(s["map_xyz"], s["q_map"][:64])
    assert np.array_equal(bi, rec["nn_idx"][:64]) and np.array_equal(bd, rec["nn_d2"][:64])
    assert (d[kind != "egate"][:, 4] < 0.75).all()
    # every kind is where it claims to be
    r = m["ratio"]
    is_ = lambda k: kind == k
    if case == "generic":
        assert (r[is_("line") | is_("graded") | is_("huge")] > 10).all()
        assert (r[is_("iso")] < 1).all()
        assert m["diagonal"][is_("prolate")].all() and (m["ev"][is_("prolate"), 0] == m["ev"][is_("prolate"), 1]).any()
        ex = is_("exact")
        assert (np.abs(m["ev"][ex, 1]) <= 1e-14 * m["ev"][ex, 2]).all()                      # rank one: ev[1] is rounding noise ...
        assert (m["ev"][ex, 1] < 0).any() or (m["ev"][ex, 0] < 0).any()                       # ... of either sign
        dup = np.nonzero(is_("dup"))[0]
        assert (m["ev"][dup[:10]] == 0).all() and not m["valid"][dup[:10]].any()              # five coincident points: the zero matrix, refused
        assert (m["ev"][dup[10:], 2] > 0).all() and (np.abs(m["ev"][dup[10:], 1]) <= 1e-14 * m["ev"][dup[10:], 2]).all()
        g = m["ev"][is_("graded")]
        assert (g[:, 1] < 1e-6 * g[:, 2]).all()
        b = r[is_("band")]
        assert (b > 1).sum() >= 20 and (b < 1).sum() >= 20 and np.abs(b - 1).min() < 1e-3
    if case == "aligned":
        ax = is_("axis") | is_("box")
        assert m["diagonal"][ax].all()                                                        # no sweep runs: the sort alone decides
        lead = np.argmax(np.abs(m["u"][ax]), axis=1)
        assert set(lead.tolist()) == {0, 1, 2} and (np.abs(m["u"][ax]).max(1) == 1.0).all()
        bx = r[is_("box")]
        assert (bx > 1).sum() >= 20 and (bx < 1).sum() >= 20 and np.abs(bx - 1).min() < 2e-4
        dg = is_("diag")
        assert (m["tied"] & dg).sum() >= 100                                                  # the f32-exact diagonals are ties
        assert (m["gap"][dg] < 5e-3).all() and not m["diagonal"][dg].any()
    if case == "exact3":
        e3 = is_("exact3")
        assert (r[e3] == 1.0).all() and m["diagonal"][e3].all()                               # ratio exactly 3 ...
        assert not rec["valid"][e3].any() and not m["valid"][e3].any()                        # ... refused by the strict gate, on both sides
        up = is_("ulp")
        assert m["decided"][up].all() and (np.abs(r[up] - 1) > 1e-8).all()
        assert (r[up] > 1).sum() >= 100 and (r[up] < 1).sum() >= 100                          # decided cases of both outcomes
        assert (np.abs(r[is_("rot345")] - 1) < 1e-12).all() and not m["diagonal"][is_("rot345")].any()
    if case == "gates":
        la = is_("lateral")
        assert np.abs(m["dist"][la] - 0.1).max() < 0.011
        if offset == "origin":
            assert (np.abs(m["dist"][la] - 0.1) < 1e-6).sum() >= 100                          # (the 500 m lattice quantises the query at 3e-5 .. 6e-5 m)
        assert ((m["dist"][la] > 0.1).sum() >= 50) and ((m["dist"][la] < 0.1).sum() >= 50)
        eg = d[is_("egate"), 4]
        assert (eg < 1).sum() >= 20 and (eg >= 1).sum() >= 20 and np.abs(eg.astype(np.float64) - 1).min() < 1e-5
    # valid flags: the model's gates on every decided cluster
    dec = m["decided"]
    assert np.array_equal(rec["valid"][dec].astype(bool), m["valid"][dec]), np.nonzero(dec & (rec["valid"].astype(bool) != m["valid"]))[0][:10]
    # A and B: one f32 ulp per component; tied clusters as an unordered pair
    ok = dec & m["valid"]
    close = E.pair_close(rec["a"], rec["b"], m["A"], m["B"], m["tied"])
    assert close[ok].all(), (np.nonzero(ok & ~close)[0][:10], kind[ok & ~close][:10])
    assert (rec["s"][ok] == np.float32(oracle.params(variant).lidar_const)).all()
    # the cap on exclusions, and both outcomes present
    und = ~dec & (kind != "rot345")
    assert und.sum() <= 0.01 * n, (und.sum(), kind[und])
    assert (dec & m["valid"]).sum() >= 20 and (dec & ~m["valid"]).sum() >= 20


def test_short_map_refuses_every_query(oracle):
    s = E.short_map()
    for variant in E.VARIANTS:
        rec = oracle.associate_edge(oracle.KdTree(s["map_xyz"]), s["q_local"], E.Q_ASSOC, E.T_ASSOC, oracle.params(variant))
        assert rec["count"] == 0 and not rec["valid"].any()


def test_dense_filler_is_dense_and_out_of_reach():
    """the filler lifts the point-weighted mean occupancy of the gate-sized cells over the fine index's threshold of 12 with a margin, and no filler point is
    within 2.5 m of a query (asserted over a seventh of the queries by the generator, over all of them here for one case)"""
    for case in E.CASES:
        for offset in E.OFFSETS:
            s, f = E.build(case, offset), E.dense_filler(case, offset)
            assert E.occupancy(np.r_[s["map_xyz"], f]) > 15
    s, f = E.build("gates", "far"), E.dense_filler("gates", "far")
    q = s["q_map"].astype(np.float64)
    assert min(np.linalg.norm(f.astype(np.float64) - p, axis=1).min() for p in q) > 2.5
