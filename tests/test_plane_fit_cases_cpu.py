"""The conditions on the inputs of tests/test_plane_fit_hard_gpu.py, and the oracle held to the exact model (cases, model and margins: tests/plane_fit_cases.py).

For every case, at both offsets and for every parameter set: the scene is what it claims (own clusters as neighbours in the order of the f32 distances, every
foreign point more than 2.9 m from every query, f32-exact kinds round-trip — asserted by the builder —, every kind where it says it is); the oracle's valid
flags are the model's on every decided query; its records are within one f32 ulp + 1 x the measured bound of the exact solution on EVERY rank-decided query
with B <= 0.1 (K is the oracle's own worst error, so it keeps 1 x everywhere by definition; up to 0.1 the first-order statement about n^ holds); the scores are
the float weight's; the strict gates decide the exact-equality kinds as derived; the NaN kinds are dropped; undecided queries outside the kinds that are
undecided by construction are at most 5 % of a case; every gate kind has decided queries of both outcomes; every rho decade is populated.  The measured
constants are printed and must not exceed the ones the bounds are built from.  Where oracle/_ref exists, the reference's own findCorrespondingSurfFeatures
gives the oracle's valid set and records bit for bit on the gate cases."""
import numpy as np
import pytest

from tests import plane_fit_cases as P

CPU_B_MAX = 0.1


def _foreign_distance(s):
    """the smallest distance from a query to a map point that is not of its cluster"""
    mp, q = s["map_xyz"].astype(np.float64), s["q_map"].astype(np.float64)
    owner = np.repeat(np.arange(s["nc"]), 5)
    best = np.inf
    for a in range(0, s["n"], 128):
        d = np.linalg.norm(q[a:a + 128, None, :] - mp[None, :, :], axis=2)
        d[owner[None, :] == s["cl"][a:a + 128, None]] = np.inf
        best = min(best, float(d.min()))
    return best


def test_the_bounds_are_built_from_the_measured_constants(oracle):
    k_qr, k_ls, k_c = P.measure_constants()
    print(f"\nmeasured: K (plain eps cond) {k_qr:.4g}, K_ls (with the residual term) {k_ls:.4g}, K_c {k_c:.4g}; in use {P.K_QR}, {P.K_LS}, {P.K_C}; the device gets {P.DEVICE_FACTOR} x")
    assert k_qr <= P.K_QR <= 1.25 * k_qr and k_ls <= P.K_LS <= 1.25 * k_ls and k_c <= P.K_C <= 1.25 * k_c


@pytest.mark.parametrize("case,offset,variant", P.GRID)
def test_oracle_meets_the_model_on_every_case(oracle, case, offset, variant):
    s, rec = P.reference(case, offset, variant)
    m = P.model(case, offset, variant, "qr")                                       # the oracle solves by the pivoted QR everywhere
    T = m["T"]
    n, kind = s["n"], s["kind"]
    is_ = lambda k: kind == k                                                      # noqa: E731
    print(case, offset, variant, P.summary(case, offset, variant, "qr"))
    # the neighbours: the query's own cluster in the order of the f32 distances (ties by index), the distances bit for bit; nothing foreign within 2.9 m
    assert np.array_equal(rec["nn_idx"], m["idx"]) and np.array_equal(rec["nn_d2"].view(np.uint32), m["d2"].view(np.uint32))
    bi, bd = oracle.knn5_brute(s["map_xyz"], s["q_map"][:64])
    assert np.array_equal(bi, rec["nn_idx"][:64]) and np.array_equal(bd, rec["nn_d2"][:64])
    assert _foreign_distance(s) > 2.9
    assert (m["d2"][~is_("kgate")][:, 4] < 0.75).all()
    # every kind is where it claims to be
    if case == "generic":
        for lo, hi in P.RHO_BANDS:
            assert (is_("strip") & (m["rho"] >= lo) & (m["rho"] < hi)).sum() >= 20, (lo, hi)
        assert (is_("strip") & (m["rho"] < P.RHO_SWITCH) & m["decided"] & m["meaningful"]).sum() >= 20        # the QR side of the switch is compared, not only counted
        t0 = is_("through0")
        # (the f32 grid tilts a 0.3 m patch by ~1e-7 rad at `origin` and ~1e-4 rad at `far`: times the 76 m / 700 m to the origin that is where the fitted plane passes it)
        reach = np.median(m["ninv"][t0] / np.maximum(np.linalg.norm(s["centre"][s["cl"]][t0], axis=1), 1.0))
        assert reach < 1e-3 and (offset == "far" or (m["ninv"][t0] < 1e-4).sum() >= 20) and (m["rho"][t0] < P.RHO_SWITCH).mean() > 0.5
        assert m["rank_full"].all() and (m["cond"][is_("tiny")] > 1e3).all()
    if case == "rank":
        z = is_("zerocol")
        assert (m["zero_cols"][z] == 1).all() and m["rank_deficient"][z].all() and (m["rho"][z] == 0).all()
        axis = np.argmax((s["map_xyz"][m["idx"]] == 0).all(1), axis=1)
        assert (m["nhat"][z, axis[z]] == 0).all() and len(set(axis[z].tolist())) == (1 if offset == "far" else 3)
        assert (z & m["decided"] & m["valid"]).sum() >= 40 and (z & m["decided"] & ~m["valid"]).sum() >= 10
        nr = is_("nearrank")
        small = np.argmin(np.abs(s["map_xyz"][m["idx"]]).max(1), axis=1)              # the column that holds nothing but the one tiny entry
        assert m["rank_full"][nr].all() and (m["sig_ratio"][nr] < 1.4e-12).sum() >= 6 and (np.abs(m["nhat"][nr, small[nr]]) > 0.999999).mean() > 0.75
        for k in ("tilt0", "colgen", "colaxis", "dup"):
            assert not m["rank_full"][is_(k)].any(), k
        assert not m["solved"][is_("tilt0")].any()                                # det(A^T A) is exactly 0: the plane passes the origin
    if case == "gates":
        d = is_("dgate") & m["decided"]
        rel = m["rmax"][is_("dgate")] / T["surf_dist_thres"] - 1.0
        assert (d & m["plane_ok"] & m["valid"]).sum() >= 50 and (d & ~m["plane_ok"]).sum() >= 50 and np.abs(rel).min() < (1e-3 if offset == "far" else 1e-6) and np.abs(rel).max() < 0.11
        w = is_("wgate") & m["decided"]
        assert (w & m["valid"]).sum() >= 40 and (w & m["plane_ok"] & ~m["weight_ok"]).sum() >= 40
        assert np.abs(m["w_exact"][is_("wgate")] - T["surf_weight_min"]).min() < 1e-5
        k = is_("kgate")
        assert m["decided"][k].all() and (k & m["valid"]).sum() >= 40 and (k & ~m["in_radius"]).sum() >= 40 and np.abs(m["d2"][k, 4].astype(np.float64) - 1).min() < 1e-4
        assert (m["valid"] == m["in_radius"])[k].all()                            # the radius alone decides them
        if offset == "origin":                                                     # pairs one f32 ulp of weight apart on the two f32 neighbours of the threshold
            lo, hi = P.f32_neighbours(T["surf_weight_min"])
            at_lo, at_hi = is_("wulp") & (m["w_chain"] == lo) & m["plane_ok"], is_("wulp") & (m["w_chain"] == hi) & m["plane_ok"]
            assert at_lo.sum() >= 4 and at_hi.sum() >= 4 and (at_lo | at_hi)[is_("wulp")].all(), (at_lo.sum(), at_hi.sum())
            assert not rec["valid"][at_lo].any() and rec["valid"][at_hi].all()     # the float weight promoted against the double literal decides
    if case == "refl":
        assert (m["sum_w"][is_("refl_eq")] == 15).all() and (m["sum_w"][is_("refl_lo")] < 15).all() and (m["sum_w"][is_("refl_hi")] > 15).all()
        assert m["decided"][is_("refl_eq")].all() and m["valid"][is_("refl_eq")].all() and rec["valid"][is_("refl_eq")].all()          # the gate is a strict >
        assert m["valid"][is_("refl_lo")].all() and not m["valid"][is_("refl_hi")].any() and not rec["valid"][is_("refl_hi")].any()
        sp = is_("refl_span")
        assert (m["w"][sp].max(1) / m["w"][sp].min(1) >= 10).all() and m["valid"][sp].all()
        for k in ("refl_zero1", "refl_zero5", "refl_inf0"):
            assert m["nan_drop"][is_(k)].all() and m["refl_ok"][is_(k)].all() and m["decided"][is_(k)].all(), k
        i0 = is_("refl_inf0")
        assert ((s["map_xyz"][m["idx"]][i0] == 0).any(2) & (s["map_refl"][m["idx"]][i0] == s["q_refl"][i0, None])).any(1).all()              # inf * 0
    if case == "dexact":
        dx = is_("dexact")
        z0, axis = P.DEXACT[variant]
        assert dx.sum() == 12 and (m["rmax"][dx] == T["surf_dist_thres"]).all() and T["surf_dist_thres"] == z0 and (m["ninv"][dx] == z0).all() and (m["nhat"][dx, axis] == -1).all()
        assert (m["zero_cols"][dx] == 2).all() and (m["idx"][dx, 0] == 5 * s["cl"][dx]).all()                                   # the origin itself is the nearest neighbour: row 0
        assert m["plane_ok"][dx].all() and m["valid"][dx].all() and rec["valid"][dx].all()                                       # |residual| == threshold: the strict > accepts
    if case == "reflwide":
        rw = is_("refl_wide")
        span = (m["w"][rw].max(1) / m["w"][rw].min(1)) ** 2
        assert (span >= 1e3).sum() >= 60 and span.max() > 6e4 and (rw & m["valid"]).sum() >= 100 and (rw & ~m["refl_ok"]).sum() >= 10
    # the NaN route: dropped, on both sides
    assert not rec["valid"][m["nan_drop"]].any() and not m["valid"][m["nan_drop"]].any()
    # valid flags: the model's gates on every decided query
    dec, o_valid = m["decided"], rec["valid"].astype(bool)
    bad = dec & (o_valid != m["valid"])
    assert not bad.any(), (kind[bad][:10], np.nonzero(bad)[0][:10])
    # records against the exact solution: one f32 ulp + 1 x the measured bound
    both = o_valid & m["rank_decided"] & (m["B"] <= CPU_B_MAX)
    worst, at, _ = P.record_excess(rec["n"], rec["d"], m, both, 1.0)
    print(f"  records: worst err / (ulp + B) {worst:.3f} on {int(both.sum())} queries (a {kind[at]} query, B {m['B'][at]:.3g})")
    assert worst <= 1.0, (worst, at, kind[at])
    z = o_valid & m["rank_deficient"]
    assert (rec["n"][z, np.argmax((s["map_xyz"][m["idx"]] == 0).all(1), axis=1)[z]] == 0).all()                               # the basic solution: nothing along a zero column
    # scores and the query itself
    lc = oracle.params(variant).lidar_const
    sc = rec["score"][o_valid]
    if variant == "frontend":
        assert (sc == 1.0).all()
    elif variant == "rot":
        wq = sc / lc
        assert np.array_equal(wq, wq.astype(np.float32).astype(np.float64))        # the weight is a float
        assert (np.abs(wq - m["w_chain"][o_valid].astype(np.float64)) <= np.spacing(m["w_chain"][o_valid]).astype(np.float64))[m["rank_decided"][o_valid] & (m["B"][o_valid] <= 1e-6)].all()
    else:
        ok = m["rank_decided"][o_valid] & (m["B"][o_valid] <= 1e-6)
        want = lc * (m["w_chain"][o_valid].astype(np.float64) + np.exp(-m["sum_w"][o_valid]))
        assert (np.abs(sc - want) <= 2.0 ** -23 * np.abs(want))[ok].all()
    assert np.array_equal(rec["cp"][o_valid], s["q_local"][o_valid])
    # the caps, on the bounds of the default and the always-QR run of the GPU test: the exclusions cannot carry the test (the fast-path-everywhere run takes
    # clusters below the switch through a determinant with relative error eps / rho: what is undecided there is printed, not capped)
    outside = ~np.isin(kind, P.UNDECIDED_BY_CONSTRUCTION)
    for mode in ("default", "qr"):
        und = ~P.model(case, offset, variant, mode)["decided"] & outside
        assert und.sum() <= 0.05 * n, (mode, int(und.sum()), n)


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_short_map_refuses_every_query(oracle, variant):
    s = P.short_map(variant)
    livox = variant == "livox"
    rec = oracle.associate_surf(oracle.KdTree(s["map"][:, :3]), s["map"][:, 3] if livox else None, s["q"][:, :3], s["q"][:, 3] if livox else None, P.Q_ASSOC, P.T_ASSOC,
                                oracle.params(variant))
    assert rec["count"] == 0 and not rec["valid"].any()


def test_dense_filler_is_dense_and_out_of_reach():
    """the filler lifts the point-weighted mean occupancy of the gate-sized cells over the fine index's threshold of 12 with a margin, and no filler point is
    within 2.5 m of a query (asserted over a seventh of the queries by the generator, over all of them here)"""
    for case, offset, variant in P.GRID:
        if variant == "frontend":
            continue
        s, f = P.build(case, offset, variant), P.dense_filler(case, offset, variant)
        assert f.shape[1] == (4 if variant == "livox" else 3)
        assert P.occupancy(np.r_[s["map_xyz"], f[:, :3]]) > 15
        q, ff = s["q_map"].astype(np.float64), f[:, :3].astype(np.float64)
        assert min(np.linalg.norm(ff - p, axis=1).min() for p in q[::3]) > 2.5


@pytest.mark.parametrize("case,offset,variant", [g for g in P.GRID if g[0] in ("gates", "refl", "dexact") and g[2] != "frontend"])
def test_the_reference_decides_the_gates_as_the_oracle_does(oracle, case, offset, variant):
    """the solver there is the oracle's restatement of Eigen's; the gates are the reference's own text (surf_weight_min is a literal in it: the configs' value)"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref is not built")
    s = P.build(case, offset, variant)
    PO = oracle.params(variant, **{k: v for k, v in P.overrides(case, offset, variant).items() if k != "surf_weight_min"})
    livox = variant == "livox"
    rec = oracle.associate_surf(oracle.KdTree(s["map_xyz"]), s["map_refl"] if livox else None, s["q_local"], s["q_refl"] if livox else None, P.Q_ASSOC, P.T_ASSOC, PO)
    if case == "dexact":
        assert rec["valid"][s["kind"] == "dexact"].all()
    rng = np.random.default_rng(3)
    edge_map = np.c_[rng.normal(0, 1, (8, 3)) + 1000.0, np.zeros(8)].astype(np.float32)
    srec, _ = ref.backend_associate(variant, np.c_[s["map_xyz"], s["map_refl"]], edge_map, np.c_[s["q_local"], s["q_refl"]], edge_map[:1], P.Q_ASSOC, P.T_ASSOC,
                                    PO.kd_max_radius, PO.surf_dist_thres, PO.lidar_const, PO.reflect_thres)
    v = rec["valid"].astype(bool)
    mine = np.c_[rec["cp"][v], rec["n"][v], rec["d"][v], rec["score"][v]].astype(np.float64)
    assert 0 < v.sum() and (v.sum() < v.size or case == "dexact")
    assert mine.shape == srec.shape and np.array_equal(mine, srec)
