"""The hard cases of the loop-closure registration without a GPU (tests/icp_cases.py): the conditions on the inputs, the exact models and the numpy restatement
(tests/icp_model.py) held to each other, the constant K of the allowance re-measured, and the mutations of the restatement that the cases must catch."""
import numpy as np
import pytest

from tests import icp_cases as Cs
from tests import icp_model as M


@pytest.fixture(scope="module")
def solved():
    """every H case with its model, computed once: (case, P, Q, origin, model)"""
    out = []
    for v in Cs.VARIANTS:
        for c in Cs.h_cases(v):
            P, Q = c["src"], c["tgt"][c["partner"]]
            out.append((c, P, Q, Cs.target_origin(c["tgt"]), Cs.exact_rotation(P, Q)))
    return out


def test_partners_are_unique_nearest_neighbours():
    for v in Cs.VARIANTS:
        for c in Cs.h_cases(v):
            assert c["src"].shape[0] <= 64
            idx, d2, mult = Cs.nn_brute(c["tgt"], c["src"], multiplicity=True)
            assert np.array_equal(idx, c["partner"]) and np.all(mult == 1), c["name"]
            assert np.all(d2.astype(np.float64) <= 0.25 * c["gate"] ** 2), c["name"]


def test_families_are_what_they_claim(solved):
    by = {c["name"]: m for c, _, _, _, m in solved}
    for v in Cs.VARIANTS:
        m = by[f"{v}/reflect"]
        assert m["det_sign"] < 0 and m["unique"] and m["sigma"][1] > 10 * m["sigma"][2]
        for ax in Cs.AXES:
            for deg in Cs.ANGLES:
                m = by[f"{v}/rot_{ax}_{deg:g}"]
                assert m["det_sign"] > 0 and m["sigma"][0] > 1e3 * m["sigma"][1]
                ang = np.rad2deg(np.arccos(np.clip((np.trace(m["R"]) - 1) / 2, -1, 1)))
                assert abs(ang - deg) < 0.01, (ax, deg, ang)
            assert by[f"{v}/rank1_{ax}"]["rank"] == 1 and not by[f"{v}/rank1_{ax}"]["unique"]
        H = by[f"{v}/zerocol"]["H"]
        assert by[f"{v}/zerocol"]["rank"] == 2 and all(H[r][2] == 0 for r in range(3)) and any(H[r][0] != 0 for r in range(3))
        H = by[f"{v}/zerorow"]["H"]
        assert by[f"{v}/zerorow"]["rank"] == 2 and all(H[2][s] == 0 for s in range(3))
        for n in (3, 4, 5, 7):
            m = by[f"{v}/rank0_{n}"]
            assert m["rank"] == 0 and m["n"] == n and np.array_equal(m["R"], np.eye(3))
        s = by[f"{v}/cube_equal"]["sigma"]
        assert s[0] == s[1] == s[2] > 0 and by[f"{v}/cube_equal"]["det_sign"] > 0
        s = by[f"{v}/box_s1_eq_s2"]["sigma"]
        assert s[0] == s[1] > s[2] > 0
        s = by[f"{v}/box_s2_eq_s3"]["sigma"]
        assert s[0] > s[1] == s[2] > 0 and by[f"{v}/box_s2_eq_s3"]["det_sign"] > 0 and by[f"{v}/box_s2_eq_s3"]["unique"]
        m = by[f"{v}/reflect_s2_eq_s3"]
        assert m["det_sign"] < 0 and m["sigma"][1] == m["sigma"][2] and not m["unique"]
        s = by[f"{v}/needle"]["sigma"]
        assert s[0] > 1e8 * s[1] and s[1] > 50 * s[2] > 0      # eight decades and two more
        assert by[f"{v}/three"]["n"] == 3 and by[f"{v}/three"]["unique"]
    far = np.linalg.norm(Cs.target_origin(Cs.h_cases("decoy")[0]["tgt"]) - Cs.h_cases("decoy")[0]["src"].mean(0))
    assert 4500 < far < 5500


def test_exact_model_is_a_rotation_that_attains_its_optimum(solved):
    for c, P, Q, o, m in solved:
        if m["R"] is None:
            continue
        R = m["R"]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15, c["name"]
        assert abs(Cs.trace_RH(R, m["H"]) - m["opt"]) <= 4 * Cs.U52 * max(m["sigma"][0], 1e-300), c["name"]


def test_exact_model_against_mpmath(solved):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    for c, P, Q, o, m in solved:
        if m["rank"] == 0:
            continue
        H = mp.matrix([[mp.mpf(x.numerator) / x.denominator for x in row] for row in m["H"]])
        U, S, V = mp.svd_r(H)
        s = sorted((float(x) for x in S), reverse=True)
        for a, b in zip(s[:m["rank"]], m["sigma"]):
            assert abs(a - b) <= 1e-14 * s[0], c["name"]
        if m["rank"] == 3 and m["unique"] and m["gap"] > 1e-9 * m["sigma"][0]:
            D = mp.diag([1, 1, mp.sign(mp.det(U) * mp.det(V))])
            R = np.array((V.T * D * U.T).tolist(), dtype=np.float64)
            assert np.abs(R - m["R"]).max() < 1e-14, c["name"]


def test_restatement_within_K_and_K_is_what_the_file_says(solved, capsys):
    worst, worst_t, worst_name, capped, unique, deficits = 0.0, 0.0, None, 0, 0, 0.0
    for c, P, Q, o, m in solved:
        R, t = Cs.restated_rotation(P, Q, o)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12, c["name"]
        aR, at, S = Cs.allowance(P, Q, o, m, 1.0)
        if m["rank"] == 0:
            continue
        if not m["unique"]:
            d = m["opt"] - Cs.trace_RH(R, m["H"])
            deficits = max(deficits, abs(d) / (Cs.U52 * S))
            assert abs(d) <= Cs.K_IN_USE * Cs.U52 * S, (c["name"], d)
            if m["rank"] == 1:
                assert np.abs(R @ m["u1"] - m["v1"]).max() <= Cs.K_IN_USE * Cs.U52 * S / m["sigma"][0], c["name"]      # the line's own gap is s1
            continue
        unique += 1
        if Cs.K_IN_USE * aR > Cs.CAP:
            capped += 1
            continue
        ratio = np.abs(R - m["R"]).max() / aR
        if ratio > worst:
            worst, worst_name = ratio, c["name"]
        if at > 0:
            worst_t = max(worst_t, np.abs(t - m["t"]).max() / at)
        assert ratio <= Cs.K_IN_USE, (c["name"], ratio)
        assert np.abs(t - m["t"]).max() <= Cs.K_IN_USE * at, (c["name"], np.abs(t - m["t"]).max(), at)
    with capsys.disabled():
        print(f"\n[icp cases] K measured {worst:.3f} ({worst_name}; in use {Cs.K_IN_USE}), translation {worst_t:.3f}, non-unique tr(R H) deficit {deficits:.3f} u S, "
              f"{capped} of {unique} unique-R cases beyond the cap")
    assert worst <= Cs.K_IN_USE and abs(worst - Cs.K_MEASURED) < 0.05 * Cs.K_MEASURED      # the docstrings quote it
    assert capped <= 0.05 * unique


def test_brute_force_neighbour_and_the_walk_agree():
    """the small walk that restates icp_nn finds what brute force finds on the tie lattice and outside the box (so its mutation below means something)"""
    for c in Cs.nn_cases():
        if c["name"] not in ("lattice_ties", "line_ny1_nz1", "two_points"):
            continue
        g = Cs.grid_restate(c["tgt"])
        src = c["src"][:120]
        idx, d2 = Cs.nn_brute(c["tgt"], src)
        widx, wd2 = Cs.walk_nn(g, c["tgt"], src)
        assert np.array_equal(idx, widx) and np.array_equal(d2.view(np.uint32), wd2.view(np.uint32)), c["name"]


def test_nn_cases_hold_what_they_claim():
    by = {c["name"]: c for c in Cs.nn_cases()}
    for c in by.values():
        assert c["tgt"].shape[0] <= (4096 if c["name"] != "dense_clamp_005" else 12000) and c["src"].shape[0] <= 2048
    _, _, mult = Cs.nn_brute(by["lattice_ties"]["tgt"], by["lattice_ties"]["src"], multiplicity=True)
    assert set(np.unique(mult)) == {1, 2, 4, 8} and all((mult == k).sum() >= 15 for k in (1, 2, 4, 8))
    _, _, mult = Cs.nn_brute(by["duplicates"]["tgt"], by["duplicates"]["src"], multiplicity=True)
    assert np.all(mult >= 3)
    g = Cs.grid_restate(by["plane_nz1"]["tgt"])
    assert g["dims"][2] == 1 and g["dims"][0] > 1 and g["dims"][1] > 1
    g = Cs.grid_restate(by["line_ny1_nz1"]["tgt"])
    assert g["dims"][1] == 1 and g["dims"][2] == 1 and g["dims"][0] > 1
    assert Cs.grid_restate(by["dense_clamp_005"]["tgt"])["cell"] == pytest.approx(0.05)
    assert Cs.grid_restate(by["sparse8_clamp_50"]["tgt"])["cell"] == pytest.approx(50.0)
    g = Cs.grid_restate(by["sparse8_max_cells"]["tgt"], by["sparse8_max_cells"]["max_cells"])
    assert g["cell"] > 50.0 and np.prod(g["dims"]) <= by["sparse8_max_cells"]["max_cells"]
    c = by["blob_halo"]
    g = Cs.grid_restate(c["tgt"])
    cells = np.floor((c["tgt"].astype(np.float64) - g["o"]) * g["inv_cell"]).astype(np.int64)
    assert np.unique(cells, axis=0, return_counts=True)[1].max() >= 300      # hundreds in one cell
    c = by["outside"]
    g = Cs.grid_restate(c["tgt"])
    u = (c["src"][:104].astype(np.float64) - g["o"]) * g["inv_cell"]
    r0 = np.maximum(np.maximum(-np.floor(u), np.floor(u) - (g["dims"] - 1)), 0).max(1)
    assert np.all(r0[:26] <= 1) and np.all((r0[26:52] >= 3) & (r0[26:52] <= 4)) and np.all(r0[52:78] >= 40) and np.all(r0[78:104] >= 1000) and (r0 >= 1000).sum() <= 64
    c = by["full_scan"]
    g = Cs.grid_restate(c["tgt"])
    u = (M.apply(c["guess"], c["src"]).astype(np.float64) - g["o"]) * g["inv_cell"]
    assert np.all(np.abs(u[:, 0]) >= 2.0 ** 28)
    c = by["gate_boundary"]
    _, d2 = Cs.nn_brute(c["tgt"], c["src"])
    assert (d2 == 25.0).sum() >= 10 and 3 <= (d2 < 25.0).sum()
    c = by["non_finite"]
    assert not np.isfinite(c["tgt"][:3]).all(1).any() and (~np.isfinite(c["src"]).all(1)).sum() == 4
    # the bound queries of `cellfaces`: the best distance within 1e-5 of the first shell's lower bound f * cell
    c = by["cellfaces"]
    g = Cs.grid_restate(c["tgt"])
    q = c["src"][400:464].astype(np.float64)
    u = (q - g["o"]) * g["inv_cell"]
    f = np.minimum(u - np.floor(u), 1 - (u - np.floor(u))).min(1) * g["cell"]
    _, d2 = Cs.nn_brute(c["tgt"], c["src"][400:464])
    near = np.abs(np.sqrt(d2.astype(np.float64)) / f - 1) < 2e-5
    assert near.sum() >= 48, near.sum()      # (a random body point may come nearer: that only blunts the query)


def test_exit_cases_end_where_they_claim():
    for c in Cs.exit_cases():
        r = M.align(Cs.BruteTree(c["tgt"]), c["tgt"], c["src"], **c["kw"])
        state, it = c["want"]
        assert r["state"] == state and (it is None or r["iterations"] == it), (c["name"], r["state"], r["iterations"])
        if c["name"] == "no_corr_later":
            assert [e["n_corr"] for e in r["log"]] == [4, 3, 2]


# ---- mutations of the restatement: every one must fail a case against the exact models ----
def _nn_last(tgt, q):
    """ties to the LARGER index"""
    idx, d2 = Cs.nn_brute(tgt[::-1], q)
    return np.where(idx >= 0, tgt.shape[0] - 1 - idx, -1), d2


def _step(tgt, src, T, gate, strict=False, nn=Cs.nn_brute):
    q = M.apply(T, src)
    idx, d2 = nn(tgt, q)
    g2 = gate * gate
    acc = (d2.astype(np.float64) < g2) if strict else (d2.astype(np.float64) <= g2)
    return np.where(acc, idx, -1), int(acc.sum())


def _align(c, min_corr=3, swapped=False):
    """icp_model.align with its two constants open to mutation"""
    kw = dict(max_corr_dist=30.0, max_iterations=100, teps=1e-6, feps=1e-6)
    kw.update(c["kw"])
    tree, T, prev, it = Cs.BruteTree(c["tgt"]), np.eye(4), Cs.DMAX, 0
    while True:
        _, _, inc, mse, n = M.step(tree, c["tgt"], c["src"], T, kw["max_corr_dist"])
        if n < min_corr:
            return M.NO_CORRESPONDENCES, it
        T, it = inc @ T, it + 1
        cos, tr2 = 0.5 * (np.trace(inc[:3, :3]) - 1.0), float(inc[:3, 3] @ inc[:3, 3])
        s = M.convergence_state(it, kw["max_iterations"], cos, tr2, mse, prev, kw["teps"], kw["feps"])
        if swapped and s in (M.ABS_MSE, M.REL_MSE, M.NOT_CONVERGED) and it < kw["max_iterations"] and not (cos >= 1.0 - kw["teps"] and tr2 <= kw["teps"]):
            rel = prev != 0 and abs(mse - prev) / prev < kw["feps"]
            s = M.REL_MSE if rel else (M.ABS_MSE if abs(mse - prev) < 1e-12 else M.NOT_CONVERGED)
        prev = mse
        if s != M.NOT_CONVERGED:
            return s, it


def test_mutations_are_caught(solved):
    caught = {}
    # the det sign dropped: every reflected case
    bad = []
    for c, P, Q, o, m in solved:
        if m["unique"] and m["rank"] > 0:
            R, _ = Cs.restated_rotation(P, Q, o, det_sign=False)
            aR, _, _ = Cs.allowance(P, Q, o, m, Cs.DEVICE_FACTOR * Cs.K_IN_USE)
            if aR <= Cs.CAP and np.abs(R - m["R"]).max() > aR:
                bad.append(c["name"])
    caught["det sign dropped"] = bad
    assert "unit/reflect" in bad and "decoy/reflect" in bad
    by = {c["name"]: c for c in Cs.nn_cases()}
    # < for <= at the gate
    c = by["gate_boundary"]
    want = _step(c["tgt"], c["src"], np.eye(4), 5.0)
    got = _step(c["tgt"], c["src"], np.eye(4), 5.0, strict=True)
    assert want[1] == 27 and got[1] < want[1]
    caught["< for <= at the gate"] = ["gate_boundary"]
    # ties to the larger index
    bad = [n for n in ("lattice_ties", "duplicates", "full_scan", "all_equal")
           if not np.array_equal(_nn_last(by[n]["tgt"], M.apply(np.eye(4) if by[n]["guess"] is None else by[n]["guess"], by[n]["src"]))[0],
                                 Cs.nn_brute(by[n]["tgt"], M.apply(np.eye(4) if by[n]["guess"] is None else by[n]["guess"], by[n]["src"]))[0])]
    assert bad == ["lattice_ties", "duplicates", "full_scan", "all_equal"]
    caught["ties to the larger index"] = bad
    # the shell walk's lower bound as r + f
    c = by["lattice_ties"]
    g = Cs.grid_restate(c["tgt"])
    idx, d2 = Cs.nn_brute(c["tgt"], c["src"][:120])
    widx, wd2 = Cs.walk_nn(g, c["tgt"], c["src"][:120], bound_shift=0)
    assert not np.array_equal(idx, widx)
    caught["lower bound r + f"] = ["lattice_ties"] + (["values too"] if not np.array_equal(d2, wd2) else [])
    # n_corr < 4
    three = next(c for c, _, _, _, _ in solved if c["name"] == "unit/three")
    c3 = dict(tgt=three["tgt"], src=three["src"], kw=dict(max_iterations=1))
    assert _align(c3) == (M.ITERATIONS, 1) and _align(c3, min_corr=4) == (M.NO_CORRESPONDENCES, 0)
    ex = {c["name"]: c for c in Cs.exit_cases()}
    assert _align(ex["no_corr_later"]) == (M.NO_CORRESPONDENCES, 2) and _align(ex["no_corr_later"], min_corr=4) == (M.NO_CORRESPONDENCES, 1)
    caught["n_corr < 4"] = ["three", "no_corr_later"]
    # the ABS_MSE and REL_MSE tests swapped
    for name in ex:
        assert _align(ex[name]) == (M.align(Cs.BruteTree(ex[name]["tgt"]), ex[name]["tgt"], ex[name]["src"], **ex[name]["kw"])["state"], _align(ex[name])[1])
    assert _align(ex["abs_before_rel"]) == (M.ABS_MSE, 2) and _align(ex["abs_before_rel"], swapped=True) == (M.REL_MSE, 2)
    caught["ABS_MSE / REL_MSE swapped"] = ["abs_before_rel"]
    assert all(caught.values())
