"""The designed linearisation inputs of tests/linearize_cases.py on the CPU: the conditions on the inputs (asserted on the model alone), the oracle
(oracle.linearize_surf / linearize_edge / linearize_rows) held to the mpmath model at 1 x the allowance, the constant K re-measured, the longdouble Gram model held
to an mpmath sum, and the SENSITIVITY of the bounds: five faults applied to the oracle's output, each of which the comparison must reject."""
import functools

import mpmath
import numpy as np
import pytest

from tests import linearize_cases as C

GRID = [(v, o) for v in C.VARIANTS for o in C.OFFSETS]
# the fewest rows a family may have per kind, (origin, far): the DMIN rule of tests/linearize_cases.py drops edge rows nearer to the line than the row condition
# allows, and a later change to DMIN, to the weights or to the scene must not empty a family unnoticed
MIN_ROWS = {("huber", "s"): (16, 16), ("cauchy", "s"): (19, 19), ("none", "s"): (10, 10), ("pose", "s"): (11, 11), ("cancel", "s"): (0, 9),
            ("huber", "e"): (14, 14), ("cauchy", "e"): (13, 9), ("none", "e"): (6, 4), ("nearline", "e"): (7, 3), ("pose", "e"): (10, 10)}


@functools.lru_cache(maxsize=None)
def _oracle_records(variant, offset):
    """the oracle's own records of the probe queries: (srec, erec | None), fields (NREC, ...)"""
    from oracle import oracle as O
    s = C.scene(variant, offset)
    si, ei = C.probe_queries(variant, offset)
    PO = O.params(variant)
    livox = variant == "livox"
    q = s["surf_q"][si]
    rs = O.associate_surf(O.KdTree(s["surf_map"][:, :3]), s["surf_map"][:, 3] if livox else None, q[:, :3], q[:, 3] if livox else None, C.Q_ASSOC, C.T_ASSOC, PO)
    assert rs["valid"].all()
    erec = None
    if variant != "frontend":
        erec = O.associate_edge(O.KdTree(s["edge_map"]), s["edge_q"][ei], C.Q_ASSOC, C.T_ASSOC, PO)
        assert erec["valid"].all()
    return rs, erec


def _oracle_row(O, row, srec, erec):
    """(X (8,), Gram (8, 8), cost, count) of one probe row by the oracle, one valid record at a time"""
    kind, prm = row["kind"], row["prm"]
    rec = C._one(srec if kind == "s" else erec, row["i"])
    one = {k: np.ascontiguousarray(np.asarray(v)[None]) for k, v in rec.items()}
    one["valid"] = np.ones(1, np.uint8)
    PO = O.params(prm["variant"], **C.oracle_overrides(prm))
    scale = C.oracle_scale(prm, kind, row["N"])
    if kind == "s":
        G, cost, cnt = O.linearize_surf(one, row["t"], row["q"], PO, scale)
    else:
        G, cost, cnt = O.linearize_edge(one, row["t"], row["q"], PO, scale)
    X = O.linearize_rows(one, row["t"], row["q"], PO, scale, kind="surf" if kind == "s" else "edge")[0]
    return X, G, cost, cnt


@functools.lru_cache(maxsize=None)
def _probe(variant, offset):
    from oracle import oracle as O
    O.build(); O.lib()
    srec, erec = _oracle_records(variant, offset)
    rows = C.probe_rows(variant, offset, srec, erec)
    return [(r, C.probe_model(r, srec, erec), _oracle_row(O, r, srec, erec)) for r in rows]


def _excess(G, Gm, allow):
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(np.asarray(G, np.float64) - np.asarray(Gm, np.float64)) / allow
    e = np.where(np.isnan(np.asarray(Gm, np.float64)) & np.isnan(np.asarray(G, np.float64)), 0.0, e)
    return float(np.where(np.isnan(e), np.inf, e).max())


@pytest.mark.parametrize("variant,offset", GRID)
def test_probe_rows_conditions_and_oracle_against_the_model(oracle, variant, offset):
    worst, fams, per_kind = {}, {}, {}
    for row, m, (Xo, Go, co, cnt) in _probe(variant, offset):
        fam = row["fam"]
        fams[fam] = fams.get(fam, 0) + 1
        per_kind[(fam, row["kind"])] = per_kind.get((fam, row["kind"]), 0) + 1
        # conditions on the model alone
        if row["prm"]["loss"] == C.LOSS_HUBER:
            a = row["prm"]["loss_a"]
            assert abs(m["raw"] - a) > 1e-9 * a, (fam, m["raw"])
        norm = np.linalg.norm(m["X"])
        assert (C.DEVICE_FACTOR * C.K_EVAL * C.EPS * m["S"]).max() <= 1e-6 * norm, (fam, row["kind"], row["i"], m["raw"], (C.K_EVAL * C.EPS * m["S"]) / norm)
        # the oracle at 1 x
        G, allow, acost = C.gram_of_row(m, 1.0)
        e = max(_excess(Go, G, allow), abs(co - m["cost"]) / (acost + C.EPS * abs(m["cost"])), float((np.abs(Xo - m["X"]) / (C.K_EVAL * C.EPS * m["S"])).max()))
        assert cnt == 1 and e <= 1.0, (fam, row["kind"], row["i"], e, m["raw"])
        assert np.array_equal(Go, Go.T)
        worst[fam] = max(worst.get(fam, 0.0), e)
    print(f"\n{variant} {offset}: rows per family {fams}; worst oracle error / allowance per family { {k: round(v, 3) for k, v in worst.items()} }")
    want = {"frontend": {"huber", "none", "pose"}, "livox": {"huber", "cauchy", "none", "pose", "nearline"}, "rot": {"cauchy", "none", "pose", "nearline"}}[variant]
    assert want | ({"cancel"} if offset == "far" else set()) == set(fams)
    for (fam, kind), low in MIN_ROWS.items():
        if fam in fams and (kind == "s" or variant != "frontend"):
            assert per_kind.get((fam, kind), 0) >= low[offset == "far"], (variant, offset, fam, kind, per_kind)


def test_constant_K_is_what_the_file_uses(oracle):
    cases = [(m, o[0], o[2]) for v, off in GRID for _, m, o in _probe(v, off)]
    k = C.measure_K(cases)
    print(f"\nK measured over {len(cases)} probe rows: {k:.3f} (in use: {C.K_EVAL})")
    assert k <= C.K_EVAL
    assert len(cases) >= 300


def test_zero_and_onepoint_rows(oracle):
    """r == 0 exactly on the f32-exact plane at the identity (the sq == 0 arm), and the edge point ON its line: NaN on both sides, as with Ceres' jets"""
    O = oracle
    mp_, q = C.exact_clouds("frontend", "surf")
    rs = O.associate_surf(O.KdTree(mp_), None, q, None, C.IDENTITY[1], C.IDENTITY[0], O.params("frontend"))
    assert list(rs["valid"]) == [0, 1, 0]
    for variant, prm in (("frontend", C.params("frontend")), ("frontend", C.params("frontend", loss=C.LOSS_NONE))):
        X, cost, raw = C.row_mp("s", prm, C._one(rs, 1), 1.0, *C.IDENTITY)
        assert raw == 0.0 and X[7] == 0.0 and cost == 0.0                          # the residual really is 0
        G, c, n = O.linearize_surf(rs, *C.IDENTITY, O.params(variant, **C.oracle_overrides(prm)), 1.0)
        assert n == 1 and c == 0.0 and np.array_equal(G, np.outer(X, X))           # the arithmetic is exact: equality
    for variant in ("livox", "rot"):
        mp_, q = C.exact_clouds(variant, "edge")
        re_ = O.associate_edge(O.KdTree(mp_), q, C.IDENTITY[1], C.IDENTITY[0], O.params(variant))
        assert list(re_["valid"]) == [0, 1, 0]
        prm = C.params(variant)
        w = float(C.weight(prm, "e", re_["s"][1:2], 1)[0])
        X, cost, raw = C.row_mp("e", prm, C._one(re_, 1), w, *C.IDENTITY)
        assert raw == 0.0 and np.isnan(X[:7]).all() and X[7] == 0.0
        G, c, n = O.linearize_edge(re_, *C.IDENTITY, O.params(variant), C.oracle_scale(prm, "e", 1))
        assert n == 1 and np.isnan(G[:7, :7]).all() and G[7, 7] == 0.0            # pinned: the oracle is NaN there


@functools.lru_cache(maxsize=None)
def _list_1025(variant, kind):
    """a 1025-row list at `far` by the oracle: (prm, rec (compacted), N, pose, oracle Gram, cost)"""
    from oracle import oracle as O
    O.build(); O.lib()
    q, v = C.partition_queries(variant, "far", kind, 1025, "all")
    s = C.scene(variant, "far")
    PO = O.params(variant)
    livox = variant == "livox"
    if kind == "s":
        rec = O.associate_surf(O.KdTree(s["surf_map"][:, :3]), s["surf_map"][:, 3] if livox else None, q[:, :3], q[:, 3] if livox else None, C.Q_ASSOC, C.T_ASSOC, PO)
    else:
        rec = O.associate_edge(O.KdTree(s["edge_map"]), q, C.Q_ASSOC, C.T_ASSOC, PO)
    assert rec["count"] == int(v.sum()) == 1025
    prm = C.params(variant)
    t, qq = C.partition_pose(variant, kind)
    f = O.linearize_surf if kind == "s" else O.linearize_edge
    G, cost, cnt = f(rec, t, qq, PO, C.oracle_scale(prm, kind, 1025))
    assert cnt == 1025
    return prm, rec, 1025, (t, qq), G, cost


def _rejects(G, cost, model, also=None):
    Gm, cm, allow, acost = model
    r = _excess(G, Gm, allow) > 1.0 or abs(cost - float(cm)) > acost + C.EPS * abs(float(cm))
    return r and (also is None or _rejects(G, cost, also))


@pytest.mark.skipif(not C.BULK_OK, reason=C.BULK_SKIP)
@pytest.mark.parametrize("variant,kind", [(v, k) for v in C.VARIANTS for k in "se" if not (v == "frontend" and k == "e")])
def test_partition_lists_oracle_against_the_longdouble_model_and_the_faults_it_must_reject(oracle, variant, kind):
    O = oracle
    prm, rec, N, (t, q), Go, co = _list_1025(variant, kind)
    model = C.gram_model(kind, prm, rec, N, t, q, 1025, 1.0)
    model8 = C.gram_model(kind, prm, rec, N, t, q, 1025, C.DEVICE_FACTOR)            # the device's allowance: the faults must leave that one as well
    e = _excess(Go, model[0], model[2])
    print(f"\n{variant} {kind}: 1025 rows, worst oracle error / allowance per entry {e:.3f}; smallest |entry| / largest {np.abs(Go).min() / np.abs(Go).max():.1e}")
    assert not _rejects(Go, co, model), e
    PO = O.params(variant)
    f = O.linearize_surf if kind == "s" else O.linearize_edge
    scale = C.oracle_scale(prm, kind, N)
    # shorter lists: every tile edge up to 1025 (valid records only in the first n queries)
    for n in (1, 63, 64, 65, 1023, 1024):
        sub = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in rec.items()}
        G, c, cnt = f(sub, t, q, PO, C.oracle_scale(prm, kind, n))
        assert cnt == n and not _rejects(G, c, C.gram_model(kind, prm, sub, n, t, q, n, 1.0)), n
    # --- sensitivity: each fault must be rejected ---
    X = O.linearize_rows(rec, t, q, PO, scale, kind="surf" if kind == "s" else "edge")
    assert X.shape == (1025, 8) and not _rejects(X.T @ X, co, (model[0], co, model[2] + 64 * C.EPS * (np.abs(X).T @ np.abs(X)), np.inf))
    k = int(np.argmin(np.linalg.norm(X, axis=1)))                                  # the row that matters least
    assert _rejects(Go - np.outer(X[k], X[k]), co, model, model8), "one row of 1025 dropped"
    Gx = Go.copy(); Gx[0, 4], Gx[1, 4] = Go[1, 4], Go[0, 4]; Gx[4, 0], Gx[4, 1] = Go[1, 4], Go[0, 4]
    assert _rejects(Gx, co, model, model8), "G[0][4] and G[1][4] exchanged"
    if prm["variant"] == "rot":
        G1, c1, _ = f(rec, t, q, PO, C.oracle_scale(prm, kind, N + 1))
        assert _rejects(G1, c1, model, model8), "scaled by N + 1"
    else:
        assert _rejects(Go * (N / (N + 1.0)) ** 2, co, model, model8), "scaled by N + 1"
    if prm["loss"] != C.LOSS_NONE:
        # rho' instead of sqrt(rho') on the row with the strongest down-weighting: f = |X| / |X unrobustified|
        Xn = O.linearize_rows(rec, t, q, O.params(variant, loss=C.LOSS_NONE), scale, kind="surf" if kind == "s" else "edge")
        with np.errstate(invalid="ignore", divide="ignore"):
            fr = np.linalg.norm(X[:, :3], axis=1) / np.linalg.norm(Xn[:, :3], axis=1)
        k = int(np.argmin(fr))
        assert fr[k] < 1.0 - 1e-9
        assert _rejects(Go - np.outer(X[k], X[k]) + np.outer(fr[k] * X[k], fr[k] * X[k]), co, model, model8), "rho' for sqrt(rho') on one row"
        if prm["loss"] == C.LOSS_HUBER:
            assert _rejects(Go - np.outer(X[k], X[k]) + np.outer(Xn[k], Xn[k]), co, model, model8), "the Huber inlier branch for one outlier"


def test_huber_inlier_branch_for_an_outlier_is_rejected_on_a_probe_row(oracle):
    """the same fault on single rows: every huber row beyond the threshold, evaluated with the inlier branch (no loss), must leave the allowance"""
    O = oracle
    n = 0
    for variant, offset in (("frontend", "origin"), ("frontend", "far"), ("livox", "far")):
        srec, erec = _oracle_records(variant, offset)
        for row, m, _ in _probe(variant, offset):
            if row["fam"] != "huber" or m["raw"] <= row["prm"]["loss_a"]:
                continue
            wrong = dict(row, prm=dict(row["prm"], loss=C.LOSS_NONE))
            Xw, Gw, cw, _ = _oracle_row(O, wrong, srec, erec)
            G, allow, _ = C.gram_of_row(m, 1.0)
            assert _excess(Gw, G, allow) > 1.0, (variant, offset, m["raw"])
            n += 1
    assert n >= 20


@pytest.mark.skipif(not C.BULK_OK, reason=C.BULK_SKIP)
@pytest.mark.parametrize("variant,kind", [("rot", "s"), ("livox", "e"), ("frontend", "s")])
def test_longdouble_gram_against_an_mpmath_sum_of_the_same_rows(oracle, variant, kind):
    """the vectorised referee (its hand-written derivative of Eigen's product included) against the mpmath rows, whose Jacobians are numerical: all 1025 rows,
    summed in mpmath; the longdouble Gram may differ by the model's own allowance scaled to the longdouble eps (its rows are evaluated the same way, in the
    wider format) and its summation error, 1025 longdouble eps sum |x_a x_b|"""
    prm, rec, N, (t, q), _, _ = _list_1025(variant, kind)
    w = C.weight(prm, kind, rec["score"] if kind == "s" else rec["s"], N)
    Gm, cm, allow, acost = C.gram_model(kind, prm, rec, N, t, q, 1025, 1.0)
    eps_ld = float(np.finfo(C.LD).eps)
    with mpmath.workprec(C.PREC):
        S = [[mpmath.mpf(0)] * 8 for _ in range(8)]
        A = [[mpmath.mpf(0)] * 8 for _ in range(8)]
        cs = mpmath.mpf(0)
        for i in range(1025):
            X, c, _ = C.row_mp(kind, prm, C._one(rec, i), w[i], t, q, as_mp=True)
            cs += c
            for a in range(8):
                for b in range(a, 8):
                    p = X[a] * X[b]
                    S[a][b] += p; A[a][b] += abs(p)
        worst = 0.0
        for a in range(8):
            for b in range(a, 8):
                err = abs(mpmath.mpf(float(Gm[a, b])) + mpmath.mpf(float(Gm[a, b] - C.LD(float(Gm[a, b])))) - S[a][b])
                worst = max(worst, float(err / (eps_ld / C.EPS * allow[a, b] + 1025 * eps_ld * A[a][b])))
        cerr = float(abs(mpmath.mpf(float(cm)) + mpmath.mpf(float(cm - C.LD(float(cm)))) - cs) / (eps_ld / C.EPS * acost + 1025 * eps_ld * abs(cs)))
    print(f"\n{variant} {kind}: longdouble Gram against the mpmath sum, worst error / (allowance eps_ld / eps + 1025 eps_ld sum |x x|) = {worst:.3f}; cost error / the same {cerr:.3f}")
    assert worst <= 1.0 and cerr <= 1.0


def test_partition_cases_have_the_intended_counts():
    want = {"all": lambda n: n, "wave0_invalid": lambda n: n - 64, "block0_invalid": lambda n: n - 1024, "last_only": lambda n: 1,
            "second_trip_only": lambda n: n - 262144, "every_other": lambda n: n // 2}
    for pat in C.PATTERNS:
        for n in C.SIZES:
            if C.partition_applies(n, pat):
                v = C.validity(n, pat)
                assert v.shape == (n,) and int(v.sum()) == want[pat](n) > 0, (pat, n)
    assert int(C.validity(262145, "second_trip_only").sum()) == 1 and int(C.validity(263169, "second_trip_only").sum()) == 1025
    assert not C.validity(263169, "second_trip_only")[:262144].any() and not C.validity(1025, "block0_invalid")[:1024].any() and C.validity(524289, "last_only")[-1]
    for variant, kind in (("rot", "s"), ("livox", "e")):
        s = C.scene(variant, "far")
        q, v = C.partition_queries(variant, "far", kind, 1025, "every_other")
        inv = s["invalid"][:q.shape[1]]
        assert (q[~v] == inv).all() and not (q[v] == inv).all(1).any() and int(v.sum()) == 512
    assert [C.summation_depth(n) for n in (1, 1024, 1025, 262144, 262145, 524289)] == [89, 89, 90, 344, 408, 472]
