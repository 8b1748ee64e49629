"""The linearisation (k_linearize, k_linearize_window, k_reduce_partials and the fused tail: surf_lin_geom / surf_lin_scale / edge_lin_row / GramAcc / lin_surf_body /
lin_edge_body, lili_s2m_dev.h; robustify / loss_eval, lili_device_math.h) on the designed inputs of tests/linearize_cases.py — families, model, allowances and
their derivation are described there; tests/test_linearize_cases_cpu.py holds the oracle to the same model and shows that the bounds reject five planted faults.

1. Probe rows: one record linearised alone (a slot of three queries of which it is the only valid one, several such slots per linearize_window call; imported
   counts through counts_import + linearize_dev).  The Gram of one row is its outer product: every entry, the cost and the counts are held to the mpmath row
   within 8 x the allowance and to the oracle (fed the device's records) within the joint 9 x; the Gram is exactly symmetric.
2. Partition: whole Grams of n = 1 .. 524 289 queries (wave tile, block, block cap, second and third grid-stride trip) under six validity patterns, per entry
   against the numpy.longdouble model; a second call gives identical bytes; rot also with an imported global count.
3. Launch structures that add the same numbers in the same order: default, fuse_tail 0 / 1, merge_kinds 0, linearize_window with the slot first / in the middle /
   last, linearize_dev into a caller's buffer — bit-identical; accumulate (which re-associates at the device pose) bit-identical to associate_dev + linearize_dev
   from the same pose.
4. Launches that linearise inside the association (fuse_lin with fuse_lin_block 0 / 64 / 256, assoc_lpq 2 / 4 / 8 / 16; rot with count_barrier = 1 through the
   in-launch count barrier where its grid is small enough — the rot legs that are not eligible take the staged launches and must give the staged step's bits):
   the Gauss-Newton step of iterate(slot, 1) against the step solved in longdouble from the model's Gram, within the first-order norm bound and the tighter
   componentwise one, and against the step of the staged launches within the two summation trees' bound alone.
5. The zero row (r == 0 exactly) and the onepoint row (nu == 0): NaN where the oracle is NaN, a non-zero step status that leaves the pose alone, and a healthy
   registration (three iterations, status 0, the pose moves) afterwards in the same context.

Measured on an MI355X, worst error / allowance (every test prints its own): probe rows against the model (of 8 x) huber 0.065, cauchy 0.119, none 0.119, cancel
0.061, nearline 0.063, pose 0.088 — below one eighth: the device is as close to the model as the oracle is (0.97 of 1 x); against the oracle (of 9 x) 0.106.  Whole
Grams against the longdouble model 0.087 (one edge record alone; 0.03 and less from 63 records on: the allowance adds magnitudes, the errors add as a random
walk), the same at 524 289 queries as at 1025.  Step of the on-the-fly launches: |error| 3e-16 .. 8e-15 against a norm bound of 2e-8 .. 2e-7 at cond(H) ~ 5e4 (1e-7
of it: cond(H) times 8 x the allowance is the worst case), 1e-3 and less of the componentwise bound, 1e-3 and less of the summation-only bound against the staged
step; every eligible leg but two (the front-end's and livox's 1025-query scene: 5 of 7) differs from the staged step in some bit, rot through the count barrier
in 4 of 4 (1025) and 2 of 2 (9000: 2 and 4 lanes) eligible legs, and its 3 / 5 legs that are not eligible are bit-identical to it.  The launch structures of
test 3 are bit-identical, the zero row is exact, the onepoint Gram is NaN where the oracle's is."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import linearize_cases as C

pytestmark = pytest.mark.gpu

GRID = [(v, o) for v in C.VARIANTS for o in C.OFFSETS]
MASK = {"s": L.MASK_SURF, "e": L.MASK_EDGE}
KIND = {"s": L.KIND_SURF, "e": L.KIND_EDGE}


@pytest.fixture
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _matcher(ctx, prm):
    return L.ScanToMapMatcher(ctx, L.make_params(prm["variant"], **C.device_overrides(prm)))


def _records(m, slot, kind, n_q):
    """the compacted records of a slot as the model wants them"""
    if kind == "s":
        g = m.surf_records(slot, n_q)
        return dict(cp=g["cp"], n=g["n"], d=g["d"], score=g["score"], query_index=g["query_index"], count=g["count"])
    g = m.edge_records(slot, n_q)
    return dict(cp=g["cp"], a=g["a"], b=g["b"], s=g["s"], query_index=g["query_index"], count=g["count"])


def _excess(G, Gm, allow):
    G, Gm = np.asarray(G, np.float64), np.asarray(Gm, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(G - Gm) / allow
    e = np.where(np.isnan(G) & np.isnan(Gm), 0.0, np.where((G == Gm) & np.isfinite(G), 0.0, e))
    return float(np.where(np.isnan(e), np.inf, e).max())


def _oracle_row(O, row, rec):
    one = {k: np.ascontiguousarray(np.asarray(v)[None]) for k, v in rec.items()}
    one["valid"] = np.ones(1, np.uint8)
    PO = O.params(row["prm"]["variant"], **C.oracle_overrides(row["prm"]))
    f = O.linearize_surf if row["kind"] == "s" else O.linearize_edge
    return f(one, row["t"], row["q"], PO, C.oracle_scale(row["prm"], row["kind"], row["N"]))


def _dev_gram(m, slot, mask, row, counts_dev, gram_dev):
    """one row through counts_import + linearize_dev at the device pose: (G, cost, (n_surf, n_edge))"""
    import torch
    counts_dev.fill_(int(row["N"]))
    m.pose_set(slot, row["t"], row["q"])
    m.counts_import(slot, counts_dev.data_ptr())
    m.linearize_dev(slot, gram_dev.data_ptr(), mask)
    m.ctx.sync()
    torch.cuda.synchronize()
    g = gram_dev.cpu().numpy()
    return g[:64].reshape(8, 8).copy(), float(g[64]), (int(g[65]), int(g[66]))


@pytest.mark.parametrize("variant,offset", GRID)
def test_probe_rows_one_record_at_a_time(ctx, oracle, variant, offset):
    import torch
    s = C.scene(variant, offset)
    si, ei = C.probe_queries(variant, offset)
    kinds = ("s",) if variant == "frontend" else ("s", "e")
    m = _matcher(ctx, C.params(variant))
    m.set_input_cloud(L.KIND_SURF, s["surf_map"])
    if "e" in kinds:
        m.set_input_cloud(L.KIND_EDGE, s["edge_map"])
    recs = {}
    for kind, idx, src in (("s", si, "surf_q"), ("e", ei, "edge_q")):
        if kind not in kinds:
            continue
        got = []
        for k, i in enumerate(idx):
            inv = s["invalid"][:s[src].shape[1]]
            m.set_queries(k, KIND[kind], np.ascontiguousarray(np.stack([inv, s[src][i], inv])))
            n = (m.find_corresponding_surf_features if kind == "s" else m.find_corresponding_corner_features)(k, C.Q_ASSOC, C.T_ASSOC)
            r = _records(m, k, kind, 3)
            assert n == 1 and r["count"] == 1 and list(r["query_index"]) == [1]                # the probe is the slot's only valid record
            got.append(r)
        recs[kind] = {f: np.concatenate([g[f] for g in got]) for f in got[0] if f not in ("count", "query_index")}
    rows = C.probe_rows(variant, offset, recs["s"], recs.get("e"))
    counts_dev = torch.zeros(2, dtype=torch.int32, device="cuda")
    gram_dev = torch.zeros(72, dtype=torch.float64, device="cuda")                  # LILI_GRAM_DOUBLES: 64 Gram, cost, n_surf, n_edge
    # batches: rows of one kind and parameter set whose records sit in different slots go into one linearize_window call
    groups = {}
    for r in rows:
        groups.setdefault((r["kind"], tuple(sorted(C.device_overrides(r["prm"]).items())), r["N"]), []).append(r)
    worst_m, worst_o, n_rows = {}, {}, 0
    for (kind, _, N), grp in groups.items():
        mm = _matcher(ctx, grp[0]["prm"])
        pending = list(grp)
        while pending:
            batch, rest, seen = [], [], set()
            for r in pending:
                (rest if r["i"] in seen else batch).append(r)
                seen.add(r["i"])
            pending = rest
            if N == 1:
                out = mm.linearize_window([r["i"] for r in batch], [r["t"] for r in batch], [r["q"] for r in batch], MASK[kind])
            else:
                out = [_dev_gram(mm, r["i"], MASK[kind], r, counts_dev, gram_dev) for r in batch]
            for r, (G, cost, counts) in zip(batch, out):
                md = C.probe_model(r, recs["s"], recs.get("e"))
                if r["prm"]["loss"] == C.LOSS_HUBER:
                    assert abs(md["raw"] - r["prm"]["loss_a"]) > 1e-9 * r["prm"]["loss_a"]
                Gm, allow, acost = C.gram_of_row(md, C.DEVICE_FACTOR)
                tag = (variant, offset, r["fam"], kind, r["i"], N, md["raw"])
                assert tuple(counts) == ((1, 0) if kind == "s" else (0, 1)), tag
                assert np.array_equal(G, G.T), tag
                e = max(_excess(G, Gm, allow), abs(cost - md["cost"]) / (acost + C.EPS * abs(md["cost"])))
                worst_m[r["fam"]] = max(worst_m.get(r["fam"], 0.0), e)
                assert e <= 1.0, tag + (e,)
                Go, co, no = _oracle_row(oracle, r, C._one(recs[kind], r["i"]))
                _, allow_o, acost_o = C.gram_of_row(md, 1.0 + C.DEVICE_FACTOR)
                eo = max(_excess(G, Go, allow_o + C.EPS * np.abs(Go)), abs(cost - co) / (acost_o + 2 * C.EPS * abs(co)))
                worst_o[r["fam"]] = max(worst_o.get(r["fam"], 0.0), eo)
                assert no == 1 and eo <= 1.0, tag + (eo,)
                n_rows += 1
    print(f"\n{variant} {offset}: {n_rows} probe rows; worst error / (8 x allowance) against the model { {k: round(v, 3) for k, v in worst_m.items()} }; "
          f"against the oracle / (9 x) { {k: round(v, 3) for k, v in worst_o.items()} }")
    assert n_rows == len(rows)


# ------------------------------------------------------------------------------------------------
# 2. partition
# ------------------------------------------------------------------------------------------------
def _partition_cases():
    """every size under every validity pattern that exists there, on every variant; the edge sizes likewise on the two variants with edge factors"""
    out = [(v, "s", n, pat) for v in C.VARIANTS for n in C.SIZES for pat in C.PATTERNS if C.partition_applies(n, pat)]
    out += [(v, "e", n, pat) for v in ("livox", "rot") for n in C.EDGE_SIZES for pat in C.PATTERNS if C.partition_applies(n, pat) and pat != "second_trip_only"]
    out += [(v, "e", 262145, "second_trip_only") for v in ("livox", "rot")]
    return out


def _set_and_associate(m, slot, variant, offset, kind, n, pattern):
    q, valid = C.partition_queries(variant, offset, kind, n, pattern)
    m.set_queries(slot, KIND[kind], q)
    cnt = (m.find_corresponding_surf_features if kind == "s" else m.find_corresponding_corner_features)(slot, C.Q_ASSOC, C.T_ASSOC)
    rec = _records(m, slot, kind, n)
    assert cnt == rec["count"] == int(valid.sum()) and np.array_equal(rec["query_index"], np.nonzero(valid)[0])          # the intended valid records, no others
    return rec, cnt


def _check_bulk(G, cost, parts, n_q, tag):
    """parts: [(kind, prm, rec, N, t, q, n_q of the kind)] — the device Gram against the sum of the kinds' longdouble models, per entry"""
    Gm, cm, allow, acost = np.zeros((8, 8), C.LD), C.LD(0), np.zeros((8, 8)), 0.0
    for kind, prm, rec, N, t, q, nk in parts:
        g, c, a, ac = C.gram_model(kind, prm, rec, N, t, q, nk, C.DEVICE_FACTOR)
        Gm, cm, allow, acost = Gm + g, cm + c, allow + a, acost + ac
    e = _excess(G, Gm, allow + C.EPS * np.abs(Gm).astype(np.float64)) if np.abs(Gm).max() > 0 else float(np.abs(G).max())
    ec = abs(cost - float(cm)) / (acost + 2 * C.EPS * abs(float(cm))) if float(cm) != 0 else abs(cost)
    assert np.array_equal(G, G.T), tag
    assert e <= 1.0 and ec <= 1.0, tag + (e, ec)
    return max(e, ec)


@pytest.mark.skipif(not C.BULK_OK, reason=C.BULK_SKIP)
@pytest.mark.parametrize("variant,kind,n,pattern", _partition_cases())
def test_partition_whole_gram_per_entry(ctx, variant, kind, n, pattern):
    offset = "far"
    s = C.scene(variant, offset)
    prm = C.params(variant)
    m = _matcher(ctx, prm)
    m.set_input_cloud(KIND[kind], s["surf_map"] if kind == "s" else s["edge_map"])
    rec, cnt = _set_and_associate(m, 0, variant, offset, kind, n, pattern)
    t, q = C.partition_pose(variant, kind)
    G, cost, counts = m.linearize(0, t, q, MASK[kind])
    G2, cost2, counts2 = m.linearize(0, t, q, MASK[kind])
    assert np.array_equal(G.view(np.uint64), G2.view(np.uint64)) and cost == cost2 and tuple(counts) == tuple(counts2)            # identical bytes
    assert tuple(counts) == ((cnt, 0) if kind == "s" else (0, cnt))
    e = _check_bulk(G, cost, [(kind, prm, rec, cnt, t, q, n)], n, (variant, kind, n, pattern))
    print(f"\n{variant} {kind} n {n} {pattern}: {cnt} records, worst error / allowance per entry {e:.3f}")


@pytest.mark.skipif(not C.BULK_OK, reason=C.BULK_SKIP)
@pytest.mark.parametrize("n", [1025, 262145])
def test_partition_rot_with_an_imported_global_count(ctx, n):
    """counts_export gives the slot's own counts; after counts_import of another global count the weights are score * 1000 / N_global"""
    import torch
    s = C.scene("rot", "far")
    prm = C.params("rot")
    m = _matcher(ctx, prm)
    m.set_input_cloud(L.KIND_SURF, s["surf_map"]); m.set_input_cloud(L.KIND_EDGE, s["edge_map"])
    rs, ns = _set_and_associate(m, 0, "rot", "far", "s", n, "every_other")
    re_, ne = _set_and_associate(m, 0, "rot", "far", "e", 1025, "all")
    counts_dev = torch.zeros(2, dtype=torch.int32, device="cuda")
    gram_dev = torch.zeros(72, dtype=torch.float64, device="cuda")
    m.counts_export(0, counts_dev.data_ptr())
    m.ctx.sync(); torch.cuda.synchronize()
    assert counts_dev.cpu().tolist() == [ns, ne]
    t, q = C.partition_pose("rot", "s")
    mask = L.MASK_SURF | L.MASK_EDGE
    for Ns, Ne in ((ns, ne), (3 * ns + 7, 2 * ne + 1)):
        counts_dev.copy_(torch.tensor([Ns, Ne], dtype=torch.int32))
        m.pose_set(0, t, q)
        m.counts_import(0, counts_dev.data_ptr())
        m.linearize_dev(0, gram_dev.data_ptr(), mask)
        m.ctx.sync(); torch.cuda.synchronize()
        g = gram_dev.cpu().numpy()
        assert (int(g[65]), int(g[66])) == (ns, ne)
        e = _check_bulk(g[:64].reshape(8, 8).copy(), float(g[64]), [("s", prm, rs, Ns, t, q, n), ("e", prm, re_, Ne, t, q, 1025)], n, ("rot", n, Ns, Ne))
        print(f"\nrot both kinds n {n}, counts ({Ns}, {Ne}): worst error / allowance per entry {e:.3f}")


@pytest.mark.skipif(not C.BULK_OK, reason=C.BULK_SKIP)
@pytest.mark.parametrize("variant", ["livox", "rot"])
@pytest.mark.parametrize("case", ["both", "edge_empty", "surf_empty", "edge_none_valid", "surf_none_valid", "big_surf"])
def test_partition_both_kinds(ctx, variant, case):
    """surf + edge in one launch; one kind with n_q == 0 after an association; one kind without a valid record"""
    s = C.scene(variant, "far")
    prm = C.params(variant)
    m = _matcher(ctx, prm)
    m.set_input_cloud(L.KIND_SURF, s["surf_map"]); m.set_input_cloud(L.KIND_EDGE, s["edge_map"])
    ns_q, ne_q = (262145 if case == "big_surf" else 0 if case == "surf_empty" else 1025), (0 if case == "edge_empty" else 1025)
    parts, want = [], []
    t, q = C.partition_pose(variant, "s")
    for kind, nq, none in (("s", ns_q, case == "surf_none_valid"), ("e", ne_q, case == "edge_none_valid")):
        if nq == 0:
            m.set_queries(0, KIND[kind], np.zeros((0, s["surf_q"].shape[1] if kind == "s" else 3), np.float32))
            assert (m.find_corresponding_surf_features if kind == "s" else m.find_corresponding_corner_features)(0, C.Q_ASSOC, C.T_ASSOC) == 0
            want.append(0)
        elif none:
            src = s["surf_q"] if kind == "s" else s["edge_q"]
            m.set_queries(0, KIND[kind], np.ascontiguousarray(np.tile(s["invalid"][:src.shape[1]], (nq, 1))))
            assert (m.find_corresponding_surf_features if kind == "s" else m.find_corresponding_corner_features)(0, C.Q_ASSOC, C.T_ASSOC) == 0
            want.append(0)
        else:
            rec, cnt = _set_and_associate(m, 0, variant, "far", kind, nq, "every_other" if kind == "s" else "all")
            parts.append((kind, prm, rec, cnt, t, q, nq)); want.append(cnt)
    G, cost, counts = m.linearize(0, t, q, L.MASK_SURF | L.MASK_EDGE)
    G2, cost2, _ = m.linearize(0, t, q, L.MASK_SURF | L.MASK_EDGE)
    assert np.array_equal(G.view(np.uint64), G2.view(np.uint64)) and cost == cost2 and list(counts) == want
    e = _check_bulk(G, cost, parts, max(ns_q, ne_q), (variant, case))
    print(f"\n{variant} {case}: counts {want}, worst error / allowance per entry {e:.3f}")


# ------------------------------------------------------------------------------------------------
# 3. launch structures that must not change a bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["rot", "livox"])
@pytest.mark.parametrize("case", ["1025", "second_trip", "both"])
def test_launch_structures_are_bit_identical(ctx, variant, case):
    import torch
    s = C.scene(variant, "far")
    prm = C.params(variant)
    m = _matcher(ctx, prm)
    m.set_input_cloud(L.KIND_SURF, s["surf_map"]); m.set_input_cloud(L.KIND_EDGE, s["edge_map"])
    mask = L.MASK_SURF | L.MASK_EDGE if case == "both" else L.MASK_SURF
    ns_q, pat = (262145, "second_trip_only") if case == "second_trip" else (1025, "all")
    t, q = C.partition_pose(variant, "s")
    others = [(2, 300, "every_other"), (5, 65, "all")]                              # two further slots for the window calls
    for slot, n, p in [(0, ns_q, pat)] + others:
        _set_and_associate(m, slot, variant, "far", "s", n, p)
        if mask & L.MASK_EDGE:
            _set_and_associate(m, slot, variant, "far", "e", 1025 if slot == 0 else 63, "all")
    ref = m.linearize(0, t, q, mask)
    assert ref[2][0] > 0

    def same(got, name):
        assert np.array_equal(np.asarray(got[0]).view(np.uint64), ref[0].view(np.uint64)) and got[1] == ref[1] and tuple(got[2]) == tuple(ref[2]), (variant, case, name)
    gram_dev, gram_acc = torch.zeros(72, dtype=torch.float64, device="cuda"), torch.zeros(72, dtype=torch.float64, device="cuda")
    t2, q2 = t + 0.01, C.qmul(C.qaxis(0.01, (1.0, 2.0, 3.0)), q)
    try:
        for ft in (0, 1):
            ctx.set_option("fuse_tail", ft)
            for mk in (1, 0):
                ctx.set_option("merge_kinds", mk)
                same(m.linearize(0, t, q, mask), f"fuse_tail {ft} merge_kinds {mk}")
            ctx.set_option("merge_kinds", 1)
            for order in ([0, 2, 5], [2, 0, 5], [2, 5, 0]):
                out = m.linearize_window(order, [t if k == 0 else t2 for k in order], [q if k == 0 else q2 for k in order], mask)
                same(out[order.index(0)], f"fuse_tail {ft} window {order}")
            m.pose_set(0, t, q)
            m.linearize_dev(0, gram_dev.data_ptr(), mask)
            m.ctx.sync(); torch.cuda.synchronize()
            g = gram_dev.cpu().numpy()
            same((g[:64].reshape(8, 8).copy(), float(g[64]), (int(g[65]), int(g[66]))), f"fuse_tail {ft} linearize_dev")
            # accumulate re-associates at the device pose, so its records are not the ones above: it is held to the two calls it stands for, from the same pose
            m.pose_set(0, t, q)
            m.associate_dev(0, mask)
            m.linearize_dev(0, gram_dev.data_ptr(), mask)
            m.pose_set(0, t, q)
            m.accumulate(0, gram_acc.data_ptr(), mask)
            m.ctx.sync(); torch.cuda.synchronize()
            a, b = gram_dev.cpu().numpy(), gram_acc.cpu().numpy()
            assert a[65] > 0 and (not mask & L.MASK_EDGE or a[66] > 0), (variant, case, a[65:67])
            assert np.array_equal(a[:67].view(np.uint64), b[:67].view(np.uint64)), (variant, case, f"fuse_tail {ft} accumulate")
            _set_and_associate(m, 0, variant, "far", "s", ns_q, pat)             # the records of the reference again
            if mask & L.MASK_EDGE:
                _set_and_associate(m, 0, variant, "far", "e", 1025, "all")
    finally:
        ctx.set_option("fuse_tail", 0); ctx.set_option("merge_kinds", 1)                # the defaults


# ------------------------------------------------------------------------------------------------
# 4. launches that linearise inside the association: only the Gauss-Newton step is observable
# ------------------------------------------------------------------------------------------------
ON_THE_FLY = [("fuse_lin_block", 0), ("fuse_lin_block", 64), ("fuse_lin_block", 256), ("assoc_lpq", 2), ("assoc_lpq", 4), ("assoc_lpq", 8), ("assoc_lpq", 16)]


def _fused(variant, opt, val, n_s, n_e):
    """does this launch structure linearise inside the association?  The flavours without count scaling: always (below 1600 association waves).  rot: only the
    cooperative launch, through its in-launch count barrier (option count_barrier), and only while its grid has at most 256 workgroups of 256 / L queries
    (launch_associate_coop) — the one-lane launch and the larger grids take the staged launches"""
    if variant != "rot":
        return True
    return opt == "assoc_lpq" and -(-n_s // (256 // val)) + -(-n_e // (256 // val)) <= 256


def _one_iteration(ctx, prm, s, variant, offset, n, mask, kinds, t0, q0):
    m = _matcher(ctx, prm)
    m.set_input_cloud(L.KIND_SURF, s["surf_map"])
    m.set_queries(0, L.KIND_SURF, C.partition_queries(variant, offset, "s", n, "every_other" if n == 1025 else "all")[0])
    if "e" in kinds:
        m.set_input_cloud(L.KIND_EDGE, s["edge_map"])
        m.set_queries(0, L.KIND_EDGE, C.partition_queries(variant, offset, "e", 1025, "all")[0])
    m.pose_set(0, t0, q0)
    m.iterate(0, 1, mask)
    d, n_upd, st = m.last_step(0)
    assert n_upd == 1 and st == 0, (variant, n, st)
    return m, d


@pytest.mark.skipif(not C.BULK_OK, reason=C.BULK_SKIP)
@pytest.mark.parametrize("n", [1025, 9000])
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_on_the_fly_linearisation_gives_the_models_step(ctx, variant, n):
    """fuse_lin with fuse_lin_block 0 / 64 / 256 on the one-lane association (k_associate_lin) and the cooperative association with 2 / 4 / 8 / 16 lanes per query
    (k_associate_coop<L, true>; rot with option count_barrier = 1, through the in-launch count barrier): pose_set, iterate(slot, 1), last_step.  Which rot legs are
    NOT eligible and take the staged launches is in _fused(): the three fuse_lin_block legs, and 8 / 16 lanes at 9000 + 1025 queries (315 / 628 workgroups).
    Held (a) as the issue sets it, to the step solved in longdouble from the model's Gram of the records that launch left behind (read through the staged
    linearize at the start pose) within cond(H) (|dH| / |H| + |dg| / |g|) |delta|; (b) to the same step within the componentwise first-order bound
    (gn_step_model), which is orders tighter; (c) to the step of the STAGED launches (fuse_lin 0, one lane, no count barrier: k_linearize + k_reduce_partials) from
    the same start pose, which computes the same rows and differs in the partition of the sum alone: within the componentwise bound of the two summation trees,
    no evaluation allowance at all — and bit for bit where the leg is not eligible.  A fused launch cannot be observed directly; that at least one eligible leg
    differs from the staged step in some bit is asserted, a silent fall-back of all of them would be bit-identical.
    `origin`: at `far` the translation and the rotation about an origin 700 m away are nearly the same motion and cond(H) is past the 1e6 the bound is good for;
    so `cancel` rows are not in this mix.  The residuals are what partition_pose gives (0 .. 0.15 m unweighted); for the front-end, that both sides of the Huber
    threshold are populated is asserted on the model."""
    offset = "origin"
    s = C.scene(variant, offset)
    prm = C.params(variant)
    kinds = ("s",) if variant == "frontend" else ("s", "e")
    mask = L.MASK_SURF if variant == "frontend" else L.MASK_SURF | L.MASK_EDGE
    t0, q0 = C.partition_pose(variant, "s")
    worst = worst_abs = worst_cw = worst_st = 0.0
    differs = eligible = 0
    try:
        ctx.set_option("fuse_lin", 0); ctx.set_option("assoc_lpq", 1); ctx.set_option("count_barrier", 0)
        _, d_staged = _one_iteration(ctx, prm, s, variant, offset, n, mask, kinds, t0, q0)
        ctx.set_option("fuse_lin", 1)
        for opt, val in ON_THE_FLY:
            ctx.set_option("assoc_lpq", val if opt == "assoc_lpq" else 1)
            ctx.set_option("fuse_lin_block", val if opt == "fuse_lin_block" else 0)
            ctx.set_option("count_barrier", 1 if variant == "rot" and opt == "assoc_lpq" else 0)
            m, d = _one_iteration(ctx, prm, s, variant, offset, n, mask, kinds, t0, q0)
            G, cost, counts = m.linearize(0, t0, q0, mask)                          # the records of that association, staged, at the start pose
            Gm, allow, asum = np.zeros((8, 8), C.LD), np.zeros((8, 8)), np.zeros((8, 8))
            for kind, cnt, nq in zip(kinds, counts, (n, 1025)):
                rec = _records(m, 0, kind, nq)
                assert rec["count"] == cnt and cnt > (400 if kind == "s" else 100)
                depth = 64 + -(-nq // 16) + 24                                      # at most one partial per 16 queries (16 lanes each)
                g, _, a, _ = C.gram_model(kind, prm, rec, cnt, t0, q0, nq, C.DEVICE_FACTOR, depth=depth)
                Gm, allow = Gm + g, allow + a
                asum += C.gram_model(kind, prm, rec, cnt, t0, q0, nq, 0.0, depth=depth)[2] + C.gram_model(kind, prm, rec, cnt, t0, q0, nq, 0.0)[2]   # the two trees, no rows
                if variant == "frontend":                                           # Huber: |r'| < a are inliers, |r'| = sqrt(a |r|) > a outliers
                    X, _, _, _ = C.rows(kind, prm, rec, np.ones(cnt), t0, q0)
                    ar = np.abs(np.asarray(X[:, 7], np.float64))
                    assert (ar < prm["loss_a"]).sum() > 0.1 * cnt and (ar > prm["loss_a"]).sum() > 0.1 * cnt, ((ar < prm["loss_a"]).sum(), cnt)
            delta, cond, bound, cw = C.gn_step_model(Gm, allow, q0)
            assert cond < 1e6, (variant, n, cond)
            e = float(np.linalg.norm(d - delta) / bound)
            ecw = float((np.abs(d - delta) / (cw + C.EPS * np.abs(delta))).max())
            worst, worst_abs, worst_cw = max(worst, e), max(worst_abs, float(np.linalg.norm(d - delta))), max(worst_cw, ecw)
            assert e <= 1.0 and ecw <= 1.0 and np.linalg.norm(delta) > 1e-3, (variant, n, opt, val, e, ecw, d, delta)
            if _fused(variant, opt, val, n, 1025):
                eligible += 1
                differs += int(not np.array_equal(d.view(np.uint64), d_staged.view(np.uint64)))
                cws = C.gn_step_model(Gm, asum, q0)[3]
                est = float((np.abs(d - d_staged) / cws).max())
                worst_st = max(worst_st, est)
                assert est <= 1.0, (variant, n, opt, val, est, d, d_staged)
            else:
                assert np.array_equal(d.view(np.uint64), d_staged.view(np.uint64)), (variant, n, opt, val)
        assert differs >= 1, (variant, n, eligible)
    finally:
        for opt, val in (("assoc_lpq", 0), ("fuse_lin_block", 0), ("count_barrier", 0), ("fuse_lin", 1)):
            ctx.set_option(opt, val)
    print(f"\n{variant} n {n}: |step| {np.linalg.norm(delta):.3g}, cond(H) {cond:.3g}; against the model: worst |step error| {worst_abs:.2e} = {worst:.2e} of the norm bound "
          f"{bound:.2e}, {worst_cw:.1e} of the componentwise bound; against the staged step: {worst_st:.1e} of the two trees' componentwise bound; "
          f"{differs} of {eligible} eligible launch structures differ from the staged step in some bit, {len(ON_THE_FLY) - eligible} not eligible are bit-identical")


# ------------------------------------------------------------------------------------------------
# 5. r == 0 and nu == 0
# ------------------------------------------------------------------------------------------------
def test_zero_residual_row_is_exact(ctx, oracle):
    """the sq == 0 arm of the corrector: f32-exact plane, the query in it, the identity pose — every entry is exact, so equality"""
    mp_, q = C.exact_clouds("frontend", "surf")
    for prm in (C.params("frontend"), C.params("frontend", loss=C.LOSS_NONE), C.params("frontend", loss=C.LOSS_CAUCHY, loss_a=1.0)):
        m = _matcher(ctx, prm)
        m.set_input_cloud(L.KIND_SURF, mp_)
        m.set_queries(0, L.KIND_SURF, q)
        assert m.find_corresponding_surf_features(0, C.IDENTITY[1], C.IDENTITY[0]) == 1
        rec = _records(m, 0, "s", 3)
        assert list(rec["query_index"]) == [1]
        X, cost, raw = C.row_mp("s", prm, C._one(rec, 0), 1.0, *C.IDENTITY)
        assert raw == 0.0 and X[7] == 0.0 and cost == 0.0                          # the residual really is 0, on the device's own record
        G, c, counts = m.linearize(0, *C.IDENTITY, L.MASK_SURF)
        assert tuple(counts) == (1, 0) and c == 0.0 and np.array_equal(G, np.outer(X, X)) and np.isfinite(G).all(), (prm["loss"], G, X)


@pytest.mark.parametrize("variant", ["livox", "rot"])
def test_onepoint_edge_row_is_nan_like_the_oracle_and_the_step_is_refused(ctx, oracle, variant):
    prm = C.params(variant)
    m = _matcher(ctx, prm)
    mp_, q = C.exact_clouds(variant, "edge")
    m.set_input_cloud(L.KIND_EDGE, mp_)
    m.set_queries(0, L.KIND_EDGE, q)
    assert m.find_corresponding_corner_features(0, C.IDENTITY[1], C.IDENTITY[0]) == 1
    rec = _records(m, 0, "e", 3)
    w = float(C.weight(prm, "e", rec["s"][:1], 1)[0])
    X, _, raw = C.row_mp("e", prm, C._one(rec, 0), w, *C.IDENTITY)
    assert raw == 0.0 and np.isnan(X[:7]).all()                                     # the point IS on the line of the device's record
    G, cost, counts = m.linearize(0, *C.IDENTITY, L.MASK_EDGE)
    one = {k: np.ascontiguousarray(np.asarray(v)[:1]) for k, v in rec.items() if k in ("cp", "a", "b", "s")}
    one["valid"] = np.ones(1, np.uint8)
    Go, co, no = oracle.linearize_edge(one, *C.IDENTITY, oracle.params(variant), C.oracle_scale(prm, "e", 1))
    assert tuple(counts) == (0, 1) and no == 1
    assert np.array_equal(np.isfinite(G), np.isfinite(Go)) and np.array_equal(np.isnan(G), np.isnan(Go)), (G, Go)           # the non-finite entries are the oracle's
    assert np.array_equal(G[np.isfinite(G)], Go[np.isfinite(Go)])
    # a Gauss-Newton step on that Gram is refused and leaves the pose bits alone.  iterate() associates at Q q_lb^-1 and linearises the edge at Q: with the
    # identity extrinsic handed over, both are the identity and the record, hence nu == 0, is the one above
    mi = L.ScanToMapMatcher(ctx, L.make_params(variant, q_lb=(1.0, 0.0, 0.0, 0.0), t_lb=(0.0, 0.0, 0.0)))
    mi.pose_set(0, *C.IDENTITY)
    before = np.concatenate(mi.pose_get(0)[:2]).view(np.uint64).copy()
    mi.iterate(0, 1, L.MASK_EDGE)
    tn, qn, st = mi.pose_get(0)
    assert st != 0 and mi.last_step(0)[2] != 0
    assert np.array_equal(np.concatenate([tn, qn]).view(np.uint64), before)
    # a healthy registration in the same context afterwards
    s = C.scene(variant, "origin")
    m.set_input_cloud(L.KIND_SURF, s["surf_map"])
    rec2, cnt = _set_and_associate(m, 1, variant, "origin", "s", 1025, "all")
    t, qq = C.partition_pose(variant, "s")
    G2, cost2, counts2 = m.linearize(1, t, qq, L.MASK_SURF)
    assert counts2[0] == 1025 and np.isfinite(G2).all() and np.isfinite(cost2)
    if C.BULK_OK:
        _check_bulk(G2, cost2, [("s", prm, rec2, cnt, t, qq, 1025)], 1025, (variant, "after onepoint"))
    m.pose_set(1, t, qq)
    m.iterate(1, 3, L.MASK_SURF)
    t3, q3, st3 = m.pose_get(1)
    d3, n3, _ = m.last_step(1)
    assert st3 == 0 and n3 == 3 and np.abs(t3 - t).max() > 1e-3 and np.isfinite(np.r_[t3, q3]).all()                     # the step path works again, and the pose moved
