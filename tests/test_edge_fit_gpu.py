"""The line fit of the association kernels (edge_fit, lili_s2m_dev.h) on hard neighbourhoods, through every launcher that calls it, against the oracle
— which solves the 3 x 3 eigen-problem by Householder tridiagonalisation and implicit QR where the device runs cyclic Jacobi sweeps — and against the
numpy model of tests/edge_fit_cases.py (cases, kinds and the margin rule are described there; tests/test_edge_fit_cases_cpu.py holds the oracle to the model).

Launchers: the one-lane kernel (assoc_lpq 1, lili_s2m.hip), the cooperative kernel with 2 / 4 / 8 / 16 lanes per query and the default choice (assoc_lpq 0,
lili_s2m_coop.hip), each with the super-row layout on and off; associate_window over two slots (k_associate_coop_window); the dense-map launch
(k_associate_fine, lili_s2m_dense.hip) — the clusters laid into a filler cloud that lifts the occupancy over the fine index's threshold and stays outside
every gate, map_density says that the fine index was built.

What must hold, per launcher: neighbour indices and d^2 are the oracle's; the valid queries are the oracle's (and the model's) on every decided cluster; A and
B are within one f32 ulp per component of the oracle's and of the model's on decided clusters (tied ones as an unordered pair); s is lidar_const; the records
of all launchers are bit-identical, tied and undecided clusters included — they call the same function on the same neighbours."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import edge_fit_cases as E

pytestmark = pytest.mark.gpu

SINGLE = [(lpq, sr) for sr in (1, 0) for lpq in (1, 2, 4, 8, 16, 0)]
GRID = [(c, o, v) for c in E.CASES for o in E.OFFSETS for v in E.VARIANTS]


def _take(m, slot, n):
    idx, d2 = m.neighbors(slot, L.KIND_EDGE, n)
    return dict(idx=idx, d2=d2, rec=m.edge_records(slot, n))


def _single(ctx, P, map_xyz, q_local, lpq, super_rows):
    ctx.set_option("assoc_lpq", lpq)
    ctx.set_option("super_rows", super_rows)
    m = L.ScanToMapMatcher(ctx, P)
    m.map_focus(None)
    m.set_input_cloud(L.KIND_EDGE, map_xyz)
    m.set_queries(0, L.KIND_EDGE, q_local)
    n = m.find_corresponding_corner_features(0, E.Q_ASSOC, E.T_ASSOC)
    out = _take(m, 0, q_local.shape[0])
    assert out["rec"]["count"] == n
    return out, m


def _window(ctx, P, map_xyz, q_local, lpq):
    ctx.set_option("assoc_lpq", lpq)
    ctx.set_option("super_rows", 1)
    m = L.ScanToMapMatcher(ctx, P)
    m.map_focus(None)
    m.set_input_cloud(L.KIND_EDGE, map_xyz)
    for slot in (0, 1):
        m.set_queries(slot, L.KIND_EDGE, q_local)
    counts = m.associate_window([0, 1], [E.T_ASSOC] * 2, [E.Q_ASSOC] * 2, L.MASK_EDGE)
    outs = [_take(m, slot, q_local.shape[0]) for slot in (0, 1)]
    assert [c[1] for c in counts] == [o["rec"]["count"] for o in outs] and all(c[0] == 0 for c in counts)
    return outs


def _dense(P, map_xyz, filler, q_local):
    """one build of clusters + filler in a fresh context (no hint of an earlier map): the fine index, hence k_associate_fine"""
    ctx = L.Context(0)
    try:
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, P)
        m.set_input_cloud(L.KIND_EDGE, np.ascontiguousarray(np.r_[map_xyz, filler]))
        occ, fcell, fr2 = m.map_density(L.KIND_EDGE)
        assert occ > 12 and fcell > 0 and fr2 > 0, (occ, fcell, fr2)             # the dense launch is the one taken (launch_associate: dense = has_fine)
        m.set_queries(0, L.KIND_EDGE, q_local)
        n = m.find_corresponding_corner_features(0, E.Q_ASSOC, E.T_ASSOC)
        out = _take(m, 0, q_local.shape[0])
        assert out["rec"]["count"] == n
        return out
    finally:
        ctx.close()


def _restore(ctx, P):
    ctx.set_option("assoc_lpq", 0)
    ctx.set_option("super_rows", 1)
    ctx.set_debug(False)
    L.ScanToMapMatcher(ctx, P).map_focus(None)


def _all_launchers(ctx, P, s, filler):
    """[(name, result)] — the first entry is the one-lane kernel"""
    got = []
    ctx.set_debug(True)
    for lpq, sr in SINGLE:
        got.append((f"lpq {lpq} super_rows {sr}", _single(ctx, P, s["map_xyz"], s["q_local"], lpq, sr)[0]))
    for lpq in (0, 4):
        for slot, out in enumerate(_window(ctx, P, s["map_xyz"], s["q_local"], lpq)):
            got.append((f"window lpq {lpq} slot {slot}", out))
    got.append(("dense", _dense(P, s["map_xyz"], filler, s["q_local"])))
    return got


def _full(rec, n):
    """the compacted record list spread over the queries"""
    valid = np.zeros(n, bool); a = np.zeros((n, 3), np.float32); b = np.zeros((n, 3), np.float32)
    qi = rec["query_index"]
    valid[qi] = True; a[qi] = rec["a"]; b[qi] = rec["b"]
    return valid, a, b


@pytest.mark.parametrize("case,offset,variant", GRID)
def test_edge_fit_on_hard_neighbourhoods_through_every_launcher(gpu_ctx, oracle, case, offset, variant):
    s, rec, mdl = E.reference(case, offset, variant)
    n, kind = s["n"], s["kind"]
    P = L.make_params(variant)
    try:
        got = _all_launchers(gpu_ctx, P, s, E.dense_filler(case, offset))
    finally:
        _restore(gpu_ctx, P)
    dec, tied = mdl["decided"], mdl["tied"]
    inside = rec["nn_d2"][:, 4] < E.EDGE_GATE
    o_valid = rec["valid"].astype(bool)
    first = got[0][1]
    for name, g in got:
        # neighbours
        assert np.array_equal(g["idx"][inside], rec["nn_idx"][inside]), name
        assert np.array_equal(g["d2"][inside].view(np.uint32), rec["nn_d2"][inside].view(np.uint32)), name
        assert not (g["d2"][~inside][:, 4] < E.EDGE_GATE).any(), name
        # the records of every launcher are those of the one-lane kernel, bit for bit
        assert g["rec"]["count"] == first["rec"]["count"], name
        for k in ("query_index", "cp", "a", "b", "s"):
            assert np.array_equal(g["rec"][k].view(np.uint32), first["rec"][k].view(np.uint32)), (name, k)
    g_valid, ga, gb = _full(first["rec"], n)
    diff = np.nonzero(g_valid != o_valid)[0]
    both = dec & g_valid & o_valid
    not_bit_equal = int((ga[both].view(np.uint32) != rec["a"][both].view(np.uint32)).sum() + (gb[both].view(np.uint32) != rec["b"][both].view(np.uint32)).sum())
    flipped = int((both & tied & (ga != rec["a"]).any(1) & (ga == rec["b"]).all(1)).sum())
    print(f"\n{case} {offset} {variant}: {E.summary(case, offset, variant)} device valid {int(g_valid.sum())}, differs from the oracle on {diff.size} undecided "
          f"{sorted(set(kind[diff].tolist()))}; A/B components not bit-equal to the oracle {not_bit_equal} of {6 * int(both.sum())}, tied pairs the other way round {flipped}")
    # valid flags
    assert np.array_equal(g_valid[dec], o_valid[dec]), (kind[dec & (g_valid != o_valid)][:10], np.nonzero(dec & (g_valid != o_valid))[0][:10])
    assert np.array_equal(g_valid[dec], mdl["valid"][dec])
    assert not g_valid[kind == "exact3"].any()                                     # ratio exactly 3: the gate is strict
    # A and B
    close_o = E.pair_close(ga, gb, rec["a"], rec["b"], tied)
    assert close_o[both].all(), (kind[both & ~close_o][:10], np.nonzero(both & ~close_o)[0][:10])
    close_m = E.pair_close(ga, gb, mdl["A"], mdl["B"], tied)
    assert close_m[both].all(), (kind[both & ~close_m][:10], np.nonzero(both & ~close_m)[0][:10])
    # s and the query itself
    r = first["rec"]
    assert (r["s"] == np.float32(P.lidar_const)).all() and np.array_equal(r["cp"], s["q_local"][r["query_index"]])


def test_edge_fit_short_map_refuses_every_query(gpu_ctx):
    """four map points: fewer than five neighbours (the reference reads past the end of its result there; both sides refuse)"""
    s = E.short_map()
    P = L.make_params("rot")
    try:
        gpu_ctx.set_debug(True)
        outs = [_single(gpu_ctx, P, s["map_xyz"], s["q_local"], lpq, 1)[0] for lpq in (1, 0, 16)] + _window(gpu_ctx, P, s["map_xyz"], s["q_local"], 0)
    finally:
        _restore(gpu_ctx, P)
    for g in outs:
        assert g["rec"]["count"] == 0 and g["rec"]["query_index"].size == 0 and (g["idx"] == -1).all()


def test_edge_fit_swapped_ends_move_nothing(gpu_ctx, oracle):
    """A sign tie cannot move a pose: the edge factor (LidarKeyframeFactor.h:38-44) is |(p - A) x (p - B)| / |A - B|, symmetric in A and B.  The records of the
    case that holds the canon_sign ties, linearised at the association pose: the device's Gram and cost equal the oracle's evaluation of the same records to
    1e-12 of the largest entry (the project's Gram bound), and so does the evaluation with A and B swapped in EVERY record; the unweighted residuals, recomputed
    in numpy, are bit-identical under the swap."""
    s, rec, mdl = E.reference("aligned", "origin", "rot")
    n = s["n"]
    P, PO = L.make_params("rot"), oracle.params("rot")
    try:
        gpu_ctx.set_debug(True)
        g, m = _single(gpu_ctx, P, s["map_xyz"], s["q_local"], 0, 1)
        G, cost, counts = m.linearize(0, E.T_ASSOC, E.Q_ASSOC, L.MASK_EDGE)
    finally:
        _restore(gpu_ctx, P)
    r = g["rec"]
    n_e = r["count"]
    valid, a, b = _full(r, n)
    assert counts[1] == n_e > 100 and (mdl["tied"] & valid).sum() > 50
    re_ = dict(valid=valid.astype(np.uint8), cp=np.ascontiguousarray(s["q_local"]), a=a, b=b, s=np.full(n, P.lidar_const, np.float32))
    Go, co, no = oracle.linearize_edge(re_, E.T_ASSOC, E.Q_ASSOC, PO, (200.0, n_e))
    Gs, cs, ns = oracle.linearize_edge(dict(re_, a=b, b=a), E.T_ASSOC, E.Q_ASSOC, PO, (200.0, n_e))
    scale = np.abs(Go).max()
    assert no == ns == n_e and scale > 0
    assert np.abs(G - Go).max() <= 1e-12 * scale and abs(cost - co) <= 1e-12 * abs(co)
    assert np.abs(Gs - Go).max() <= 1e-12 * scale and abs(cs - co) <= 1e-12 * abs(co)
    assert np.abs(G - Gs).max() <= 1e-12 * scale and abs(cost - cs) <= 1e-12 * abs(co)
    lp = s["q_map"].astype(np.float64)[valid]          # (the factor moves the f32 query by the pose in f64; the rounded point serves the symmetry just as well)
    A, B = a[valid].astype(np.float64), b[valid].astype(np.float64)
    res = lambda A, B: np.linalg.norm(np.cross(lp - A, lp - B), axis=1) / np.linalg.norm(A - B, axis=1)
    assert np.array_equal(res(A, B), res(B, A))
