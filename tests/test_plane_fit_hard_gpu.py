"""The plane fit of the association kernels (surf_fit, lili_s2m_dev.h) on hard neighbourhoods, through every launcher that calls it, against the oracle —
which solves every fit by the column-pivoted Householder QR where the device takes the centred normal equations above the switch — and against the exact
model of tests/plane_fit_cases.py (cases, kinds, bounds and margins are described there; tests/test_plane_fit_cases_cpu.py holds the oracle to the model).

Launchers: the one-lane kernel (assoc_lpq 1, lili_s2m.hip), the cooperative kernel with 2 / 4 / 8 / 16 lanes per query and the default choice (assoc_lpq 0,
lili_s2m_coop.hip), each with the super-row layout on and off; associate_window over two slots; the dense-map launch (k_associate_fine, lili_s2m_dense.hip) in a
fresh context, the clusters laid into a filler cloud that lifts the occupancy over the fine index's threshold and stays outside every gate.  On the one-lane
kernel also LILI_DEBUG 16384 (the QR everywhere) and 2048 (the fast path wherever its denominator is positive), held to the model and the oracle like the
default, with the bound of their own path; they need not be bit-equal to it.

What must hold: neighbour indices and d^2 are the oracle's bit for bit inside the radius and no query outside has d2[4] < kd_max_radius; all launchers give
bit-identical records, undecided clusters included; the valid flags are the oracle's and the model's on every decided query; n and d are within one f32 ulp +
8 x the bound of the model (queries with a meaningful direction) and within the two sides' joint bound of the oracle (every rank-decided query, the basic
solution of the zero-column clusters among them); the score is 1 (frontend), lidar_const times a float within one ulp of the oracle's weight (rot), within one
f32 ulp relative of the oracle's (livox); cp is the local query."""
import os

import numpy as np
import pytest

import lili_om_amd as L
from tests import plane_fit_cases as P

pytestmark = pytest.mark.gpu

SINGLE = [(lpq, sr) for sr in (1, 0) for lpq in (1, 2, 4, 8, 16, 0)]


def _take(m, slot, n):
    idx, d2 = m.neighbors(slot, L.KIND_SURF, n)
    return dict(idx=idx, d2=d2, rec=m.surf_records(slot, n))


def _single(ctx, prm, mp, ql, lpq, super_rows):
    ctx.set_option("assoc_lpq", lpq)
    ctx.set_option("super_rows", super_rows)
    m = L.ScanToMapMatcher(ctx, prm)
    m.map_focus(None)
    m.set_input_cloud(L.KIND_SURF, mp)
    m.set_queries(0, L.KIND_SURF, ql)
    n = m.find_corresponding_surf_features(0, P.Q_ASSOC, P.T_ASSOC)
    out = _take(m, 0, ql.shape[0])
    assert out["rec"]["count"] == n
    return out


def _with_debug(bits, fn):
    """fn() with LILI_DEBUG = bits (0: unset), the environment restored"""
    old = os.environ.get("LILI_DEBUG")
    if bits:
        os.environ["LILI_DEBUG"] = str(bits)
    else:
        os.environ.pop("LILI_DEBUG", None)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("LILI_DEBUG", None)
        else:
            os.environ["LILI_DEBUG"] = old


def _window(ctx, prm, mp, ql, lpq):
    ctx.set_option("assoc_lpq", lpq)
    ctx.set_option("super_rows", 1)
    m = L.ScanToMapMatcher(ctx, prm)
    m.map_focus(None)
    m.set_input_cloud(L.KIND_SURF, mp)
    for slot in (0, 1):
        m.set_queries(slot, L.KIND_SURF, ql)
    counts = m.associate_window([0, 1], [P.T_ASSOC] * 2, [P.Q_ASSOC] * 2, L.MASK_SURF)
    outs = [_take(m, slot, ql.shape[0]) for slot in (0, 1)]
    assert [c[0] for c in counts] == [o["rec"]["count"] for o in outs] and all(c[1] == 0 for c in counts)
    return outs


def _dense(prm, mp, filler, ql):
    """one build of clusters + filler in a fresh context (no hint of an earlier map): the fine index, hence k_associate_fine"""
    ctx = L.Context(0)
    try:
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, prm)
        m.set_input_cloud(L.KIND_SURF, np.ascontiguousarray(np.r_[mp, filler]))
        occ, fcell, fr2 = m.map_density(L.KIND_SURF)
        assert occ > 12 and fcell > 0 and fr2 > 0, (occ, fcell, fr2)             # the dense launch is the one taken (launch_associate: dense = has_fine)
        m.set_queries(0, L.KIND_SURF, ql)
        n = m.find_corresponding_surf_features(0, P.Q_ASSOC, P.T_ASSOC)
        out = _take(m, 0, ql.shape[0])
        assert out["rec"]["count"] == n
        return out
    finally:
        ctx.close()


def _restore(ctx, prm):
    ctx.set_option("assoc_lpq", 0)
    ctx.set_option("super_rows", 1)
    ctx.set_debug(False)
    L.ScanToMapMatcher(ctx, prm).map_focus(None)


def _all_launchers(ctx, prm, mp, ql, filler):
    """[(name, result)] — the first entry is the one-lane kernel"""
    got = []
    for lpq, sr in SINGLE:
        got.append((f"lpq {lpq} super_rows {sr}", _single(ctx, prm, mp, ql, lpq, sr)))
    for lpq in (0, 4):
        for slot, out in enumerate(_window(ctx, prm, mp, ql, lpq)):
            got.append((f"window lpq {lpq} slot {slot}", out))
    got.append(("dense", _dense(prm, mp, filler, ql)))
    return got


def _full(rec, n):
    """the compacted record list spread over the queries"""
    valid = np.zeros(n, bool); nn = np.zeros((n, 3), np.float32); d = np.zeros(n, np.float32); sc = np.zeros(n)
    qi = rec["query_index"]
    valid[qi] = True; nn[qi] = rec["n"]; d[qi] = rec["d"]; sc[qi] = rec["score"]
    return valid, nn, d, sc


def _check_mode(case, offset, variant, mode, s, rec, g, prm):
    """one run (the records g of the one-lane kernel under one LILI_DEBUG) against the oracle's records rec and the model built with that run's bound"""
    m = P.model(case, offset, variant, mode)
    tag = f"{case} {offset} {variant} {mode}"
    n, kind = s["n"], s["kind"]
    o_valid = rec["valid"].astype(bool)
    g_valid, gn, gd, gs = _full(g["rec"], n)
    dec = m["decided"]
    diff = np.nonzero(g_valid != o_valid)[0]
    # valid flags: the oracle's and the model's on every decided query, no tolerance
    bad = dec & ((g_valid != o_valid) | (g_valid != m["valid"]))
    und = {k: int((~dec & (kind == k)).sum()) for k in sorted(set(kind[~dec].tolist()))}
    print(f"\n{tag}: {P.summary(case, offset, variant, mode)}\n  device valid {int(g_valid.sum())}, oracle {int(o_valid.sum())}; differs from the oracle on {diff.size} undecided "
          f"{sorted(set(kind[diff].tolist()))}; undecided by kind {und}")
    assert not bad.any(), (tag, kind[bad][:10], np.nonzero(bad)[0][:10])
    assert not g_valid[m["nan_drop"]].any()                                       # dropped through NaN, as the reference does
    assert g_valid[kind == "dexact"].all()                                        # the largest residual EQUALS surf_dist_thres, in exact arithmetic on every path: a strict >
    # n and d: the model within one f32 ulp + 8 x the bound where the direction means something; the oracle within the joint bound on every rank-decided query
    sel_m = g_valid & m["solved"] & m["meaningful"]
    worst_m, at_m, _ = P.record_excess(gn, gd, m, sel_m, P.DEVICE_FACTOR)
    sel_o = g_valid & o_valid & m["rank_decided"]
    worst_o, at_o, _ = P.oracle_excess(gn, gd, rec["n"], rec["d"], m, sel_o, P.DEVICE_FACTOR)
    same = int((gn[sel_o].view(np.uint32) == rec["n"][sel_o].view(np.uint32)).all(1).sum())
    print(f"  worst err / (ulp + 8 B) against the model {worst_m:.3f} ({kind[at_m]}, B {m['B'][at_m]:.3g}) on {int(sel_m.sum())} queries; against the oracle {worst_o:.3f} "
          f"({kind[at_o]}) on {int(sel_o.sum())}, {same} normals bit-equal")
    assert worst_m <= 1.0, (tag, worst_m, at_m, kind[at_m])
    assert worst_o <= 1.0, (tag, worst_o, at_o, kind[at_o])
    zc = g_valid & m["rank_deficient"]
    axis = np.argmax((s["map_xyz"][m["idx"]] == 0).all(1), axis=1)
    assert (gn[zc, axis[zc]] == 0).all()                                          # the basic solution: nothing along an exactly zero column
    # score; the float weight may differ from the oracle's by what the solutions differ by, carried through pd, and one rounding
    r = g["rec"]
    qn = np.linalg.norm(s["q_map"].astype(np.float64), axis=1)
    slack = 0.9 * ((1.0 + P.DEVICE_FACTOR) * m["B"] + 8.0 * P.EPS) * (qn + m["ninv"]) / np.sqrt(qn)
    if variant == "frontend":
        assert (r["score"] == 1.0).all()
    elif variant == "rot":
        wq = gs / prm.lidar_const
        assert np.array_equal(wq[g_valid], wq[g_valid].astype(np.float32).astype(np.float64))                                  # the weight is a float
        wo = rec["score"] / prm.lidar_const
        assert (np.abs(wq - wo) <= np.spacing(np.maximum(wq, wo).astype(np.float32)).astype(np.float64) + slack)[sel_o].all()
    else:
        assert (np.abs(gs - rec["score"]) <= 2.0 ** -23 * np.abs(rec["score"]) + prm.lidar_const * slack)[sel_o].all()
    assert np.array_equal(r["cp"], s["q_local"][r["query_index"]])
    return worst_m, worst_o


@pytest.mark.parametrize("case,offset,variant", P.GRID)
def test_plane_fit_on_hard_neighbourhoods_through_every_launcher(gpu_ctx, oracle, case, offset, variant):
    s, rec = P.reference(case, offset, variant)
    n = s["n"]
    mp, ql = P.clouds(s, variant)
    prm = L.make_params(variant, **P.overrides(case, offset, variant))
    try:
        gpu_ctx.set_debug(True)
        got = _with_debug(0, lambda: _all_launchers(gpu_ctx, prm, mp, ql, P.dense_filler(case, offset, variant)))
        forced = {mode: _with_debug(P.MODES[mode], lambda: _single(gpu_ctx, prm, mp, ql, 1, 1)) for mode in ("qr", "fast")}
    finally:
        _restore(gpu_ctx, prm)
    inside = rec["nn_d2"][:, 4].astype(np.float64) < P.KD_MAX_RADIUS
    first = got[0][1]
    for name, g in got + [(mode, forced[mode]) for mode in forced]:
        # neighbours
        assert np.array_equal(g["idx"][inside], rec["nn_idx"][inside]), name
        assert np.array_equal(g["d2"][inside].view(np.uint32), rec["nn_d2"][inside].view(np.uint32)), name
        assert not (g["d2"][~inside][:, 4].astype(np.float64) < P.KD_MAX_RADIUS).any(), name
    for name, g in got:
        # the records of every launcher are those of the one-lane kernel, bit for bit
        assert g["rec"]["count"] == first["rec"]["count"], name
        for k in ("query_index", "cp", "n", "d", "score"):
            a, b = np.ascontiguousarray(g["rec"][k]), np.ascontiguousarray(first["rec"][k])
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, k)
    for mode, g in [("default", first)] + list(forced.items()):
        _check_mode(case, offset, variant, mode, s, rec, g, prm)
    # the strict gates on the device
    m = P.model(case, offset, variant)
    g_valid = _full(first["rec"], n)[0]
    if case == "refl":
        assert g_valid[s["kind"] == "refl_eq"].all() and not g_valid[s["kind"] == "refl_hi"].any()                              # sum_w == reflect_thres passes: a strict >
    if case == "gates":
        k = s["kind"] == "kgate"
        assert np.array_equal(g_valid[k], m["in_radius"][k])


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_plane_fit_short_map_refuses_every_query(gpu_ctx, variant):
    """four map points: fewer than five neighbours (the reference reads past the end of its result there; both sides refuse)"""
    s = P.short_map(variant)
    prm = L.make_params(variant)
    try:
        gpu_ctx.set_debug(True)
        outs = [_single(gpu_ctx, prm, s["map"], s["q"], lpq, 1) for lpq in (1, 0, 16)] + _window(gpu_ctx, prm, s["map"], s["q"], 0)
    finally:
        _restore(gpu_ctx, prm)
    for g in outs:
        assert g["rec"]["count"] == 0 and g["rec"]["query_index"].size == 0 and (g["idx"] == -1).all()
