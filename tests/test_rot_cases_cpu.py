"""Conditions on the inputs of tests/rot_cases.py, on the oracle alone (atan_mode = 2, stable_sort = 1) and the two small numpy models kept beside the cases:
every case sits in the branch it claims and away from every threshold it does not mean to test.  tests/test_rot_branches_gpu.py then holds the device against
the oracle on the same cases, tests/test_reference_cpu.py the oracle against the reference's own Preprocessing.cpp."""
import functools

import numpy as np
import pytest

from tests import rot_cases as RC

PI = np.pi


@functools.lru_cache(maxsize=None)
def _oracle_of(name):
    from oracle import oracle as O
    O.build()
    return RC.run_oracle(O, RC.by_name(name))


def _names(*families):
    return [c["name"] for c in RC.cases_of(*families)]


def _ring_of_full(o):
    """Ring id of every point of the concatenated cloud, from the ring table."""
    n = o["full"].shape[0]
    ring = np.full(n, -1, np.int64)
    cnt = o["ring_end"] - o["ring_start"] + 11
    for r in range(len(cnt)):
        if cnt[r] > 0:
            ring[o["ring_start"][r] - 5:o["ring_end"][r] + 6] = r
    return ring, cnt


def test_every_family_has_cases():
    for f in RC.FAMILIES:
        assert len(RC.cases_of(f)) >= 1, f
    for c in RC.all_cases():
        assert set(c) == {"name", "family", "raw", "n_scans", "ds_rate", "ds_v", "near_range", "q_imu", "q_lb", "claim", "ref"}
        assert c["raw"].shape[0] <= 300_000


# ------------------------------------------------------------------------------------------------ sweep, latch, reltime
@pytest.mark.parametrize("name", _names("sweep", "latch", "reltime"))
def test_azimuth_branches_match_the_claim(oracle, name):
    c = RC.by_name(name)
    o = _oracle_of(name)
    cl = c["claim"]
    m32, m64 = RC.azimuth_model(c, o["full_src"], np.float32), RC.azimuth_model(c, o["full_src"], np.float64)
    print(name, {k: m32[k] for k in ("corr", "half_idx", "A1", "A2", "B1", "B2", "rel_min", "rel_max")})
    for m in (m32, m64):                                    # float32 as the reference computes, float64: no count hangs on a rounding
        assert m["corr"] == cl["corr"]
        assert m["half_idx"] == cl["half_idx"]
        for k in ("A1", "A2", "B1", "B2"):
            assert m[k] == cl[k], k
        assert abs(m["rel_min"] - cl["rel_min"]) < 1e-4 and abs(m["rel_max"] - cl["rel_max"]) < 1e-4
    # the model IS the oracle: intensity = ring + 0.1 * relTime of every point, bit for bit (the arctangents are numpy's: allow their last bit)
    ring, _ = _ring_of_full(o)
    order = np.argsort(o["full_src"], kind="stable")
    want = (ring[order].astype(np.float64) + 0.1 * m32["rel"].astype(np.float64)).astype(np.float32)
    np.testing.assert_allclose(o["full"][order, 3], want, rtol=0, atol=4e-6)
    if "half_idx_by_hand" in cl and cl["half_idx_by_hand"] is not None:
        assert m32["half_idx"] == cl["half_idx_by_hand"]
    if name == "latch_natural":                             # about half way, in no special place
        assert 9000 < m32["half_idx"] < 10500
    if "by_hand" in cl:
        h = cl["by_hand"]
        assert h["rel_min"][0] <= m32["rel_min"] <= h["rel_min"][1] and h["rel_max"][0] <= m32["rel_max"] <= h["rel_max"][1]
        neg = ring[order][m32["rel"] < 0]
        if h["neg_rings"] == "zero":
            assert neg.size >= 20 and (neg == 0).all()
            assert (o["full"][order, 3][m32["rel"] < 0] < 0).all()          # intensity < 0: (int) truncates towards zero, the slerp parameter is negative
        elif h["neg_rings"] == "positive":
            assert neg.size >= 50 and (neg > 0).all()
            i = o["full"][order, 3][m32["rel"] < 0]
            assert np.array_equal(i.astype(np.int64), neg - 1)              # line = id - 1
        else:
            assert neg.size == 0 and (m32["rel"] >= 1).sum() >= 50


def test_azimuth_families_cover_every_branch():
    cs = RC.cases_of("sweep", "latch", "reltime")
    cl = [c["claim"] for c in cs]
    for k in ("A1", "A2", "B1", "B2"):
        assert max(x[k] for x in cl) >= 100, k                 # each wrap branch taken by >= 100 points in some case
        assert min(x[k] for x in cl) == 0, k
    assert {x["corr"] for x in cl} == {"none", "minus", "plus"}
    sw = [c["claim"] for c in RC.cases_of("sweep")]
    for s in RC.SWEEP_STARTS:                                  # every start azimuth sees a sweep that latches and one that does not
        mine = [x for x in sw if x["start"] == s]
        assert any(x["half_idx"] == RC.INT_MAX for x in mine) and any(x["half_idx"] != RC.INT_MAX for x in mine)
    assert any(x["half_idx"] == RC.INT_MAX and x["sweep"] < PI for x in sw)
    assert any(x["rel_min"] < -0.01 for x in cl) and any(x["rel_max"] > 1.01 for x in cl)
    # no azimuth of a design lies within 1e-4 rad of a threshold: checked by the float32 / float64 agreement above; the latch cases differ only in the stray point
    lat = {c["name"]: c for c in RC.cases_of("latch")}
    for a, b, row in (("latch_none", "latch_last_workgroup", RC.LATCH_LAST_ROW), ("latch_natural", "latch_row_1023", 1023), ("latch_natural", "latch_row_1024", 1024)):
        d = np.nonzero((lat[a]["raw"].view(np.uint32) != lat[b]["raw"].view(np.uint32)).any(axis=1))[0]
        assert list(d) == [row]
    n = lat["latch_none"]["raw"].shape[0]
    assert RC.LATCH_LAST_ROW // 1024 == (n - 1) // 1024 and lat["latch_last_workgroup"]["claim"]["half_idx"] == RC.LATCH_LAST_ROW


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", _names("tables"))
def test_ring_tables_at_every_boundary(oracle, name):
    c = RC.by_name(name)
    ids = c["claim"]["ids"]
    res = [RC.run_oracle(oracle, c, atan_mode=m) for m in (0, 1, 2)]
    for o in res:
        got = np.full(c["raw"].shape[0], -1, np.int64)
        ring, _ = _ring_of_full(o)
        got[o["full_src"]] = ring
        assert np.array_equal(got, ids)                      # every point on the ring its designed elevation says, in all three atan definitions
    assert (ids < 0).sum() == c["claim"]["n_dropped"] > 0
    hit = c["claim"]["ids_hit"]
    assert hit == list(range(c["n_scans"] if c["n_scans"] != 64 else 51))      # every ring of the table, 0 .. 50 of the 64-ring table
    if c["n_scans"] == 64:
        assert RC.table_id(-18.08 + 0.02, 64) == 50 and RC.table_id(-18.08 - 0.02, 64) == -1     # scanID 50 | 51
        assert RC.table_id(-8.83 + 0.02, 64) == 32 == RC.table_id(-8.83 - 0.02, 64)
        assert RC.table_id(2.02, 64) == -1 and RC.table_id(1.98, 64) == 0
    if c["n_scans"] == 16:
        assert RC.table_id(-17.98, 16) == 0 and RC.table_id(-18.02, 16) == -1 and RC.table_id(15.98, 16) == 15 and RC.table_id(16.02, 16) == -1
    if c["n_scans"] == 32:
        assert RC.table_id(-31.98, 32) == 0 and RC.table_id(-32.02, 32) == -1 and RC.table_id(11.98, 32) == 31 and RC.table_id(12.02, 32) == -1


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("name", _names("sizes"))
def test_sizes_match_the_claim(oracle, name):
    c = RC.by_name(name)
    o = _oracle_of(name)
    cl = c["claim"]
    assert c["raw"].shape[0] == cl["rows"]
    _, cnt = _ring_of_full(o)
    span = o["ring_end"] - o["ring_start"]
    if "ring_counts" in cl:
        assert list(cnt) == list(cl["ring_counts"])
    if name == "sizes_two_trips":
        assert cl["rows"] >= RC.ONE_TRIP_ROWS + 1 + 1024 and o["full"].shape[0] == cl["n_full"]
        assert cnt.max() == cl["max_ring"] <= RC.LDS_CAP and len(o["edge_idx"]) > 100 and len(o["surf"]) > 1000
    if name == "sizes_ring_counts":
        assert (span[[0, 1, 13, 14]] < 0).all() and span[2] == 0 and span[3] == 5 and span[4] == 6 and span[5] == 63 and span[6] == 64
        sel = [r for r in range(16) if span[r] >= 6]
        assert sel == [4, 5, 6, 7, 10, 11, 12, 15]
        ring, _ = _ring_of_full(o)
        assert set(ring[o["lessflat_idx"]]) | set(ring[o["edge_idx"]]) == set(sel)
    if cl.get("mixed"):
        sel = cnt[span >= 6]
        assert (sel <= RC.LDS_CAP).any() and (sel > RC.LDS_CAP).any() and RC.LDS_CAP in sel and RC.LDS_CAP + 1 in sel
        assert span.max() == RC.LDS_CAP + 1 - 11
    if "min_segment" in cl:
        r = int(np.argmax(cnt))
        seg = [RC.segment_bounds(int(cnt[r]), j) for j in range(6)]
        assert min(ep - sp + 1 for sp, ep in seg) >= cl["min_segment"] and len(o["edge_idx"]) >= 10
    if name.startswith("sizes_n"):
        assert o["full"].shape[0] <= cl["rows"] and (cl["rows"] > 1 or o["full"].shape[0] == 1)


# ------------------------------------------------------------------------------------------------ picks, borders: margins and the segment model
def _selected_segments(o, n_scans, ds_rate):
    for r in range(n_scans):
        rs, re = int(o["ring_start"][r]), int(o["ring_end"][r])
        if re - rs >= 6 and r % ds_rate == 0:
            for j in range(6):
                yield r, j, rs + (re - rs) * j // 6, rs + (re - rs) * (j + 1) // 6 - 1


@pytest.mark.parametrize("name", _names("picks", "borders"))
def test_polyline_margins_and_model(oracle, name):
    """No curvature of a selected segment within a factor 1.05 of 2.0 or 0.1, no gap a pick's suppression tests within 1.02 of 0.05; the serial model gives the
    oracle's picks."""
    c = RC.by_name(name)
    o = _oracle_of(name)
    cv = o["curvature"].astype(np.float64)
    for r, j, sp, ep in _selected_segments(o, c["n_scans"], c["ds_rate"]):
        s = cv[sp:ep + 1]
        for thr in (RC.CURV_SHARP, RC.CURV_FLAT):
            assert not ((s > thr / 1.05) & (s < thr * 1.05)).any(), (j, thr, s[(s > thr / 1.05) & (s < thr * 1.05)])
    picks = np.concatenate([o["edge_idx"], o["flat_idx"]])
    for p in picks:
        for l in range(-5, 5):
            g = float(RC.gap2(o["full"], p + l + 1, p + l))
            assert not (RC.GAP_BREAK / 1.02 < g < RC.GAP_BREAK * 1.02), (p, l, g)
    ser = RC.ring_serial(o, RC.POLY_RING)
    assert [i for s in ser for i in s["edge"]] == list(o["edge_idx"])
    assert [i for s in ser for i in s["flat"]] == list(o["flat_idx"])
    assert o["n_ties"] == 0


def test_picks_claims(oracle):
    # 2, 10 and 12 eligible candidates
    c, o = RC.by_name("picks_counts"), _oracle_of("picks_counts")
    ser = RC.ring_serial(o, RC.POLY_RING)
    for j, cnt in c["claim"]["eligible"].items():
        sp, ep = ser[j]["sp"], ser[j]["ep"]
        el = np.nonzero(o["curvature"][sp:ep + 1] > RC.CURV_SHARP)[0] + sp
        assert list(el) == [k for k in c["claim"]["spikes"] if sp <= k <= ep] and len(el) == cnt
        assert len(ser[j]["edge"]) == min(cnt, 10)
        assert (o["label"][ser[j]["edge"]] == 2).sum() == 2 and (o["label"][ser[j]["edge"]] == 1).sum() == min(cnt, 10) - 2
    # the fourth flat pick: the candidate next in the order after the third pick lies within five points of it and is passed over; the fourth pick marks nothing
    c, o = RC.by_name("picks_flat_fourth"), _oracle_of("picks_flat_fourth")
    ser = RC.ring_serial(o, RC.POLY_RING)
    s0 = ser[0]
    assert s0["flat"] == c["claim"]["flat_seg0"]
    order = s0["sp"] + np.argsort(o["curvature"][s0["sp"]:s0["ep"] + 1], kind="stable")
    third = int(np.nonzero(order == s0["flat"][2])[0][0])
    assert order[third + 1] == c["claim"]["skipped"] and abs(int(order[third + 1]) - s0["flat"][2]) <= 5 and o["label"][order[third + 1]] == 0
    assert (o["curvature"][order[:60]] < RC.CURV_FLAT / 1.05).sum() >= 30
    marks = ser[1]["marks_in"]
    f4 = s0["flat"][3]
    assert marks[f4:f4 + 6].sum() == 0 and marks[f4 - 5:f4].sum() == 5 and marks[s0["flat"][2]] == 1      # broke BEFORE its suppression (the five before it: the third pick's)
    # gaps at every offset
    c, o = RC.by_name("picks_gaps"), _oracle_of("picks_gaps")
    seen = set()
    for p, l, side in c["claim"]["gaps"]:
        assert p in o["edge_idx"]
        b = RC.break_offset(o["full"], p, 1 if l > 0 else -1)
        g = float(RC.gap2(o["full"], p + l, p + l - 1) if l > 0 else RC.gap2(o["full"], p + l, p + l + 1))
        if side == "above":
            assert b == abs(l) and RC.GAP_BREAK * 1.02 <= g <= RC.GAP_BREAK * 1.05, (p, l, b, g)
        else:
            assert b is None and RC.GAP_BREAK / 1.05 <= g <= RC.GAP_BREAK / 1.02, (p, l, b, g)
        seen.add((l, side))
    assert len(seen) == 20
    # the caps
    c, o = RC.by_name("picks_caps"), _oracle_of("picks_caps")
    assert (len(o["edge_idx"]), len(o["sharp_idx"]), len(o["flat_idx"])) == c["claim"]["caps"]
    assert all(len(s["edge"]) == 10 and len(s["flat"]) == 4 for s in RC.ring_serial(o, RC.POLY_RING))


@pytest.mark.parametrize("name", _names("borders"))
def test_borders_claims(oracle, name):
    c, o = RC.by_name(name), _oracle_of(name)
    cl = c["claim"]
    ser = RC.ring_serial(o, RC.POLY_RING)
    serial_edges = set(int(i) for i in o["edge_idx"])
    for j, p in cl["hit"]:
        alone = RC.segment_alone(o, RC.POLY_RING, j)
        assert p in alone["edge"] and p not in serial_edges and 0 <= p - alone["sp"] < 5 and ser[j]["marks_in"][p] == 1
    for j, p in cl["not_hit"]:
        alone = RC.segment_alone(o, RC.POLY_RING, j)
        assert alone["edge"] == ser[j]["edge"] and alone["flat"] == ser[j]["flat"] and p in serial_edges and 0 <= p - alone["sp"] < 5
        assert ser[j]["marks_in"][alone["sp"]:alone["sp"] + 5].sum() == 0
        prev = [e for e in ser[j - 1]["edge"] if e >= ser[j - 1]["ep"] - 4]
        assert prev                                           # there IS a pick in the last five of the segment before: its marks stop at the gap
    if "chain" in cl:
        (j, _), (j1, e) = cl["hit"][0], cl["chain"]
        assert j1 == j + 1
        first = RC.segment_alone(o, RC.POLY_RING, j)                                        # segment j as it first runs: no incoming marks
        alone1 = RC.segment_alone(o, RC.POLY_RING, j1)
        with_first = RC.segment_alone(o, RC.POLY_RING, j1, marks_in=_spill_only(first, alone1))
        assert with_first["edge"] == alone1["edge"] and e in alone1["edge"]                   # the first run's spill does not reach E ...
        assert 0 <= e - alone1["sp"] < 5 and e not in serial_edges and ser[j1]["marks_in"][e] == 1   # ... the redo's does
        assert len(first["edge"]) == 10 and len(ser[j]["edge"]) == 10 and set(first["edge"]) != set(ser[j]["edge"])
    # everything else of the ring is where an independent run and the serial run agree
    special = {j for j, _ in cl["hit"]} | ({cl["chain"][0]} if "chain" in cl else set())
    for j in range(6):
        if j not in special:
            a = RC.segment_alone(o, RC.POLY_RING, j)
            assert a["edge"] == ser[j]["edge"] and a["flat"] == ser[j]["flat"], j


def _spill_only(first, nxt):
    """Marks of a segment's run restricted to the first five points of the next segment."""
    m = np.zeros_like(first["marks_out"])
    m[nxt["sp"]:nxt["sp"] + 5] = first["marks_out"][nxt["sp"]:nxt["sp"] + 5]
    return m


# ------------------------------------------------------------------------------------------------ near
def test_near_claims(oracle):
    c, o = RC.by_name("near_half_metre"), _oracle_of("near_half_metre")
    r2 = np.array([float(RC.range2(o["full"], k)) for k in range(o["full"].shape[0])])
    near = r2 < 0.25
    assert near.sum() >= c["claim"]["min_near"] and not near[o["flat_idx"]].any() and not near[o["lessflat_idx"]].any()
    assert ((r2 > 0.25 / 1.05) & (r2 < 0.25 * 1.05)).sum() == 0
    would = []
    for r in range(16):
        for s in RC.ring_serial(o, r, near_check=False):
            would += [k for k in s["flat"] if near[k]]
    assert len(would) >= c["claim"]["min_flat_otherwise"] and (o["curvature"][would] < RC.CURV_FLAT / 1.05).all()
    assert len(o["flat_idx"]) >= 16                            # the farther points still give flat picks
    v = RC.voxel_coords(o["full"][:, :3], c["ds_v"])
    far_vox = {tuple(x) for x in v[o["lessflat_idx"]]}
    assert sum(tuple(x) in far_vox for x in v[near]) >= 20     # near points in voxels that farther points fill


# ------------------------------------------------------------------------------------------------ voxels
def _interior(o):
    """Ring-interior points [scanStartInd, scanEndInd]: the ones k_rot_scatter forms a voxel key for."""
    m = np.zeros(o["full"].shape[0], bool)
    for r in range(len(o["ring_start"])):
        if o["ring_end"][r] >= o["ring_start"][r]:
            m[o["ring_start"][r]:o["ring_end"][r] + 1] = True
    return m


def test_voxels_claims(oracle):
    c, o = RC.by_name("voxels_alternating"), _oracle_of("voxels_alternating")
    v = RC.voxel_coords(o["full"][o["lessflat_idx"], :3], c["ds_v"])
    runs = 1 + int((v[1:] != v[:-1]).any(axis=1).sum())
    assert len({tuple(x) for x in v}) == c["claim"]["n_voxels"] == o["surf"].shape[0]
    assert runs == v.shape[0] >= c["claim"]["min_runs"]        # the run count equals the candidate count
    assert sorted(o["surf_cnt"])[0] > 1400

    c, o = RC.by_name("voxels_all_picked"), _oracle_of("voxels_all_picked")
    v = RC.voxel_coords(o["full"][:, :3], c["ds_v"])
    lf = {tuple(x) for x in v[o["lessflat_idx"]]}
    inner = _interior(o)
    for p in c["claim"]["spikes"]:
        assert o["label"][p] > 0 and tuple(v[p]) not in lf                      # its voxel: no less-flat point, no centroid
        assert all(o["label"][k] > 0 for k in np.nonzero(inner & (v == v[p]).all(axis=1))[0])
    assert o["surf"].shape[0] == len(lf)

    lim = np.array([[-1024, 1023], [-1024, 1023], [-256, 255]])
    crossed = {}
    for name in ("voxels_last_key", "voxels_one_past"):
        c, o = RC.by_name(name), _oracle_of(name)
        v = RC.voxel_coords(o["full"][_interior(o), :3], c["ds_v"])
        out = ((v < lim[:, 0]) | (v > lim[:, 1]))
        crossed[name] = int(out.any(axis=1).sum())
        assert crossed[name] == c["claim"]["overflow"]
        for k in range(3):                                                      # the last packed coordinate on either side is there
            assert (v[:, k] == lim[k, 0]).any() and (v[:, k] == lim[k, 1]).any(), (name, k)
        if crossed[name]:
            assert v[out.any(axis=1)][0, 0] == lim[0, 1] + 1 and out.sum() == 1      # by one voxel, in x
        frac = o["full"][_interior(o), :3].astype(np.float64) / c["ds_v"]
        at_limit = (v <= lim[:, 0]) | (v >= lim[:, 1])
        assert (np.abs(frac - np.round(frac))[at_limit] > 0.2).all()             # the points on the last coordinates sit in the middle of their voxels
    assert crossed == {"voxels_last_key": 0, "voxels_one_past": 1}

    for ds in (3, 5, 17):
        c, o = RC.by_name(f"voxels_ds_rate_{ds}"), _oracle_of(f"voxels_ds_rate_{ds}")
        ring, _ = _ring_of_full(o)
        assert sorted(set(ring[o["lessflat_idx"]])) == c["claim"]["rings"] and set(ring[o["edge_idx"]]) <= set(c["claim"]["rings"])
        assert len(o["surf"]) > 50


# ------------------------------------------------------------------------------------------------ ties, slerp, the link to the reference
def test_ties_claims(oracle):
    c, o = RC.by_name("ties_collinear"), _oracle_of("ties_collinear")
    assert o["n_ties"] >= c["claim"]["min_ties"] and np.array_equal(o["curvature"].view(np.uint32), np.zeros(o["full"].shape[0], np.uint32))   # every curvature +0
    assert np.array_equal(o["full"][:, :3].view(np.uint32), c["raw"][:, :3].view(np.uint32))
    for s in RC.ring_serial(o, 6):
        assert s["flat"] == [s["sp"], s["sp"] + 6, s["sp"] + 12, s["sp"] + 18]                  # all ranks come from the index
    c, o = RC.by_name("ties_equal_spikes"), _oracle_of("ties_equal_spikes")
    sharp = o["curvature"] > RC.CURV_SHARP
    assert o["n_ties"] >= c["claim"]["min_ties"] and sharp.sum() > 70 and (o["curvature"][sharp] == np.float32(c["claim"]["spike_curv"])).all()
    ser = RC.ring_serial(o, 6)
    assert [i for s in ser for i in s["edge"]] == list(o["edge_idx"])
    for s in ser:                                                                              # more than ten equal candidates: the ten with the LARGEST indices
        el = np.nonzero(sharp[s["sp"]:s["ep"] + 1])[0] + s["sp"]
        assert len(el) > 10 and s["edge"] == list(el[::-1][:10])
    assert np.unique(o["curvature"][(o["curvature"] > 0) & ~sharp]).size == 1


def test_slerp_cases(oracle):
    cs = RC.cases_of("slerp")
    assert {c["claim"]["q"] for c in cs} == set(RC.SLERP_Q) and len(cs) == 2 * len(RC.SLERP_Q)
    q = RC.SLERP_Q
    assert q["identity"] == RC.IDENTITY and q["negated"][0] < 0 and abs(2 * np.arccos(q["three_rad"][0]) - 3.0) < 1e-12
    assert 1.0 - 2.2e-16 <= q["one_ulp_below_one"][0] < 1.0 and any(v != 0 for v in q["one_ulp_below_one"][1:])
    by = {c["name"]: _oracle_of(c["name"]) for c in cs}
    for ln in ("qlb", "unit"):
        ident, neg, three = by[f"slerp_identity_{ln}"], by[f"slerp_negated_{ln}"], by[f"slerp_three_rad_{ln}"]
        raw = cs[0]["raw"]
        assert np.abs(ident["full"][:, :3] - raw[ident["full_src"], :3]).max() < 1e-4               # identity: nothing moves
        assert np.abs(neg["full"][:, :3] - ident["full"][:, :3]).max() > 0.05                       # q and -q: the same small rotation
        assert np.abs(three["full"][:, :3] - ident["full"][:, :3]).max() > 50.0                     # 3 rad over the sweep
        assert np.abs(by[f"slerp_one_ulp_below_one_{ln}"]["full"][:, :3] - ident["full"][:, :3]).max() < 1e-4


def test_reference_link_cases_have_no_ties(oracle):
    """Every case that takes part in the comparison with the literal reference build: no equal curvatures inside a sorted segment (std::sort's order on ties is
    unspecified), parameters the node can express."""
    n = 0
    for c in RC.all_cases():
        if c["ref"]:
            o = _oracle_of(c["name"])
            assert o["n_ties"] == 0, c["name"]
            assert c["near_range"] == 3.0 and c["ds_v"] == 0.6 and c["n_scans"] in (16, 32, 64)
            n += 1
    assert n >= 50 and not any(c["ref"] for c in RC.cases_of("near", "ties"))
    assert {c["family"] for c in RC.all_cases() if c["ref"]} == set(RC.FAMILIES) - {"near", "ties"}
