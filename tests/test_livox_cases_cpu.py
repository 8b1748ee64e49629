"""The cases of tests/livox_cases.py on the oracle alone: every case is in the branch it claims to be in, and away from every threshold by a margin that
two correct implementations cannot differ by.  These are conditions on the INPUTS of tests/test_livox_branches_gpu.py, not measurements of the device.

  - per designed block: num, the number of lines with a candidate, the candidates and both decisions of the numpy model (livox_cases.block_model) are the
    case's claim, and the model's edge / surf cells are the oracle's, in order
  - ev0 / ev1 a factor 1.05 from surf_thres, ev2 / ev1 a factor 1.05 from edge_thres, every Laplacian 1e-3 from 0.06, rival maxima bit-equal or a relative
    1e-6 apart; where a normal or a direction is emitted its eigenvalue is 1e-3 of the largest away from its neighbour (what atol = 2e-6 on the stored
    vectors rests on)
Cases whose decision rests on the sign of rounding noise (the exactly collinear patch: ev0 ~ ev1 ~ 0) are not among them."""
import numpy as np
import pytest

from tests import livox_cases as LC


def _walk(oracle, case, q=LC.IDENTITY):
    o = oracle.extract_livox(case["rows"], q)
    xyz, curv = LC.grid_of(case["rows"], o)
    return o, xyz, curv, LC.depth_grid(xyz)


@pytest.mark.parametrize("case", [c for c in LC.constructed_cases() if c["name"] != "empty"], ids=lambda c: c["name"])
def test_constructed_case_is_where_it_claims(oracle, case):
    o, xyz, curv, dep = _walk(oracle, case)
    num = LC.occupancy(curv)
    edge_cells, surf_cells = [], []
    for b in range(LC.BLOCKS):
        claim = case["designed"].get(b)
        if claim is None:      # the rest of the grid: empty, or the context columns of a designed block
            assert num[b] <= 24, b
            continue
        m = LC.block_model(xyz, curv, dep, b)
        assert (m["num"], m["ne"], m["emit_edge"], m["emit_surf"]) == (claim["num"], claim["ne"], claim["edge"], claim["surf"]), (b, m)
        if "cand" in claim:
            assert [(k, LC.block_col(b) + jr) for k, jr in enumerate(claim["cand"])] == m["cand"], b
        assert LC.cells_of_block(o["edge_cell"], b) == m["edge_cells"] and LC.cells_of_block(o["surf_cell"], b) == m["surf_cells"], b
        if m["num"] >= 25:
            assert LC.margin_failures(m) == [], b
        edge_cells += m["edge_cells"]
        surf_cells += m["surf_cells"]
        if "tie" in claim:          # two columns of one line with the same Laplacian, bit for bit: the first is the candidate
            k, first, later = claim["tie"]
            assert m["g1"][k, first] == m["g1"][k, later] > LC.G1_THRES and (k, LC.block_col(b) + first) in m["cand"]
        if "rivals" in claim:       # the later column larger by a margin: it is the candidate
            k, first, later = claim["rivals"]
            assert m["g1"][k, later] - m["g1"][k, first] >= 1e-6 * m["g1"][k, later] and m["g1"][k, first] > LC.G1_THRES
            assert (k, LC.block_col(b) + later) in m["cand"]
        if claim.get("coplanar"):   # ev0 is rounding noise, ev1 is not
            assert abs(m["ev"][0]) < 1e-12 * m["ev"][1]
    # nothing else is emitted: the columns in front of the first block and behind the last one belong to no block
    assert edge_cells == [int(c) for c in o["edge_cell"]] and surf_cells == [int(c) for c in o["surf_cell"]]
    for cells in (o["edge_cell"], o["surf_cell"]):
        col = np.asarray(cells) % LC.COLS
        assert ((col >= 5) & (col <= 3988)).all()


def test_constructed_cases_cover_the_branches(oracle):
    cases = {c["name"]: c for c in LC.constructed_cases()}
    claims = [cl for c in cases.values() for cl in c["designed"].values()]
    assert {cl["num"] for cl in cases["occupancy"]["designed"].values()} == {24, 25, 26, 36}
    for ne in (3, 4, 5, 6):
        assert any(cl["ne"] == ne for cl in claims)
    assert {(cl["edge"], cl["surf"]) for cl in cases["edges"]["designed"].values() if cl["ne"] > 3} == {(True, True), (True, False), (False, True), (False, False)}
    assert 0 in cases["edges"]["designed"] and 663 in cases["edges"]["designed"]
    # the border columns are filled, and the first and last block's candidates reach into them
    o, xyz, curv, dep = _walk(oracle, cases["edges"])
    assert (o["cell_src"][:, :5] >= 0).all() and (o["cell_src"][:, 3989:] >= 0).all()
    # the occupancy grid's 24-cell blocks stand where the grid before it emits edges and planes
    order = [c["name"] for c in LC.constructed_cases()]
    assert order.index("occupancy") == order.index("edges") + 1
    for b, cl in cases["occupancy"]["designed"].items():
        if cl["num"] == 24:
            assert cases["edges"]["designed"][b]["edge"] and cases["edges"]["designed"][b]["surf"]
    # the empty cells of the 24 / 25 / 26 blocks: lane 0, the last lane, a whole line
    _, _, curv, _ = _walk(oracle, cases["occupancy"])
    for num in (24, 25, 26):
        seen = set()
        for b, cl in cases["occupancy"]["designed"].items():
            if cl["num"] != num or b == 663:
                continue
            v = ~(curv[:, LC.block_col(b):LC.block_col(b) + 6] <= 0)      # [line, jr]
            seen |= {"lane0"} if not v[0, 0] else set()
            seen |= {"last"} if not v[5, 5] else set()
            seen |= {"line"} if (~v).all(axis=1).any() else set()
        assert seen == {"lane0", "last", "line"}, num


def test_first_writer_decides(oracle):
    """Had the later of each pair won its cell, the block would not be a plane: the model says so on the grid with the pairs swapped."""
    case, swapped = LC.case_first_writer(), LC.case_first_writer(later_first=True)
    o = oracle.extract_livox(case["rows"])
    _, xyz, curv, dep = _walk(oracle, swapped)
    for b, _ in LC.FIRST_WRITER:
        m = LC.block_model(xyz, curv, dep, b)
        assert (m["num"], m["ne"], m["emit_surf"]) == (36, 1, False) and LC.margin_failures(m) == []
        assert len(LC.cells_of_block(o["surf_cell"], b)) == 36
    # in the case itself the later row of every pair is in the cut cloud and owns no cell
    cl = case["rows"][:, 3]
    vals, cnt = np.unique(cl, return_counts=True)
    twice = vals[cnt == 2]
    assert twice.shape[0] == len(LC.FIRST_WRITER)
    for v in twice:
        first, later = np.nonzero(cl == v)[0]
        assert first in o["cell_src"] and later not in o["cell_src"] and later in o["cut_src"]


def test_scan_cases_are_where_they_claim(oracle):
    S = LC.scan_cases()
    res = {}
    for name, rows in S.items():
        o = oracle.extract_livox(rows, LC.Q_SCAN)
        _, curv = LC.grid_of(rows, o)
        res[name] = (o, LC.occupancy(curv))
    o, num = res["thin70"]
    assert (num < 25).sum() > 100 and (num == 24).sum() > 20 and (num == 25).sum() > 20 and (num > 25).sum() > 100
    assert len(res["head5000"][0]["surf"]) > 1000 and len(res["every_third"][0]["surf"]) == 0 and len(res["every_third"][0]["edge"]) == 0
    assert S["triple"].shape[0] > 65536 + 256 and len(res["triple"][0]["edge"]) > 5      # more than 256 workgroups of 256 points
    n = S["triple"].shape[0] // 3
    assert (res["triple"][0]["cell_src"] < n).all()
    for m in (1, 255, 256, 257):
        assert S["n%d" % m].shape[0] == m == len(res["n%d" % m][0]["cutted"])
    o, _ = res["hole"]
    assert not ((o["cut_src"] >= 512) & (o["cut_src"] < 1024)).any() and (o["cut_src"] >= 1024).any() and len(o["surf"]) > 5000
    o, _ = res["all_dropped"]
    assert S["all_dropped"].shape[0] == 3000 and len(o["cutted"]) == 0 and (o["cell_src"] == -1).all()


def test_prep_rows_are_where_they_claim(oracle):
    rows, at = LC.prep_rows()
    t = rows[:, 3]
    for name, q in LC.PREP_Q.items():
        o = oracle.extract_livox(rows, q)
        cut, grid = set(o["cut_src"].tolist()), set(o["cell_src"][o["cell_src"] >= 0].tolist())
        r = at["intensity"]
        # NaN, +inf, 3e9 (no int holds them: the reference's conversion gives INT_MIN), -1.5 and 6.0 are dropped; -0.5 is line 0 with a negative column
        assert [x in cut for x in r] == [False, False, False, False, True, True, False, True, True, True, True, True, True], name
        assert [x in grid for x in r] == [False, False, False, False, False, True, False, True, True, False, False, False, False], name
        assert o["cell_src"][5, 3995] == r[5] and o["cell_src"][0, 3999] == r[7] and o["cell_src"][2, 3999] == r[8]      # 5.0999; 0.1 and 2.1000001: clamped, column 3999
        # either side of k + 0.5: the two neighbours land in columns k and k + 1
        for (line, k), lo, hi in zip(LC.PREP_COLUMN_LINES, at["half_column"][0::2], at["half_column"][1::2]):
            assert o["cell_src"][line, k] == lo and o["cell_src"][line, k + 1] == hi, (name, line, k)
        for line, rs in zip((1, 4), (at["column_3999"][:3], at["column_3999"][3:])):
            assert o["cell_src"][line, 3999] == rs[0], name                # the first of the three owns column 3999, the others are in the cut cloud only
            assert all(x in cut for x in rs)
        # curvature: float32(0.05) and the value below float32(25.45) pass, their outer neighbours do not; NaN passes every comparison
        c = at["curvature"]
        assert [x in grid for x in c] == [False, True, True, True, False, False, True], name
        assert all(x in cut for x in c)
        # squared range: both sides of 4.0 and of 40000.0 occur
        rg = at["range"]
        assert all(x in cut for x in rg)
        assert {x in grid for x in rg[:8]} == {True, False} and {x in grid for x in rg[8:]} == {True, False}, name
    assert np.isnan(t[at["intensity"][0]]) and LC.PREP_Q["negated"][0] < 0 and abs(LC.PREP_Q["linear"][0]) >= 1 - 2.3e-16
    assert abs(LC.PREP_Q["three_rad"][0]) < 0.1 and abs(np.linalg.norm(LC.PREP_Q["three_rad"]) - 1) < 1e-15
