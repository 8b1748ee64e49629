"""Cases that take the Livox Horizon extractor (lili_extract_livox.hip) through the branches no synthetic scan reaches: blocks at the occupancy limit
(24 / 25 / 26 of 36 cells), planes on either side of surf_thres, edge candidates on 3 .. 6 lines (collinear and scattered), edges without a plane and
with one (tombstones), ties for the largest Laplacian, the first and the last block, first-writer-wins at chosen stream distances, scans that are thin,
tiny, tripled or dropped altogether, and the prep stage's filters at their limits under the quaternions the slerp branches on.

Shared by tests/test_livox_cases_cpu.py (the conditions on the inputs, on the oracle alone) and tests/test_livox_branches_gpu.py (the device against the
oracle).  Referee: oracle.extract_livox.  block_model is a numpy f64 restatement of ONE block (L/src/Preprocessing.cpp:270-383) whose only purpose is to
say in which branch a case is and by what margin.

Geometry of a constructed block b (columns i .. i + 5, i = 5 + 6 b; the sensor at the origin looks along +x):
  wall   cell (line k, column i + jr) -> (depth + noise * s, 0.05 (jr - 2.5), 0.05 (k - 2.5)),  s = (-1)^(jr + k): a plane across the line of sight
  graze  cell -> (x, 0.2 x + noise * s, 0.05 (k - 2.5)),  x = depth + 0.05 (jr - 2.5): a plane along the line of sight — a step in depth stays IN the plane
A `near` cell has depth 8 instead of 10: its Laplacian is (8 * 10 - 8 * 8) / 64 = 0.25 > 0.06, every other cell's is negative or noise / depth.
Designed blocks stand three apart with four context columns on either side (the reach of the Laplacian): the blocks in between hold 24 cells and emit nothing."""
import functools

import numpy as np

from lili_om_amd import synth

LINES, COLS, BLOCKS = 6, 4000, 664
T_INTERVAL = 0.1 / (COLS - 1)
SURF_THRES, EDGE_THRES = 0.28, 4.0          # L/config/config_fr_iosb.yaml:5-6, the extractor's defaults
G1_THRES = 0.06
IDENTITY = (1.0, 0.0, 0.0, 0.0)
EMPTY = np.zeros((0, 5), np.float32)


def check(g, o):
    assert np.array_equal(g["cut_src"], o["cut_src"])
    assert np.array_equal(g["cutted"].view(np.uint32), o["cutted"].view(np.uint32))
    assert np.array_equal(g["cell_src"], o["cell_src"])
    assert np.array_equal(g["edge_cell"], o["edge_cell"])
    assert np.array_equal(g["surf_cell"], o["surf_cell"])
    for k in ("edge", "surf"):
        a, b = g[k], o[k]
        assert a.shape == b.shape
        assert np.array_equal(a[:, [0, 1, 2, 6, 7]].view(np.uint32), b[:, [0, 1, 2, 6, 7]].view(np.uint32))
        np.testing.assert_allclose(a[:, 3:6], b[:, 3:6], rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------------------
# grid builder
# ------------------------------------------------------------------------------------------------
def column_of(intensity, line):
    """L:262 on float32 intensities (line = int(intensity))."""
    frac = (np.asarray(intensity, np.float32) - np.asarray(line, np.float32)).astype(np.float64)
    q = frac / T_INTERVAL
    return (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(np.int64)          # round(): halves away from zero


def grid_rows(cells):
    """cells: (line, col, x, y, z, curvature) in STREAM order (duplicates of a cell, and which of them comes first, are the caller's).
    -> (n, 5) float32 rows, intensity = float32(line + col * 0.1 / 3999); every row lands in the cell asked for."""
    c = np.asarray(cells, np.float64).reshape(-1, 6)
    line, col = c[:, 0].astype(np.int64), c[:, 1].astype(np.int64)
    assert ((0 <= line) & (line < LINES) & (0 <= col) & (col < COLS)).all()
    rows = np.empty((c.shape[0], 5), np.float32)
    rows[:, :3] = c[:, 2:5]
    rows[:, 3] = (line + col * 0.1 / (COLS - 1)).astype(np.float32)
    rows[:, 4] = c[:, 5]
    assert np.array_equal(rows[:, 3].astype(np.int64), line) and np.array_equal(column_of(rows[:, 3], line), col)
    return rows


def block_col(b):
    return 5 + 6 * b


def lane(jr, k):
    """Lane of k_livox_blocks that owns cell (line k, column i + jr): the order in which the reference visits the 36 cells."""
    return 6 * jr + k


def _point(plane, k, jr, depth, noise):
    s = 1.0 if (jr + k) % 2 == 0 else -1.0
    if plane == "wall":
        return depth + noise * s, 0.05 * (jr - 2.5), 0.05 * (k - 2.5)
    if plane == "graze":
        x = depth + 0.05 * (jr - 2.5)
        return x, 0.2 * x + noise * s, 0.05 * (k - 2.5)
    if plane == "coplanar":      # dyadic coordinates on the plane x = 10 + y / 4: exact in float32, ev0 is the f64 sums' rounding noise
        y = (jr - 2.5) / 16.0
        return depth + 0.25 * y, y, (k - 2.5) / 16.0
    raise ValueError(plane)


def patch(b, plane="wall", noise=0.01, absent=(), near=None, ctx=(4, 4), depth=10.0, near_depth=8.0, curv=1.0, override=None):
    """Cells of block b in (column, line) order, with ctx = (left, right) context columns.  absent: lanes left empty.  near: {line: jr} cells at
    near_depth.  override: {(line, jr): (x, y, z)}."""
    i = block_col(b)
    near, override, absent = near or {}, override or {}, set(absent)
    out = []
    for jr in range(-ctx[0], 6 + ctx[1]):
        for k in range(LINES):
            if 0 <= jr < 6 and lane(jr, k) in absent:
                continue
            p = _point(plane, k, jr, near_depth if near.get(k) == jr else depth, noise)
            p = override.get((k, jr), p)
            out.append((k, i + jr, p[0], p[1], p[2], curv))
    return out


def absent_lanes(n_absent, must=(), whole_line=None, avoid=()):
    """n_absent lanes of a block: `must`, all of `whole_line`, the rest drawn from the others (never from `avoid`)."""
    lanes = list(must) + ([lane(jr, whole_line) for jr in range(6)] if whole_line is not None else [])
    rng = np.random.default_rng(1000 + 37 * n_absent + len(lanes))
    pool = [int(x) for x in rng.permutation(36) if x not in lanes and x not in avoid and (whole_line is None or x % 6 != whole_line)]
    lanes += pool[:n_absent - len(lanes)]
    assert len(set(lanes)) == n_absent
    return tuple(sorted(lanes))


def border_fill(left=True, right=True):
    """Wall cells in columns 0 .. 4 and 3989 .. 3999: they belong to no block."""
    cols = (list(range(0, 5)) if left else []) + (list(range(3989, COLS)) if right else [])
    return [(k, c, 10.0, 0.05 * ((c % 6) - 2.5), 0.05 * (k - 2.5), 1.0) for c in cols for k in range(LINES)]


# ------------------------------------------------------------------------------------------------
# numpy f64 model of one block, L:270-383
# ------------------------------------------------------------------------------------------------
def grid_of(rows, o):
    """The reference's mat[][] after L:243-268, from the oracle's cell_src / cutted: xyz (6, 4000, 3) float32 and curvature (6, 4000) float32, 0 = empty."""
    inv = np.full(max(rows.shape[0], 1), -1, np.int64)
    inv[o["cut_src"]] = np.arange(o["cut_src"].shape[0])
    src = o["cell_src"]
    xyz = np.zeros((LINES, COLS, 3), np.float32)
    curv = np.zeros((LINES, COLS), np.float32)
    m = src >= 0
    cut = o["cutted"][inv[src[m]]]
    xyz[m] = cut[:, :3]
    curv[m] = cut[:, 7]
    return xyz, curv


def depth_grid(xyz):
    """getDepth per cell: float32 products, sums and square root, widened (L:100-102 on float members)."""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    d = np.sqrt((x * x + y * y) + z * z)
    assert d.dtype == np.float32
    return d.astype(np.float64)


def occupancy(curv):
    """num of all 664 blocks."""
    v = ~(curv[:, 5:5 + 6 * BLOCKS] <= 0)
    return v.reshape(LINES, BLOCKS, 6).sum(axis=(0, 2))


def block_model(xyz, curv, dep, b, surf_thres=SURF_THRES, edge_thres=EDGE_THRES):
    i = block_col(b)
    valid = ~(curv[:, i:i + 6] <= 0)                       # [line, jr]; a NaN curvature counts, as in the reference
    num = int(valid.sum())
    m = dict(b=b, num=num, valid=valid, g1=None, ne=0, cand=[], ev=None, eve=None, emit_edge=False, emit_surf=False, edge_cells=[], surf_cells=[])
    if num < 25:
        return m
    P = xyz[:, i:i + 6].astype(np.float64)
    order = [(jr, k) for jr in range(6) for k in range(LINES) if valid[k, jr]]
    c = np.zeros(3)
    for jr, k in order:
        c = c + P[k, jr]
    c = c / num
    A = np.zeros((3, 3))
    for jr, k in order:
        z = P[k, jr] - c
        A = A + np.outer(z, z)
    m["ev"] = np.linalg.eigvalsh(A)
    g1 = np.full((LINES, 6), np.nan)
    for k in range(LINES):
        max_s, idx = 0.0, i
        for jr in range(6):
            if not valid[k, jr]:
                continue
            d = dep[k, i + jr - 4:i + jr + 5]
            g = d[0] + d[1] + d[2] + d[3] - 8 * d[4] + d[5] + d[6] + d[7] + d[8]
            g = g / (8 * d[4] + 1e-3)
            g1[k, jr] = g
            if g > G1_THRES and g > max_s:
                max_s, idx = g, i + jr
        if max_s != 0:
            m["cand"].append((k, idx))
    m["g1"] = g1
    ne = m["ne"] = len(m["cand"])
    if ne > 0:
        ce = np.zeros(3)
        for k, col in m["cand"]:
            ce = ce + xyz[k, col].astype(np.float64)
        ce = ce / ne
        AE = np.zeros((3, 3))
        for k, col in m["cand"]:
            z = xyz[k, col].astype(np.float64) - ce
            AE = AE + np.outer(z, z)
        m["eve"] = np.linalg.eigvalsh(AE)
        m["emit_edge"] = bool(ne > 3 and m["eve"][2] > edge_thres * m["eve"][1])
    m["emit_surf"] = bool(m["ev"][0] < surf_thres * m["ev"][1])
    tomb = set()
    if m["emit_edge"]:
        m["edge_cells"] = [k * COLS + col for k, col in m["cand"]]
        tomb = set(m["edge_cells"])
    if m["emit_surf"]:
        m["surf_cells"] = [k * COLS + i + jr for jr, k in order if k * COLS + i + jr not in tomb]
    return m


def cells_of_block(cells, b):
    """The entries of an emitted cell list (edge_cell / surf_cell of the oracle or the device) that lie in block b, in list order."""
    col = np.asarray(cells) % COLS
    i = block_col(b)
    return [int(c) for c in np.asarray(cells)[(col >= i) & (col < i + 6)]]


def margin_failures(m, surf_thres=SURF_THRES, edge_thres=EDGE_THRES):
    """The conditions of tests/test_livox_cases_cpu.py on one modelled block with num >= 25; returns the list of those it misses."""
    bad = []
    ev, eve = m["ev"], m["eve"]
    # ev0 / ev1 a factor 1.05 from surf_thres (ev0 may be rounding noise of either sign: then only ev1 > 0 matters)
    if m["emit_surf"]:
        if not (ev[1] > 0 and 1.05 * ev[0] <= surf_thres * ev[1]):
            bad.append(("surf_thres", ev))
        if not (ev[1] - ev[0] >= 1e-3 * ev[2]):
            bad.append(("normal separation", ev))
    elif not (ev[0] >= 1.05 * surf_thres * ev[1]):
        bad.append(("surf_thres", ev))
    if m["ne"] > 3:
        if m["emit_edge"]:
            if not (eve[2] >= 1.05 * edge_thres * abs(eve[1])):
                bad.append(("edge_thres", eve))
            if not (eve[2] - eve[1] >= 1e-3 * eve[2]):
                bad.append(("direction separation", eve))
        elif not (1.05 * eve[2] <= edge_thres * eve[1]):
            bad.append(("edge_thres", eve))
    g = m["g1"][m["valid"]]
    if not (np.abs(g - G1_THRES) >= 1e-3).all():
        bad.append(("g1 threshold", g))
    for k in range(LINES):      # rival maxima of a line: bit-equal or apart by a relative 1e-6
        gk = np.sort(m["g1"][k][m["valid"][k] & (m["g1"][k] > G1_THRES)])[::-1]
        if gk.shape[0] > 1 and gk[0] != gk[1] and not (gk[0] - gk[1] >= 1e-6 * gk[0]):
            bad.append(("rival maxima", k, gk))
    return bad


# ------------------------------------------------------------------------------------------------
# constructed grids.  A case: dict(name, rows, q_imu, designed = {block: what the case claims about it})
# claim: num, ne, edge (emitted), surf (emitted) and, where it matters, cand = the candidate columns (jr) per line
# ------------------------------------------------------------------------------------------------
ALL_LINES = (0, 1, 2, 3, 4, 5)


def _near(lines, jr):
    jrs = jr if isinstance(jr, (tuple, list)) else [jr] * len(lines)
    return dict(zip(lines, jrs))


def _tie_override(later_gain=0.0):
    """Line 2 of a wall block whose candidates sit at jr = 1: its depths repeat with period 3 over the columns jr = -3 .. 8 (only the sign of y differs from
    one period to the next, which no float32 product sees), so the Laplacians of jr = 1 and jr = 4 are the same sums of the same numbers: bit-identical.
    later_gain > 0 brings the point at jr = 4 closer by that fraction: then the later column is the larger one."""
    base = {0: (10.0, 0.125, -0.025), 1: (8.0, 0.075, -0.025), 2: (10.2, 0.1, -0.025)}
    ov = {}
    for jr in range(-3, 9):
        x, y, z = base[jr % 3]
        if jr == 4:
            x = x * (1.0 - later_gain)
        ov[(2, jr)] = (x, y if (jr // 3) % 2 else -y, z)
    return ov


def case_wall_all():
    cells = border_fill()
    for b in range(BLOCKS):
        cells += patch(b, ctx=(0, 0))
    claim = dict(num=36, ne=0, edge=False, surf=True)
    return dict(name="wall_all", rows=grid_rows(sorted(cells, key=lambda c: (c[1], c[0]))), designed={b: claim for b in range(BLOCKS)})


def case_edges():
    """Edge candidates on 3 .. 6 lines, collinear and scattered, with and without a plane; ties; candidates with empty neighbours; the two border blocks."""
    D, cells = {}, border_fill()

    def add(b, claim, **kw):
        cells.extend(patch(b, **kw))
        D[b] = claim

    # edges AND a plane (graze): the surf list lacks exactly the tombstoned cells.  Block 0's candidates sit in its first column: their Laplacians reach column 1
    add(0, dict(num=36, ne=6, edge=True, surf=True, cand=[0] * 6), plane="graze", near=_near(ALL_LINES, 0))
    add(3, dict(num=36, ne=4, edge=True, surf=True), plane="graze", near=_near((0, 2, 3, 5), 2))
    add(6, dict(num=36, ne=5, edge=True, surf=True), plane="graze", near=_near((0, 1, 2, 4, 5), 3))
    add(9, dict(num=36, ne=3, edge=False, surf=True), plane="graze", near=_near((1, 3, 4), 2))              # three collinear candidates: no edge, all 36 cells in the plane
    # edges and NO plane (wall with a step across it)
    add(12, dict(num=36, ne=6, edge=True, surf=False), near=_near(ALL_LINES, 2))
    add(15, dict(num=36, ne=4, edge=True, surf=False), near=_near((1, 2, 3, 4), 3))
    add(18, dict(num=36, ne=5, edge=True, surf=False), near=_near((0, 1, 3, 4, 5), 2))
    add(21, dict(num=36, ne=3, edge=False, surf=False), near=_near((0, 2, 5), 2))
    # scattered candidates: ne > 3, the ratio test fails
    add(24, dict(num=36, ne=6, edge=False, surf=False), near=_near(ALL_LINES, (0, 5, 0, 5, 0, 5)))
    add(27, dict(num=36, ne=4, edge=False, surf=True), plane="graze", near=_near((0, 2, 3, 5), (0, 5, 5, 0)))
    # ties for the largest Laplacian of line 2
    add(30, dict(num=36, ne=6, edge=True, surf=False, cand=[1, 1, 1, 1, 1, 1], tie=(2, 1, 4)), near=_near(ALL_LINES, 1), override=_tie_override())
    add(33, dict(num=36, ne=6, edge=True, surf=False, cand=[4, 4, 4, 4, 4, 4], rivals=(2, 1, 4)), near=_near(ALL_LINES, 4), override=_tie_override(1e-3))
    # candidates with empty neighbours (depth 0): a whole column of the block empty two columns behind them; the cell four columns in front of them empty
    add(36, dict(num=30, ne=6, edge=True, surf=False), near=_near(ALL_LINES, 2), absent=[lane(4, k) for k in range(LINES)])
    add(39, dict(num=36, ne=6, edge=True, surf=False), near=_near(ALL_LINES, 0), ctx=(3, 4))
    # the last block: candidates in its last column, their Laplacians reach column 3992
    add(663, dict(num=36, ne=6, edge=True, surf=True, cand=[5] * 6), plane="graze", near=_near(ALL_LINES, 5))
    return dict(name="edges", rows=grid_rows(cells), designed=D)


def case_occupancy():
    """Planar blocks with 24 (nothing emitted), 25, 26 and 36 cells; the empty cells include lane 0 / the last lane / a whole line.  The 24-cell blocks stand where
    case_edges emits edges and planes: run behind it, a count left over from the scan before shows."""
    D, cells = {}, border_fill()
    b = 0
    for num in (24, 25, 26):
        for kw in (dict(must=(0,), avoid=(35,)), dict(must=(35,), avoid=(0,)), dict(whole_line=2, avoid=(0, 35))):
            cells += patch(b, absent=absent_lanes(36 - num, **kw))
            D[b] = dict(num=num, ne=0, edge=False, surf=num >= 25)
            b += 3
    cells += patch(b)
    D[b] = dict(num=36, ne=0, edge=False, surf=True)
    cells += patch(663, absent=absent_lanes(11, must=(0, 35)))
    D[663] = dict(num=25, ne=0, edge=False, surf=True)
    return dict(name="occupancy", rows=grid_rows(cells), designed=D)


def case_plane():
    """Planes on either side of surf_thres (the wall's roughness decides) and an exactly coplanar block."""
    D, cells = {}, []
    for b, noise, surf in ((0, 0.01, True), (3, 0.04, True), (6, 0.055, False), (9, 0.2, False)):
        cells += patch(b, noise=noise)
        D[b] = dict(num=36, ne=0, edge=False, surf=surf)
    cells += patch(12, plane="coplanar", depth=float(np.float32(10.3)), absent=(7, 20, 30))      # (no symmetry: the centre is a rounded quotient)
    D[12] = dict(num=33, ne=0, edge=False, surf=True, coplanar=True)
    return dict(name="plane", rows=grid_rows(cells), designed=D)


FIRST_WRITER = ((2, 20500), (40, 1), (80, 255), (120, 256), (160, 257))   # (block whose first cell is written twice, distance in the stream)


def case_first_writer(later_first=False):
    """The full wall with five cells written twice, the second time 1, 255, 256, 257 and > 20 000 rows later by a point 6 m off the wall: it must lose, and the
    block stays a plane.  later_first = True swaps each pair — what the grid would be had the later point won: the model then says `no plane`."""
    cells = sorted(case_wall_all_cells(), key=lambda c: (c[1], c[0]))
    pairs = []
    for b, dist in (FIRST_WRITER[:1] + FIRST_WRITER[:0:-1]):      # the far pair first, the others from the back: no insertion moves a pair apart that is already in place
        i = block_col(b)
        idx = next(r for r in range(len(cells)) if i <= cells[r][1] < i + 6)
        first = cells[idx]
        dup = (first[0], first[1], 4.0, first[3], first[4], first[5])
        cells.insert(idx + dist, first if later_first else dup)
        if later_first:
            cells[idx] = dup
        pairs.append((first[0], first[1], dist))
    rows = grid_rows(cells)
    cl = np.asarray(cells)[:, :2].astype(np.int64)
    for k, col, dist in pairs:      # the distances asked for are the distances in the stream
        at = np.nonzero((cl[:, 0] == k) & (cl[:, 1] == col))[0]
        assert at.shape[0] == 2 and (at[1] - at[0] == dist if dist < 20000 else at[1] - at[0] > 20000), (k, col, dist, at)
    claim = dict(num=36, ne=0, edge=False, surf=True)
    D = {b: claim for b in range(BLOCKS)}
    if later_first:
        for b, _ in FIRST_WRITER:
            D[b] = dict(num=36, ne=1, edge=False, surf=False)
    return dict(name="first_writer_swapped" if later_first else "first_writer", rows=rows, designed=D)


def case_wall_all_cells():
    cells = border_fill()
    for b in range(BLOCKS):
        cells += patch(b, ctx=(0, 0))
    return cells


@functools.lru_cache(maxsize=None)
def constructed_cases():
    """In the order the device test runs them in one context: the occupancy grid behind the edge grid (stale per-block counts), the empty scan between two."""
    return (case_wall_all(), case_edges(), case_occupancy(), dict(name="empty", rows=EMPTY, designed={}), case_plane(), case_first_writer())


# ------------------------------------------------------------------------------------------------
# scan-level cases (synth.make_livox_scan)
# ------------------------------------------------------------------------------------------------
Q_SCAN = (np.cos(0.01), 0.6 * np.sin(0.01), -0.3 * np.sin(0.01), 0.74 * np.sin(0.01))          # the quaternion of test_livox_extractor_parity


@functools.lru_cache(maxsize=None)
def scan_cases():
    scan = synth.make_livox_scan(11)
    n = scan.shape[0]
    out = {}
    keep = np.random.default_rng(70).random(n) < 0.7
    out["thin70"] = scan[keep]
    out["head5000"] = scan[:5000]
    out["every_third"] = scan[::3]
    out["triple"] = np.concatenate([scan, scan, scan])
    for m in (1, 255, 256, 257):
        out["n%d" % m] = scan[30:30 + m]
    hole = scan.copy()
    hole[512:768, 0] = np.nan           # two whole workgroups of k_livox_prep without a kept point, in the middle of the scan
    hole[768:1024, 3] = 7.0
    out["hole"] = hole
    gone = scan[:3000].copy()
    gone[:, 3] += 6.0                   # a non-empty scan, every point dropped
    out["all_dropped"] = gone
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------
# prep-stage rows mixed into a normal scan
# ------------------------------------------------------------------------------------------------
def _f32_neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def _around(target):
    """The float32 values on either side of a float64 target."""
    lo = np.float32(target)
    if float(lo) > target:
        lo = np.nextafter(lo, np.float32(-np.inf))
    return [lo, np.nextafter(lo, np.float32(np.inf))]


PREP_INTENSITIES = [np.float32(np.nan), np.float32(np.inf), np.float32(3e9), np.float32(-1.5), np.float32(-0.5), np.float32(5.0999), np.float32(6.0),
                    # fraction at or beyond 0.1: the ratio clamp applies; a column of 4000 or more is dropped
                    np.float32(0.1), np.nextafter(np.float32(2.1), np.float32(np.inf)), np.float32(2.10002), np.float32(2.5), np.float32(3.9999), np.float32(4.25)]
PREP_COLUMN_LINES = ((0, 100), (2, 103), (1, 1234), (3, 2000), (5, 3997), (5, 170))          # (line, k): col at k + 0.5 as closely as float32 allows
PREP_Q = {
    "scan": Q_SCAN,
    "negated": tuple(-v for v in Q_SCAN),                 # b.w < 0: every output bit-identical to "scan"
    "linear": (1.0, 1e-9, -2e-9, 1e-9),                  # |w| >= 1 - eps with a vector part
    "identity": IDENTITY,
    "three_rad": (np.cos(1.5), 0.6 * np.sin(1.5), -0.3 * np.sin(1.5), np.sqrt(1 - 0.36 - 0.09) * np.sin(1.5)),
}


@functools.lru_cache(maxsize=None)
def prep_rows():
    """-> (rows, at): a scan with the crafted rows written over every third of its first rows (so that each of them is the first writer of the cell
    it lands in); at = {what: row indices}."""
    scan = synth.make_livox_scan(3).copy()
    at, nxt = {}, [20]

    def put(what, **f):
        r = nxt[0]
        while not (np.isfinite(scan[r]).all() and 5.0 < float((scan[r, :3].astype(np.float64) ** 2).sum()) < 30000.0 and 0.1 < scan[r, 4] < 25.0):
            r += 1      # (a row that passes every filter as it is)
        nxt[0] = r + 3
        for col, v in f.items():
            scan[r, {"x": 0, "y": 1, "z": 2, "i": 3, "c": 4}[col]] = v
        at.setdefault(what, []).append(r)

    for v in PREP_INTENSITIES:
        put("intensity", i=v)
    for line, k in PREP_COLUMN_LINES:
        for v in _around(line + (k + 0.5) * T_INTERVAL):
            put("half_column", i=v)
    for line in (1, 4):
        for v in _f32_neighbours(line + 0.1):
            put("column_3999", i=v)
    d = np.array([0.6, -0.64, 0.48])                     # a unit vector
    for r2 in (4.0, 40000.0):
        for v in (-1e-6, -2e-7, 0.0, 2e-7, 1e-6):
            p = d * np.sqrt(r2) * (1.0 + v)
            put("range", x=p[0], y=p[1], z=p[2])
        for v in _f32_neighbours(np.sqrt(r2)):           # on the axis: the squared range is 4.0 / 40000.0 itself or its neighbour
            put("range", x=v, y=0.0, z=0.0)
    for c in (0.05, 25.45):
        for v in _f32_neighbours(c):
            put("curvature", c=v)
    put("curvature", c=np.float32(np.nan))
    return np.ascontiguousarray(scan, np.float32), at
