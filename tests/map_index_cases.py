"""Designed clouds for the map index build (lili_map_set: k_cell_count, k_cell_count_narrow, k_scan_lookback_t, the three-kernel scan, k_scatter_t,
k_rowtot9, k_start9, k_scatter9), one family per size at which a kernel changes behaviour.  tests/test_map_index_cases_cpu.py proves that every case
reaches its designed cell count, box, largest occupancy, scan tile count and stretch count; tests/test_map_index_gpu.py builds each on the device and
compares the index read back by lili_map_debug_index with tests/map_index_model.py, cell by cell.

Every case is a few hundred to a few thousand points.  A point at the origin and one at (d - 1) * cell + cell / 2 along each axis pin the measured box, so
the grid has exactly the designed d cells per axis; the other points sit near the centres of designed cells (+- 0.3 cell), so their cells do not depend on
rounding — except in the `faces` family, which is about exactly that."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from tests import dense_grid_model as G

# count table and scan of a build: the options a case is built under
COMBOS = {"narrow_lookback": dict(map_narrow_counts=1, scan_lookback=1),
          "wide_lookback": dict(map_narrow_counts=0, scan_lookback=1),
          "wide_three_kernel": dict(map_narrow_counts=0, scan_lookback=0)}
ALL = tuple(COMBOS)
WIDE = ("wide_lookback", "wide_three_kernel")

NONFINITE = [tuple(v if k == j else 1.0 for k in range(3)) for j in range(3) for v in (np.nan, np.inf, -np.inf)]      # NaN, +inf, -inf in each coordinate


@dataclass
class Case:
    name: str
    family: str
    points: np.ndarray                 # (n, 3) f32, or (n, 4) with the auxiliary float in column 3
    dims: tuple                        # designed (nx, ny, nz)
    msr: float = 1.0                   # max_sq_radius of the build (the gate)
    cells: np.ndarray = None           # designed cell of every point (None: the model decides — the faces family)
    max_occ: int = None                # designed largest cell occupancy (None: as `cells` gives it)
    tiles: tuple = None                # designed (look-back tiles, three-kernel tiles) of the cell array (None: not part of the design)
    box: tuple = None                  # designed (bx0, by0, bz0, bnx, bny, bnz) (None: the whole grid)
    stretches: int = None              # designed stretch count of the super-row copy (None: derived from the box)
    spw: int = 1                       # designed stretches per wave
    row_tiles: int = None              # designed look-back tiles of the super-row totals (None: not part of the design)
    both_start9_branches: bool = False  # k_start9 must meet all-empty and populated stretches
    combos: tuple = ALL
    options: dict = field(default_factory=dict)      # further context options of the build
    focus: tuple = None                # (centre, radius) for lili_map_focus
    variant: str = "frontend"          # "livox": the cloud carries the auxiliary float
    probes: list = None                # faces: (row, axis, face, side) — side -1 must fall into cell face - 1, side +1 into cell face

    @property
    def n(self):
        return self.points.shape[0]

    @property
    def n_cells(self):
        return self.dims[0] * self.dims[1] * self.dims[2]


def cell_edge(msr):
    return G.gate_cell(msr)


def corners(dims, cell):
    """the two points that pin the box: the origin and (d - 1) * cell + cell / 2 along each axis"""
    return np.array([[0.0, 0.0, 0.0], [(d - 1) * cell + cell / 2 for d in dims]], np.float64)


def unravel(c, dims):
    c = np.asarray(c, np.int64)
    return np.stack([c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])], 1)


def ravel(xyz, dims):
    xyz = np.asarray(xyz, np.int64)
    return (xyz[:, 2] * dims[1] + xyz[:, 1]) * dims[0] + xyz[:, 0]


def points_in(cells, dims, cell, rng):
    """one point near the centre of every listed (linear) cell"""
    xyz = unravel(cells, dims).astype(np.float64)
    return (xyz + 0.5 + rng.uniform(-0.3, 0.3, xyz.shape)) * cell


def with_corners(inner_cells, dims, msr, rng, aux=False):
    """[origin, points of inner_cells in the order given, far corner] as f32 and the designed cell of each"""
    cell = cell_edge(msr)
    co = corners(dims, cell)
    inner_cells = np.asarray(inner_cells, np.int64)
    pts = np.concatenate([co[:1], points_in(inner_cells, dims, cell, rng), co[1:]]).astype(np.float32)
    cells = np.concatenate([[0], inner_cells, [dims[0] * dims[1] * dims[2] - 1]]).astype(np.int64)
    if aux:
        pts = np.concatenate([pts, (100.0 + 0.01 * np.arange(pts.shape[0]))[:, None].astype(np.float32)], 1)
    return np.ascontiguousarray(pts), cells


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# scan tiles: k_scan_lookback_t (tiles of 16384, look-back trips of 64 tiles), k_scan_block_sums / k_scan_sums / k_scan_apply (tiles of 2048)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
#            n_cells: (dims, (look-back tiles, three-kernel tiles), gate)
SCAN_SIZES = {1: ((1, 1, 1), (1, 1), 1.0), 2: ((2, 1, 1), (1, 1), 1.0),
              2047: ((23, 89, 1), (1, 1), 1.0), 2048: ((64, 32, 1), (1, 1), 1.0), 2049: ((3, 683, 1), (1, 2), 1.0),
              16383: ((127, 43, 3), (1, 8), 1.0), 16384: ((128, 128, 1), (1, 8), 1.0), 16385: ((113, 29, 5), (2, 9), 1.0),
              32767: ((7, 31, 151), (2, 16), 1.0), 32768: ((32, 32, 32), (2, 16), 1.0), 32769: ((33, 331, 3), (3, 17), 1.0),
              # more than 64 tiles: a look-back of the last tiles takes a second (third) trip of 64 predecessors if the nearer ones have no prefix yet
              1048575: ((1025, 1023, 1), (64, 512), 0.01), 1048577: ((17, 61681, 1), (65, 513), 0.01), 1064960: ((1040, 1024, 1), (65, 520), 0.01),
              1064961: ((27, 39443, 1), (66, 521), 0.01), 2113537: ((181, 11677, 1), (130, 1033), 0.01)}


def _scan_case(n_cells):
    dims, tiles, msr = SCAN_SIZES[n_cells]
    rng = np.random.default_rng(n_cells)
    want = {0, n_cells - 1}
    for tile in (2048, 16384):
        for e in range(tile, n_cells, tile):      # both sides of every tile edge
            want |= {e - 1, e}
    if n_cells > 2:
        want |= set(int(v) for v in rng.integers(0, n_cells, 24))
    want = np.array(sorted(want), np.int64)
    # 5 or 6 points per cell (prefixes that are not the cell numbers; every point has its five nearest inside the gate, in its own cell and, where the two cells at
    # a tile edge are neighbours in x, across the edge); the largest grids keep that for the edges of the look-back tiles and put one point at the others
    many = (n_cells < 100000) | ((want + 1) % 16384 < 2)
    inner = np.repeat(want, np.where(many, 5 + want % 2, 1))
    inner = inner[rng.permutation(inner.size)]
    pts, cells = with_corners(inner, dims, msr, rng)
    return Case(f"scan_{n_cells}", "scan", pts, dims, msr=msr, cells=cells, tiles=tiles)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# count pass: k_cell_count (lanes of one cell share an atomic), k_cell_count_narrow (lanes of one table word do), k_scatter_t (eight slabs of workgroups)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
COUNT_DIMS = (64, 2, 2)            # 256 cells = 64 words of the narrow table; the far corner sits in the last one
COUNT_N = (1, 63, 64, 65, 255, 256, 257, 1792, 2047, 2048, 2049, 2055)      # partial last waves and workgroups; 1, 7, 8, 9 workgroups (the scatter launches 8, 8, 8, 16)


def _order_cells(order, m, rng):
    """designed cells of the m points between the corners; no cell gets more than 255 (the narrow table stays narrow: the 256-point case is its own)"""
    i = np.arange(m, dtype=np.int64)
    if order == "one_cell":            # every lane of a wave in one cell, wave after wave (a new cell, in another word, every 255 points)
        return 5 + 4 * (i // 255)
    if order == "two_alternating":     # no two neighbouring lanes share a cell; the two cells share a table word (even blocks) or not (odd blocks)
        j = i // 510
        return np.where(i & 1, np.where(j & 1, 8 * j + 5, 8 * j + 3), 8 * j + 2)
    if order == "word_cycle":          # the four cells of one table word, cycled: one narrow atomic per wave carries four counts
        return 4 * (3 + i // 1020) + (i & 3)
    if order == "wave_runs":           # runs of 48: every other run crosses a wave boundary
        return ((i // 48) * 5) % 251 + 1
    if order == "voxel":               # long runs in ascending cell order, as a voxel-filtered map arrives
        return 1 + i // 100
    if order == "random":
        return rng.integers(0, 256, m)
    raise ValueError(order)


ORDERS = ("one_cell", "two_alternating", "word_cycle", "wave_runs", "voxel", "random")


def _count_case(n, order):
    rng = np.random.default_rng(1000 * n + ORDERS.index(order))
    if n == 1:
        return Case(f"count_{n}_{order}", "count", np.zeros((1, 3), np.float32), (1, 1, 1), cells=np.zeros(1, np.int64), combos=("narrow_lookback", "wide_lookback"))
    pts, cells = with_corners(_order_cells(order, n - 2, rng), COUNT_DIMS, 1.0, rng)
    return Case(f"count_{n}_{order}", "count", pts, COUNT_DIMS, cells=cells, combos=("narrow_lookback", "wide_lookback"))


def _occupancy_case(occ):
    """cell 42 (word 10, byte 2) holds exactly `occ` points that arrive in three pieces from different waves and workgroups; its neighbour in the word, cell 43,
    holds exactly 3"""
    rng = np.random.default_rng(occ)
    x, nb = 42, 43
    filler = lambda k: rng.choice(np.r_[1:40, 44:250], k)      # noqa: E731
    inner = np.concatenate([np.full(100, x), [nb], np.full(100, x), [nb], filler(30), np.full(occ - 200, x), [nb], filler(30)])
    pts, cells = with_corners(inner, COUNT_DIMS, 1.0, rng)
    return Case(f"occupancy_{occ}", "occupancy", pts, COUNT_DIMS, cells=cells, max_occ=occ, combos=("narrow_lookback",))


def _one_cell_wide():
    """2053 points in one cell: ranks far beyond a byte, 32-bit table only"""
    rng = np.random.default_rng(7)
    pts, cells = with_corners(np.full(2053, 5), COUNT_DIMS, 1.0, rng)
    return Case("count_2055_one_cell_wide", "count", pts, COUNT_DIMS, cells=cells, max_occ=2053, combos=WIDE)


def _nonfinite_case():
    dims = (8, 4, 2)
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, 64, 120), np.concatenate([rng.integers(0, 64, 90), np.zeros(6, np.int64)])      # cell 0 also holds finite points
    pts, cells = with_corners(np.concatenate([a, b]), dims, 1.0, rng)
    bad = np.array(NONFINITE, np.float32)
    cut = 1 + a.size
    pts = np.concatenate([bad, pts[:cut], bad, pts[cut:], bad])          # head, middle and tail of the cloud
    cells = np.concatenate([np.zeros(9, np.int64), cells[:cut], np.zeros(9, np.int64), cells[cut:], np.zeros(9, np.int64)])
    return Case("nonfinite", "nonfinite", np.ascontiguousarray(pts), dims, cells=cells, combos=("narrow_lookback", "wide_lookback"))


def _no_finite_case():
    bad = np.array(NONFINITE + [(np.nan, np.nan, np.nan)], np.float32)
    pts = np.ascontiguousarray(bad[np.arange(70) % bad.shape[0]])
    return Case("no_finite_point", "nonfinite", pts, (1, 1, 1), cells=np.zeros(70, np.int64), combos=("narrow_lookback", "wide_lookback"))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# faces: cell_of at coordinates exactly on a cell face and one f32 ulp on either side; the box maximum one ulp below the face that would open a new cell
# ---------------------------------------------------------------------------------------------------------------------------------------------------
FACE_DIMS = (6, 5, 4)


def _faces_case():
    dims, cell = FACE_DIMS, cell_edge(1.0)
    rng = np.random.default_rng(5)
    rows, probes = [[0.0, 0.0, 0.0]], []
    for k in range(3):
        for i in range(1, dims[k]):
            f = np.float32(float(i) * cell)
            for side, v in ((-1, np.nextafter(f, np.float32(-np.inf))), (0, f), (1, np.nextafter(f, np.float32(np.inf)))):
                p = (rng.integers(0, dims) + 0.5 + rng.uniform(-0.3, 0.3, 3)) * cell
                p[k] = float(v)
                probes.append((len(rows), k, i, side))
                rows.append(list(p))
    far = [float(np.nextafter(np.float32(float(d) * cell), np.float32(0))) for d in dims]
    while any(f >= float(d) * cell for f, d in zip(far, dims)):          # strictly below the face in f64 as well
        far = [float(np.nextafter(np.float32(f), np.float32(0))) for f in far]
    rows.append(far)
    return Case("faces", "faces", np.ascontiguousarray(np.array(rows, np.float32)), dims, probes=probes, combos=("narrow_lookback", "wide_lookback"))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# super-rows: k_rowtot9, the look-back scan of the row totals, k_start9 (64 cells x 32 rows per workgroup, a shortcut for empty stretches), k_scatter9
# ---------------------------------------------------------------------------------------------------------------------------------------------------
SUPER_DIMS = [(1, 1, 1), (1, 7, 5), (63, 31, 1), (64, 8, 4), (65, 9, 3), (128, 32, 3), (129, 33, 5), (65, 1, 4), (64, 7, 3), (63, 8, 5), (128, 9, 1), (129, 31, 4),
              (65, 32, 1), (1, 33, 3)]


def _sparse_rows(dims, rng, n_blob=220):
    """populated rows next to stretches whose 30 source rows are all empty: the four edge rows of the grid (their source rows fall outside it), a blob in the low
    corner, and nothing else"""
    nx, ny, nz = dims
    edge = [(rng.integers(0, nx), y, z) for y in (0, ny - 1) for z in (0, nz - 1) for _ in range(6)]
    blob = np.stack([rng.integers(0, nx, n_blob), rng.integers(0, max(1, ny // 4), n_blob), rng.integers(0, max(1, nz // 2), n_blob)], 1)
    inner = ravel(np.concatenate([np.array(edge, np.int64).reshape(-1, 3), blob]), dims)
    return inner[rng.permutation(inner.size)]


def _super_case(dims, aux=False, options=None, name=None):
    rng = np.random.default_rng(dims[0] * 10007 + dims[1] * 101 + dims[2])
    pts, cells = with_corners(_sparse_rows(dims, rng), dims, 1.0, rng, aux=aux)
    return Case(name or "super_%dx%dx%d" % dims, "super", pts, dims, cells=cells, both_start9_branches=dims[1] >= 31 and dims[2] >= 3,
                combos=("narrow_lookback",), options=options or {}, variant="livox" if aux else "frontend")


#                 dims: (row-total tiles, stretches, spw)
ROW_SCAN = {(1, 127, 129): (1, 16383, 1), (1, 128, 128): (1, 16384, 1), (1, 113, 145): (2, 16385, 1),
            (1, 511, 513): (16, 262143, 1), (1, 512, 512): (16, 262144, 2), (1, 1024, 512): (32, 524288, 4)}


def _row_scan_case(dims):
    row_tiles, n_str, spw = ROW_SCAN[dims]
    rng = np.random.default_rng(n_str)
    rows = dims[1] * dims[2]
    want = {0, rows - 1} | {e + s for e in range(16384, rows, 16384) for s in (-1, 0)} | set(int(v) for v in rng.integers(0, rows, 150))
    inner = np.array(sorted(want), np.int64)
    inner = np.repeat(inner, 5 + inner % 2)          # (neighbouring rows are neighbouring cells: five nearest across the edges of the row-total tiles)
    pts, cells = with_corners(inner[rng.permutation(inner.size)], dims, 0.01, rng)
    return Case("rows_%dx%dx%d" % dims, "super", pts, dims, msr=0.01, cells=cells, stretches=n_str, spw=spw, row_tiles=row_tiles, both_start9_branches=True,
                tiles=((rows + 16383) // 16384, (rows + 2047) // 2048), combos=("narrow_lookback",))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# focus box: build_grid's b0 / b1 arithmetic, box-relative prefixes in k_rowtot9 / k_start9 / k_scatter9 (bx0 > 0)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
FOCUS_DIMS = (40, 30, 6)
#        name: (centre in cells, radius in cells, designed box)
FOCUS = {"inside_below_a_cell": ((20.5, 15.5, 3.5), 0.4, (18, 13, 1, 5, 5, 5)),
         "inside_r3": ((20.5, 15.5, 3.5), 3.0, (15, 10, 0, 11, 11, 6)),
         "inside_r12": ((20.5, 15.5, 3.5), 12.0, (6, 1, 0, 29, 29, 6)),
         "inside_above_the_map": ((20.5, 15.5, 3.5), 100.0, (0, 0, 0, 40, 30, 6)),
         "on_a_face": ((10.0, 15.5, 3.5), 0.4, (7, 13, 1, 6, 5, 5)),
         "outside_r3": ((-8.0, 15.5, 3.5), 3.0, (0, 10, 0, 1, 11, 6)),
         "outside_r12": ((-8.0, 15.5, 3.5), 12.3, (0, 1, 0, 7, 29, 6)),
         "far_outside": ((200.0, 200.0, 200.0), 3.0, (39, 29, 5, 1, 1, 1))}


def _focus_case(name):
    centre, radius, box = FOCUS[name]
    cell = cell_edge(1.0)
    rng = np.random.default_rng(40)              # the same cloud for every focus
    pts, cells = with_corners(rng.integers(0, 40 * 30 * 6, 600), FOCUS_DIMS, 1.0, rng)
    return Case("focus_" + name, "focus", pts, FOCUS_DIMS, cells=cells, box=box, focus=(tuple(v * cell for v in centre), radius * cell), combos=("narrow_lookback",))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# where the box comes from, the cell cap, the fine index, the layouts
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _plain_case(name, dims, n, seed, aux=False, options=None, family="box"):
    rng = np.random.default_rng(seed)
    pts, cells = with_corners(rng.integers(0, dims[0] * dims[1] * dims[2], n), dims, 1.0, rng, aux=aux)
    return Case(name, family, pts, dims, cells=cells, combos=("narrow_lookback",), options=options or {}, variant="livox" if aux else "frontend")


MAX_CELLS_CAP = 500          # below the 2000 cells the cloud of `max_cells` needs at the gate's edge


def blob(n=3000, seed=3):
    """a small dense blob: ~15 points per gate-sized cell, far above fine_occupancy 2 and far below 256"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.uniform(0.0, 1.0, (n, 3)) * np.array([4.0, 4.0, 2.0]) + np.array([3.0, -2.0, 1.0])).astype(np.float32))


@lru_cache(maxsize=None)
def cases():
    out = [_scan_case(n) for n in SCAN_SIZES]
    out += [_count_case(n, o) for n in COUNT_N for o in (ORDERS if n > 1 else ORDERS[:1])]
    out += [_one_cell_wide(), _occupancy_case(255), _occupancy_case(256), _nonfinite_case(), _no_finite_case(), _faces_case()]
    out += [_super_case(d) for d in SUPER_DIMS]
    out += [_super_case((65, 9, 4), aux=True, name="super_aux"), _super_case((65, 9, 4), options={"super_rows": 0}, name="super_rows_off")]
    out += [_row_scan_case(d) for d in ROW_SCAN]
    out += [_focus_case(k) for k in FOCUS]
    out += [_plain_case("box_sources", (30, 20, 4), 700, 21), _plain_case("max_cells", (20, 20, 5), 500, 22, options={"max_cells": MAX_CELLS_CAP}),
            _plain_case("layouts", (20, 12, 3), 900, 23, aux=True, family="layouts")]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


def names(family=None, exclude=()):
    return [k for k, c in cases().items() if (family is None or c.family == family) and c.family not in exclude]
