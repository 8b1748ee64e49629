"""The map index of lili_map_set restated in plain numpy f64 (lili_map.hip: build_grid; lili_s2m.hip: k_cell_count*, the scans, k_scatter_t, k_rowtot9, k_start9,
k_scatter9), for tests/test_map_index_gpu.py and tests/test_map_index_cases_cpu.py.

From a source cloud and the grid scalars: the cell of every point (cell_of), the histogram, cell_start, and the per-cell sets of original indices.  From the
device's own base array (the order inside a cell belongs to the count pass's atomics): the super-row arrays — start9 and the gather that the super part must
equal byte for byte.  The grid itself comes from tests/dense_grid_model.py."""
import numpy as np

from tests import dense_grid_model as G

LB_TILE = 16384      # k_scan_lookback_t: cells per workgroup
S3_TILE = 2048       # the three-kernel scan's


def grid_of(points, max_sq_radius, max_cells=G.MAX_CELLS, cell_pct=G.CELL_PCT, reach=G.GRID_REACH, margin_cells=0.0):
    """The gate-sized grid of a build that measures its box (margin_cells 0) or guesses it from that box (0.75 per side); a cloud without a finite point
    gets the one cell at the origin."""
    p = np.asarray(points, np.float32)[:, :3]
    cell = G.gate_cell(max_sq_radius, reach, cell_pct)
    if np.isfinite(p).all(1).any():
        mn, mx = G.box_of(p)
    else:
        mn, mx = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    m = margin_cells * cell
    return G.build_grid([v - m for v in mn], [v + m for v in mx], cell, max_cells)


def cell_of(points, g):
    """cell_of of lili_s2m_dev.h for every point: floor((f64(v) - o) * inv_cell) clamped per axis, x fastest; a non-finite point goes to cell 0."""
    p = np.asarray(points, np.float32)[:, :3]
    finite = np.isfinite(p).all(1)
    c = np.zeros(p.shape[0], np.int64)
    stride = 1
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (o, d) in enumerate(((g.ox, g.nx), (g.oy, g.ny), (g.oz, g.nz))):
            u = np.floor((p[:, k].astype(np.float64) - o) * g.inv_cell)
            u = np.where(finite, np.clip(u, 0.0, float(d - 1)), 0.0)
            c += u.astype(np.int64) * stride
            stride *= d
    return c


def histogram(cells, n_cells):
    return np.bincount(cells, minlength=n_cells).astype(np.int64)


def cell_start(hist):
    """the exclusive cumulative sum with the total at [n_cells]"""
    out = np.zeros(hist.size + 1, np.int64)
    np.cumsum(hist, out=out[1:])
    return out


def canonical(cells, idx):
    """the per-cell SETS of indices as one array: indices ordered by (cell, index).  Two assignments hold the same set in every cell iff these are equal."""
    return np.asarray(idx)[np.lexsort((idx, cells))]


def position_cells(cs):
    """the cell every position of the sorted array belongs to, from a cell_start array"""
    cs = np.asarray(cs, np.int64)
    return np.repeat(np.arange(cs.size - 1, dtype=np.int64), np.diff(cs))


def super_rows(cs, dims, box, n_points):
    """(start9, gather): start9[(x, y', z')] = n_points + the populations of every super cell before it in srow_index order (z' slowest, x fastest, box
    relative), the end of the copy at [bnx * bny * bnz]; gather = the positions of the base array whose entries make up the super part, in order — super cell
    (x, y', z') holds cells (x, y' + dy, z' + dz) in the order k = (dz + 1) * 3 + (dy + 1), each as the base array has it; rows outside the grid give nothing."""
    nx, ny, nz = dims
    bx0, by0, bz0, bnx, bny, bnz = box
    cs = np.asarray(cs, np.int64)
    hist = np.diff(cs).reshape(nz, ny, nx)
    start = cs[:-1].reshape(nz, ny, nx)
    pop = np.zeros((bnz, bny, bnx), np.int64)
    parts = []
    for k in range(9):
        dy, dz = k % 3 - 1, k // 3 - 1
        # super rows (y', z') of the box whose source row (y' + dy, z' + dz) lies in the grid
        y_lo, y_hi = max(by0, -dy), min(by0 + bny, ny - dy)
        z_lo, z_hi = max(bz0, -dz), min(bz0 + bnz, nz - dz)
        if y_lo >= y_hi or z_lo >= z_hi:
            continue
        src = (slice(z_lo + dz, z_hi + dz), slice(y_lo + dy, y_hi + dy), slice(bx0, bx0 + bnx))
        dst = (slice(z_lo - bz0, z_hi - bz0), slice(y_lo - by0, y_hi - by0), slice(None))
        h = hist[src]
        pop[dst] += h
        zz, yy, xx = np.nonzero(h)
        if zz.size:
            s = ((zz + (z_lo - bz0)) * bny + (yy + (y_lo - by0))) * bnx + xx          # srow_index of the super cell
            parts.append(np.stack([s, np.full(s.size, k), start[src][zz, yy, xx], h[zz, yy, xx]], 1))
    start9 = np.zeros(pop.size + 1, np.int64)
    np.cumsum(pop.ravel(), out=start9[1:])
    start9 += n_points
    if parts:
        t = np.concatenate(parts)
        t = t[np.lexsort((t[:, 1], t[:, 0]))]
        cnt = t[:, 3]
        first = np.cumsum(cnt) - cnt
        gather = np.repeat(t[:, 2] - first, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    else:
        gather = np.zeros(0, np.int64)
    assert gather.size == start9[-1] - n_points
    return start9, gather


class Index:
    """what the base part of an index must be: the grid, the box of super cells, every point's cell, the histogram, cell_start and the per-cell sets"""

    def __init__(self, points, g, focus=None):
        self.g = g
        self.dims = (g.nx, g.ny, g.nz)
        self.box = G.focus_box(g, *focus) if focus else G.focus_box(g)
        self.cells = cell_of(points, g)
        self.hist = histogram(self.cells, g.n_cells)
        self.cell_start = cell_start(self.hist)
        self.canonical = canonical(self.cells, np.arange(self.cells.size, dtype=np.int64))
        self.mean_occupancy = 1.0 + 2.0 * float(int((self.hist * (self.hist - 1) // 2).sum())) / float(self.cells.size)      # lili_map_set's: 1 + 2 sum(rank) / n


def index_of(points, max_sq_radius, max_cells=G.MAX_CELLS, focus=None, margin_cells=0.0):
    return Index(points, grid_of(points, max_sq_radius, max_cells=max_cells, margin_cells=margin_cells), focus)


def start9_branches(cs, dims, box):
    """(waves of k_start9 that take the empty-stretch shortcut, waves that take the general branch): a wave serves the stretch of 64 cells at x block bx for
    the 8 super-rows from y0 in plane z' and tests its (8 + 2) x 3 source rows inside the stretch"""
    nx, ny, nz = dims
    bx0, by0, bz0, bnx, bny, bnz = box
    hist = np.diff(np.asarray(cs, np.int64)).reshape(nz, ny, nx)
    empty = occupied = 0
    for zs in range(bz0, bz0 + bnz):
        z_lo, z_hi = max(zs - 1, 0), min(zs + 2, nz)
        for y0 in range(by0, by0 + bny, 8):
            y_lo, y_hi = max(y0 - 1, 0), min(y0 + 9, ny)
            for xa in range(bx0, bx0 + bnx, 64):
                xb = min(xa + 64, bx0 + bnx)
                if hist[z_lo:z_hi, y_lo:y_hi, xa:xb].any():
                    occupied += 1
                else:
                    empty += 1
    return empty, occupied


def scan_tiles(n_items, lookback=True):
    tile = LB_TILE if lookback else S3_TILE
    return (n_items + tile - 1) // tile


def stretches(box):
    """(stretches, spw) of k_scatter9's launch: runs of 64 super cells, and how many of them a wave takes"""
    n_str = ((box[3] + 63) // 64) * box[4] * box[5]
    spw = 1
    while spw < 64 and n_str // (spw * 2) >= 131072:
        spw *= 2
    return n_str, spw
