"""The sizing of a dense map's fine index restated in plain Python f64 (lili_map.hip: map_set_impl and build_grid).

Given the map's measured bounding box (its f32 extremes), the gate and the point-weighted mean occupancy of the gate-sized cells that the
count pass reports (lili_map_density), the model returns what lili_map_density reports for the fine index — the fine cell edge and the squared
radius it covers, rounded down to f32 — and the grid itself (origin, inverse cell, cell, cell counts), so that tests can place queries on its
faces.  cbrt comes from the C math library through ctypes: the library's host code calls the same libm."""
import ctypes
import ctypes.util
import math
from dataclasses import dataclass

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cbrt.restype = ctypes.c_double
_libm.cbrt.argtypes = [ctypes.c_double]

MAX_CELLS = 1 << 27          # lili_ctx defaults
FINE_OCCUPANCY = 12
GRID_REACH = 2
CELL_PCT = 65


def cbrt(x):
    return _libm.cbrt(float(x))


@dataclass
class Grid:
    ox: float
    oy: float
    oz: float
    inv_cell: float
    cell: float                  # g.cell = 1 / (1 / c), what the kernels use
    cell_used: float             # the edge after coarsening (lili_map_info / lili_map_density report this one)
    nx: int
    ny: int
    nz: int

    @property
    def n_cells(self):
        return self.nx * self.ny * self.nz

    def cell_coord(self, v, k):
        """cell_coord of lili_s2m_dev.h: floor((v - o) * inv_cell) in f64."""
        o = (self.ox, self.oy, self.oz)[k]
        return math.floor((float(v) - o) * self.inv_cell)

    def face(self, k, i):
        """position of the lower face of cell i along axis k, as the kernels compute it (o + i * cell, f64)."""
        return (self.ox, self.oy, self.oz)[k] + float(i) * self.cell


def gate_cell(max_sq_radius, reach=GRID_REACH, cell_pct=CELL_PCT):
    cell = math.sqrt(max_sq_radius) * 1.01 * ((cell_pct / 100.0) if reach == 2 else 1.0)
    return cell if cell > 1e-6 else 1e-6


def build_grid(mn, mx, cell, max_cells=MAX_CELLS):
    """build_grid's sizing: the coarsening loop, the origin and g.cell = 1 / (1 / c)."""
    while True:
        nx = math.floor((mx[0] - mn[0]) / cell) + 1
        ny = math.floor((mx[1] - mn[1]) / cell) + 1
        nz = math.floor((mx[2] - mn[2]) / cell) + 1
        total = float(nx) * float(ny) * float(nz)
        if total <= float(max_cells):
            break
        cell *= cbrt(total / float(max_cells)) * 1.02
    inv = 1.0 / cell
    return Grid(float(mn[0]), float(mn[1]), float(mn[2]), inv, 1.0 / inv, cell, int(nx), int(ny), int(nz))


def focus_box(g, focus=None, radius=0.0):
    """build_grid's b0 / b1 arithmetic: (bx0, by0, bz0, bnx, bny, bnz), the box of cells that gets super cells — the whole grid, or with lili_map_focus the
    cells within `radius` (+ two cells) of `focus`, clamped into the grid.  The division is by the edge after coarsening, as in the library."""
    dims = (g.nx, g.ny, g.nz)
    b0, b1 = [0, 0, 0], [d - 1 for d in dims]
    if focus is not None and radius > 0:
        mn = (g.ox, g.oy, g.oz)
        for k in range(3):
            lo = (float(focus[k]) - float(radius) - mn[k]) / g.cell_used - 2.0
            hi = (float(focus[k]) + float(radius) - mn[k]) / g.cell_used + 2.0
            b0[k] = int(min(max(math.floor(lo), 0.0), float(dims[k] - 1)))
            b1[k] = int(min(max(math.floor(hi), float(b0[k])), float(dims[k] - 1)))
    return (b0[0], b0[1], b0[2], b1[0] - b0[0] + 1, b1[1] - b0[1] + 1, b1[2] - b0[2] + 1)


def uncoarsened_fine_cell(occ, cell):
    fc = cell * math.sqrt(3.0 / occ)
    return min(max(fc, cell / 16.0), cell / 1.5)


def fbound(fcell_used, reach=GRID_REACH):
    """the squared radius the fine index covers completely, rounded DOWN to f32; also whether the rounding had to step down."""
    rb = float(reach) * fcell_used / 1.01
    exact = rb * rb * (1.0 - 1e-6)
    fb = np.float32(exact)
    stepped = float(fb) > exact
    if stepped:
        fb = np.nextafter(fb, np.float32(0))
    return float(fb), stepped


def box_of(points):
    """the measured box: the f32 extremes of the finite points, as doubles."""
    p = np.asarray(points, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)]
    return [float(v) for v in p.min(0)], [float(v) for v in p.max(0)]


def fine_index(mn, mx, max_sq_radius, occ, max_cells=MAX_CELLS, fine_occupancy=FINE_OCCUPANCY, reach=GRID_REACH, cell_pct=CELL_PCT):
    """(fine Grid or None, fine_cell_edge, fine_sq_radius) as lili_map_density reports them for a measured box and occupancy."""
    cell = gate_cell(max_sq_radius, reach, cell_pct)
    g = build_grid(mn, mx, cell, max_cells)
    if not (occ > float(fine_occupancy) and g.cell_used == cell):      # a gate-sized grid coarsened by max_cells is not refined
        return None, 0.0, 0.0
    fc = uncoarsened_fine_cell(occ, cell)
    fmn = [v - 4.0 * fc for v in mn]
    fmx = [v + 4.0 * fc for v in mx]
    fg = build_grid(fmn, fmx, fc, max_cells)
    fb, _ = fbound(fg.cell_used, reach)
    return fg, fg.cell_used, fb
