"""Invariants of tests/dense_grid_model.py, the f64 restatement of how lili_map_set sizes a dense map's fine index (no GPU).  The GPU tests
(test_dense_map_gpu.py, test_dense_rebuild_gpu.py) hold lili_map_density to this model bit for bit and place queries on its faces."""
import math

import numpy as np
import pytest

from tests import dense_grid_model as M


def test_cbrt_is_the_c_library_one():
    for x in (1.0, 8.0, 27.0, 2.0, 1e-3, 12345.678):
        assert abs(M.cbrt(x) - x ** (1.0 / 3.0)) <= 4e-16 * max(1.0, x ** (1.0 / 3.0))
    assert M.cbrt(64.0) == 4.0 and M.cbrt(-8.0) == -2.0


@pytest.mark.parametrize("seed", range(6))
def test_fbound_is_rounded_down_and_only_shrinks(seed):
    rng = np.random.default_rng(seed)
    stepped = 0
    for fc in rng.uniform(0.02, 0.7, 2000):
        fb, st = M.fbound(fc)
        rb = 2.0 * fc / 1.01
        assert fb <= rb * rb * (1.0 - 1e-6) < rb * rb                  # never above the radius the fine cells cover
        assert float(np.nextafter(np.float32(fb), np.float32(np.inf))) > rb * rb * (1.0 - 1e-6)     # and the largest such f32
        stepped += st
    assert 200 < stepped < 1800                                         # round-to-nearest went up about half of the time


def test_fine_cell_is_clamped_and_coarsening_respects_max_cells():
    cell = M.gate_cell(1.0)
    assert cell == math.sqrt(1.0) * 1.01 * 0.65
    for occ in (13.0, 50.0, 170.0, 1e4, 1e7):
        fc = M.uncoarsened_fine_cell(occ, cell)
        assert cell / 16.0 <= fc <= cell / 1.5
    assert M.uncoarsened_fine_cell(1e7, cell) == cell / 16.0 and M.uncoarsened_fine_cell(2.0, cell) == cell / 1.5
    mn, mx = [-40.0, -30.0, -0.01], [40.0, 30.0, 12.01]
    for max_cells in (1 << 27, 10_000_000, 1_000_000, 50_000, 1000, 7):
        g = M.build_grid(mn, mx, 0.02, max_cells)
        fits = math.prod(math.floor((mx[k] - mn[k]) / 0.02) + 1 for k in range(3)) <= max_cells
        assert g.n_cells <= max_cells
        assert (g.cell_used == 0.02) if fits else (g.cell_used > 0.02)
        assert g.cell == 1.0 / (1.0 / g.cell_used) and abs(g.cell - g.cell_used) <= 1e-15 * g.cell_used
        # the grid covers the box: every extreme falls into a cell of the grid
        for k in range(3):
            assert 0 <= g.cell_coord(mn[k], k) and g.cell_coord(mx[k], k) < (g.nx, g.ny, g.nz)[k]


def test_fine_index_margin_and_bound_shrink_with_coarsening():
    mn, mx = [-6.0, -4.5, 0.0], [6.0, 4.5, 4.0]
    fg, fc, fb = M.fine_index(mn, mx, 1.0, 170.0)
    assert fg is not None and fc == M.uncoarsened_fine_cell(170.0, M.gate_cell(1.0))
    for k in range(3):          # four empty cells of margin on every side
        assert fg.cell_coord(mn[k], k) == 4 and fg.cell_coord(mx[k], k) >= (fg.nx, fg.ny, fg.nz)[k] - 5
    prev_fb = fb
    for max_cells in (fg.n_cells, fg.n_cells - 1, fg.n_cells // 8, 20_000):
        g2, fc2, fb2 = M.fine_index(mn, mx, 1.0, 170.0, max_cells=max_cells)
        if g2 is None:
            assert fc2 == 0.0 and fb2 == 0.0
            continue
        assert g2.n_cells <= max_cells and fc2 >= fc and fb2 >= prev_fb      # coarser fine cells cover more
        prev_fb = fb2
    # a gate-sized grid coarsened by max_cells gets no fine index
    gate = M.build_grid(mn, mx, M.gate_cell(1.0))
    assert M.fine_index(mn, mx, 1.0, 170.0, max_cells=gate.n_cells - 1) == (None, 0.0, 0.0)
    # too sparse
    assert M.fine_index(mn, mx, 1.0, 12.0) == (None, 0.0, 0.0)
