"""The Livox Horizon extractor on the device against the oracle on the cases of tests/livox_cases.py — the branches of k_livox_prep, k_livox_cut_grid, k_livox_blocks
and k_livox_compact that no scan of synth.make_livox_scan reaches (tests/test_livox_cases_cpu.py holds, on the oracle alone, that every case is where it
claims to be and away from every threshold).  The comparison is the one of tests/test_extract_livox_gpu.py: cut_src, cell_src, edge_cell and surf_cell equal,
payloads bit-exact, stored normals / directions within 2e-6."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import livox_cases as LC

pytestmark = pytest.mark.gpu


def test_constructed_grids_in_one_context(gpu_ctx, oracle):
    """Occupancy 24 / 25 / 26 / 36, planes on either side of surf_thres, candidates on 3 .. 6 lines, edges with and without a plane, ties, the border blocks, first writer
    wins — one extractor, one grid after another: the 24-cell blocks follow a grid that emitted edges and planes in their place (a per-block count left behind by the
    early return would show), and an empty scan stands between two grids (the re-arm of the ownership table)."""
    ex = L.LivoxExtractor(gpu_ctx)
    for case in LC.constructed_cases():
        g = ex.extract(case["rows"], debug=True)
        o = oracle.extract_livox(case["rows"])
        print(case["name"], g["cutted"].shape[0], g["edge"].shape[0], g["surf"].shape[0], "oracle", o["cutted"].shape[0], o["edge"].shape[0], o["surf"].shape[0])
        LC.check(g, o)


def test_scan_level_cases(gpu_ctx, oracle):
    """A thinned scan (blocks at 24 and 25 cells by the dozen), the sparser scans, the scan three times over (290 workgroups: the second trip of the cut's count loop),
    n = 1, 255, 256, 257, two workgroups without a kept point in the middle of a scan, a scan whose every point is dropped."""
    ex = L.LivoxExtractor(gpu_ctx)
    for name, rows in LC.scan_cases().items():
        g = ex.extract(rows, LC.Q_SCAN, debug=True)
        o = oracle.extract_livox(rows, LC.Q_SCAN)
        print(name, rows.shape[0], g["cutted"].shape[0], g["edge"].shape[0], g["surf"].shape[0], "oracle", o["cutted"].shape[0], o["edge"].shape[0], o["surf"].shape[0])
        LC.check(g, o)


@pytest.mark.parametrize("q_name", list(LC.PREP_Q))
def test_prep_stage_rows(gpu_ctx, oracle, q_name):
    """Intensities no line id holds (NaN, +inf, 3e9), negative and too large lines, fractions at and beyond 0.1 (ratio clamp, column >= 4000), columns at k + 0.5 and
    at 3999, squared ranges and curvatures on either side of their limits, NaN curvature — under a quaternion with w < 0, one in the slerp's linear branch with a
    vector part, the identity and an angle of 3 rad."""
    rows, at = LC.prep_rows()
    ex = L.LivoxExtractor(gpu_ctx)
    q = LC.PREP_Q[q_name]
    g = ex.extract(rows, q, debug=True)
    o = oracle.extract_livox(rows, q)
    nan_row = at["intensity"][0]
    print(q_name, "n_cut", g["cutted"].shape[0], "oracle", o["cutted"].shape[0], "NaN-intensity row in cut_src:", bool((g["cut_src"] == nan_row).any()),
          "owner of cell (0, 0):", int(g["cell_src"][0, 0]), "oracle", int(o["cell_src"][0, 0]))
    LC.check(g, o)
    if q_name == "negated":      # q and -q are the same rotation: every output bit-identical
        p = ex.extract(rows, LC.PREP_Q["scan"], debug=True)
        for k in g:
            assert np.array_equal(g[k].view(np.uint32) if g[k].dtype == np.float32 else g[k], p[k].view(np.uint32) if p[k].dtype == np.float32 else p[k]), k
