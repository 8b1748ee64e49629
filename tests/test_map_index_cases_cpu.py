"""The designed clouds of tests/map_index_cases.py reach what they were designed for: under the plain model of the build (tests/map_index_model.py, the grid
of tests/dense_grid_model.py) every case has its designed cell count and box, its designed largest cell occupancy, its designed number of scan tiles and
stretches — and the model's own super-row arithmetic is consistent.  No GPU: tests/test_map_index_gpu.py compares the device's index with the same model."""
import numpy as np
import pytest

from tests import dense_grid_model as G
from tests import map_index_cases as Cs
from tests import map_index_model as M


def _model(c, margin_cells=0.0):
    return M.index_of(c.points, c.msr, max_cells=c.options.get("max_cells", G.MAX_CELLS), focus=c.focus, margin_cells=margin_cells)


@pytest.mark.parametrize("name", Cs.names(exclude=("faces",)))
def test_case_reaches_its_design(name):
    c = Cs.cases()[name]
    assert 1 <= c.n <= 4096
    I = _model(c)
    if name == "max_cells":          # the designed grid is what the cap leaves of the (20, 20, 5) the gate asks for
        assert G.build_grid(*G.box_of(c.points), Cs.cell_edge(c.msr)).n_cells == 2000 > Cs.MAX_CELLS_CAP
        assert I.g.cell_used > Cs.cell_edge(c.msr) and I.g.n_cells <= Cs.MAX_CELLS_CAP
        assert I.dims == (12, 12, 3), I.dims          # two trips through the coarsening loop: (13, 13, 3) = 507 cells after the first
        return
    assert I.dims == c.dims and I.g.n_cells == c.n_cells
    assert np.array_equal(I.cells, c.cells)                                   # every point in its designed cell
    whole = (0, 0, 0) + c.dims
    assert I.box == (c.box or whole)
    assert I.hist.max() == (c.max_occ if c.max_occ is not None else np.bincount(c.cells).max())
    assert I.hist.max() <= 255 or name in ("occupancy_256", "count_2055_one_cell_wide")
    assert c.tiles is None or (M.scan_tiles(I.g.n_cells, True), M.scan_tiles(I.g.n_cells, False)) == c.tiles
    n_str, spw = M.stretches(I.box)
    assert n_str == (c.stretches if c.stretches is not None else ((I.box[3] + 63) // 64) * I.box[4] * I.box[5])
    assert spw == c.spw
    assert c.row_tiles is None or M.scan_tiles(I.box[4] * I.box[5], True) == c.row_tiles
    # the first and the last cell are populated (the corners), cell_start ends with n
    assert I.hist[0] >= 1 and I.hist[-1] >= 1 and I.cell_start[-1] == c.n and I.cell_start[0] == 0
    if c.both_start9_branches:
        empty, occupied = M.start9_branches(I.cell_start, I.dims, I.box)
        assert empty > 0 and occupied > 0, (empty, occupied)


def test_scan_family_sits_on_every_tile_edge():
    for n_cells, (dims, tiles, msr) in Cs.SCAN_SIZES.items():
        c = Cs.cases()[f"scan_{n_cells}"]
        assert dims[0] * dims[1] * dims[2] == n_cells
        hist = _model(c).hist
        for tile in (M.S3_TILE, M.LB_TILE):
            for e in range(tile, n_cells, tile):
                assert hist[e - 1] >= 1 and hist[e] >= 1, (n_cells, e)
    assert {1, 2, 2047, 2048, 2049, 16383, 16384, 16385, 32767, 32768, 32769, 64 * 16384 - 1, 64 * 16384 + 1, 65 * 16384 + 1, 129 * 16384 + 1} <= set(Cs.SCAN_SIZES)


def test_search_check_has_something_to_check():
    """the GPU test compares the 5-NN of every self-query whose fifth neighbour lies inside the gate: such queries exist where a search can go wrong"""
    from tests.knn_brute import BruteKnn5

    def inside(c):
        _, d = BruteKnn5(c.points).query(c.points, reach=1.01 * np.sqrt(c.msr))
        return d[:, 4] < c.msr
    for n_cells in Cs.SCAN_SIZES:
        c = Cs.cases()[f"scan_{n_cells}"]
        ok = inside(c)
        if n_cells >= 2047:
            for e in range(16384 if n_cells > 100000 else 2048, n_cells, 16384 if n_cells > 100000 else 2048):      # on both sides of the tile edges
                assert ok[c.cells == e - 1].any() or ok[c.cells == e].any(), (n_cells, e)
    for name in Cs.names("super") + Cs.names("focus") + Cs.names("count"):
        c = Cs.cases()[name]
        assert inside(c).sum() >= (5 if c.n >= 255 else 0), name          # (63 .. 65 random points over 256 cells are too sparse for five within the gate)


def test_count_family_covers_the_wave_and_workgroup_edges():
    assert {1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2055} <= set(Cs.COUNT_N)
    wgs = {(n + 255) // 256 for n in Cs.COUNT_N}
    assert {1, 7, 8, 9} <= wgs
    assert {8 * ((w + 7) // 8) - w for w in wgs} >= {0, 1, 7}          # surplus workgroups of the scatter's eight-slab launch
    c = Cs.cases()["count_2055_two_alternating"]
    assert (np.diff(c.cells[1:-1]) != 0).all()                         # no two neighbouring lanes share a cell
    c = Cs.cases()["count_2055_word_cycle"]
    assert np.array_equal(c.cells[1:65] >> 2, np.full(64, 3)) and set(c.cells[1:65] & 3) == {0, 1, 2, 3}
    c = Cs.cases()["count_2055_wave_runs"]
    heads = np.nonzero(np.diff(c.cells) != 0)[0] + 1
    assert ((heads % 64) != 0).any() and (np.diff(heads)[1:-1] == 48).all()
    for occ in (255, 256):
        c = Cs.cases()[f"occupancy_{occ}"]
        h = _model(c).hist
        assert h[42] == occ and h[43] == 3 and h.max() == occ
        rows = np.nonzero(c.cells == 42)[0]
        assert len({int(r) // 64 for r in rows}) >= 3 and len({int(r) // 256 for r in rows}) == 2      # several waves, two workgroups


def test_nonfinite_rows_go_to_cell_zero_next_to_finite_points():
    c = Cs.cases()["nonfinite"]
    bad = ~np.isfinite(c.points).all(1)
    assert bad.sum() == 27 and bad[:9].all() and bad[-9:].all() and bad[9:-9].sum() == 9
    for k in range(3):
        col = c.points[bad, k]
        assert np.isnan(col).sum() == 3 and np.isposinf(col).sum() == 3 and np.isneginf(col).sum() == 3
    I = _model(c)
    assert (I.cells[bad] == 0).all() and I.hist[0] > bad.sum()
    c = Cs.cases()["no_finite_point"]
    I = _model(c)
    assert not np.isfinite(c.points).all(1).any() and I.dims == (1, 1, 1) and (I.g.ox, I.g.oy, I.g.oz) == (0.0, 0.0, 0.0) and I.hist[0] == c.n


def test_faces_family_straddles_every_face():
    c = Cs.cases()["faces"]
    I = _model(c)
    assert I.dims == c.dims == Cs.FACE_DIMS
    seen = set()
    for row, k, i, side in c.probes:
        v = float(c.points[row, k])
        assert abs(v - I.g.face(k, i)) <= abs(float(np.spacing(np.float32(v)))) * 1.5
        cc = I.g.cell_coord(c.points[row, k], k)
        if side < 0:
            assert cc == i - 1
        elif side > 0:
            assert cc == i
        else:
            assert cc in (i - 1, i)
        seen.add((k, i, side))
    assert len(seen) == 3 * sum(d - 1 for d in c.dims)
    # the box maximum sits in the last cell without a clamp
    far = c.points[-1]
    assert [I.g.cell_coord(far[k], k) for k in range(3)] == [d - 1 for d in c.dims]
    assert I.cells[-1] == I.g.n_cells - 1


def test_super_family_covers_the_designed_box_sizes():
    dims = [Cs.cases()[n].dims for n in Cs.names("super")]
    assert {d[0] for d in dims} >= {1, 63, 64, 65, 128, 129}
    assert {d[1] for d in dims} >= {1, 7, 8, 9, 31, 32, 33}
    assert {d[2] for d in dims} >= {1, 3, 4, 5}
    assert {d[1] * d[2] for d in dims} >= {16383, 16384, 16385}
    assert {Cs.cases()[n].spw for n in Cs.names("super")} == {1, 2, 4}
    assert {M.stretches((0, 0, 0) + d)[0] for d in dims} >= {262143, 262144, 524288}
    boxes = [Cs.cases()[n].box for n in Cs.names("focus")]
    assert any(b[0] > 0 for b in boxes) and any(b == (0, 0, 0) + Cs.FOCUS_DIMS for b in boxes) and any(b[3:] == (1, 1, 1) for b in boxes)


@pytest.mark.parametrize("dims,box", [((5, 4, 3), (0, 0, 0, 5, 4, 3)), ((7, 6, 5), (2, 1, 1, 3, 4, 3)), ((70, 3, 2), (3, 0, 0, 66, 3, 2)), ((1, 1, 1), (0, 0, 0, 1, 1, 1))])
def test_super_row_model_against_a_cell_by_cell_loop(dims, box):
    """M.super_rows (vectorised) against the definition written as loops"""
    rng = np.random.default_rng(sum(dims))
    nx, ny, nz = dims
    hist = rng.integers(0, 4, nx * ny * nz) * (rng.random(nx * ny * nz) < 0.4)
    cs = M.cell_start(hist)
    n = int(cs[-1])
    start9, gather = M.super_rows(cs, dims, box, n)
    bx0, by0, bz0, bnx, bny, bnz = box
    want_start, want_gather = [], []
    for zs in range(bz0, bz0 + bnz):
        for ys in range(by0, by0 + bny):
            for x in range(bx0, bx0 + bnx):
                want_start.append(n + len(want_gather))
                for k in range(9):
                    y, z = ys + k % 3 - 1, zs + k // 3 - 1
                    if 0 <= y < ny and 0 <= z < nz:
                        c = (z * ny + y) * nx + x
                        want_gather += list(range(int(cs[c]), int(cs[c + 1])))
    want_start.append(n + len(want_gather))
    assert start9.tolist() == want_start and gather.tolist() == want_gather


def test_focus_box_is_the_whole_grid_without_a_focus():
    g = G.build_grid([0.0, 0.0, 0.0], [10.0, 5.0, 2.0], 0.5)
    assert G.focus_box(g) == (0, 0, 0, g.nx, g.ny, g.nz) == G.focus_box(g, (1.0, 1.0, 1.0), 0.0)


def _device_like(c, I, seed=0):
    """a read-back as a correct build would return it, assembled from the model: cells in order, any order inside a cell"""
    import lili_om_amd as L
    rng = np.random.default_rng(seed)
    n = c.n
    order = np.lexsort((rng.random(n), I.cells))
    base = np.zeros((n, 4), np.float32)
    base[:, :3] = c.points[order, :3]
    base[:, 3] = order.astype(np.int32).view(np.float32)
    aux = np.ascontiguousarray(c.points[order, 3]) if c.points.shape[1] > 3 else None
    start9, gather = M.super_rows(I.cell_start, I.dims, I.box, n)
    info = L.api.MapIndexInfo()
    info.nx, info.ny, info.nz = I.dims
    info.bx0, info.by0, info.bz0, info.bnx, info.bny, info.bnz = I.box
    info.n_points, info.reach, info.has_aux, info.has_super, info.narrow = n, G.GRID_REACH, int(aux is not None), 1, 1
    info.ox, info.oy, info.oz, info.inv_cell, info.cell = I.g.ox, I.g.oy, I.g.oz, I.g.inv_cell, I.g.cell
    info.n_cells, info.n_super = I.g.n_cells, gather.size
    return dict(info=info, cell_start=I.cell_start.astype(np.int32), base=base, aux=aux, cell_start9=start9.astype(np.int32), super=base[gather].copy(),
                super_aux=None if aux is None else aux[gather].copy())


def test_the_gpu_tests_checker_rejects_a_subtly_wrong_index():
    """check_index of tests/test_map_index_gpu.py accepts an index assembled from the model and refuses each of the errors the random-query tests would let
    through: a wrong last cell_start word, two points swapped between cells, a point stored twice, one wrong bit in a coordinate or an aux value, a super cell
    that starts one entry late, one mis-copied entry of the super part."""
    from tests.test_map_index_gpu import check_index
    c = Cs.cases()["super_aux"]
    I = _model(c)
    check_index(_device_like(c, I), I, c.points, True, want_narrow=True)
    check_index(_device_like(c, I, seed=5), I, c.points, True, want_narrow=True)          # the order inside a cell is free

    def broken(edit):
        rb = _device_like(c, I)
        edit(rb)
        with pytest.raises(AssertionError):
            check_index(rb, I, c.points, True, want_narrow=True)

    a = int(I.cell_start[np.nonzero(I.hist)[0][3]])          # first position of the fourth populated cell: its predecessor lies in another cell

    def total(rb): rb["cell_start"][-1] -= 1
    def swap(rb): rb["base"][[a - 1, a]] = rb["base"][[a, a - 1]]
    def twice(rb): rb["base"][a] = rb["base"][a - 1]
    def coord(rb): rb["base"][:, 1].view(np.uint32)[a] ^= 1
    def auxbit(rb): rb["aux"].view(np.uint32)[a] ^= 1
    def late(rb): rb["cell_start9"][int(np.nonzero(np.diff(rb["cell_start9"]))[0][2])] += 1
    def miscopy(rb): rb["super"][-1] = rb["super"][0]
    def superaux(rb): rb["super_aux"].view(np.uint32)[7] ^= 1
    def origin(rb): rb["info"].ox = np.nextafter(rb["info"].ox, 1.0)
    def nocopy(rb): rb["info"].has_super = 0
    def wide(rb): rb["info"].narrow = 0
    for edit in (total, swap, twice, coord, auxbit, late, miscopy, superaux, origin, nocopy, wide):
        broken(edit)
