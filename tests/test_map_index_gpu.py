"""The map index itself, cell by cell: lili_map_set builds the designed clouds of tests/map_index_cases.py, lili_map_debug_index reads the index back, and
every word of it is compared with the plain f64 model of tests/map_index_model.py (grid from tests/dense_grid_model.py).  Integer and bit equality only.

Which kernel and branch each family exists for (all in lili_s2m.hip, launched by build_grid in lili_map.hip):

  scan        k_scan_lookback_t<true> / <false>: the last tile whole, one cell short, one cell over (`whole` and the bounded stores), data[n] from the last tile,
              grids of 64, 65, 66 and 130 tiles where a look-back that meets no prefix among 64 predecessors goes round again; k_scan_block_sums / k_scan_sums /
              k_scan_apply at 2047 .. 2049 cells (one tile, two) and up to 1033 tiles (k_scan_sums' second trip of 256).  Each size under the narrow table + look-back,
              the 32-bit table + look-back and the 32-bit table + three kernels; scan_fallbacks stays 0.
  count       k_cell_count (run heads by cell, one atomic per run) and k_cell_count_narrow (runs by table WORD, four counts per atomic, ranks from ballots): all lanes
              in one cell, no two neighbours alike, the four bytes of one word cycled, runs across wave boundaries, voxel order, random; n at the partial-wave and
              partial-workgroup edges; k_scatter_t's eight-slab order with 0, 1 and 7 surplus workgroups.
  occupancy   k_cell_count_narrow's byte limit: 255 points (from several waves and two workgroups) stay narrow, 256 raise bit 8 of the check word -> the build is
              repeated with k_cell_count and the kind stays wide; the neighbour byte of the same word keeps its 3.
  nonfinite   the isfinite branch of both count kernels and of cell_of (k_scatter_t): NaN, +-inf in each coordinate at head, middle and tail go to cell 0, which
              finite points share; k_bbox_src / decode_box without any finite point.
  faces       cell_coord's f64 floor at coordinates on a face and one f32 ulp either side; the box maximum in the last cell.
  super       k_rowtot9 (rows outside the grid), the look-back scan of the row totals at 16383 / 16384 / 16385 rows, k_start9 (x blocks of 64: 63, 64, 65, 128, 129
              columns; 32 rows per workgroup: 31, 32, 33; the all-empty shortcut next to the general branch), k_scatter9 (tiles of 4 x 4 rows, spw 1 / 2 / 4), the
              auxiliary float, option super_rows 0.
  focus       build_grid's b0 / b1 box and the box-relative prefixes of k_rowtot9 / k_start9 / k_scatter9 (bx0 > 0, box of one cell, whole grid).
  box         measured, guessed (k_cell_count*'s check word) and given boxes, lili_map_set_begin / _end, the max_cells coarsening loop.
  fine        the second build_grid of a dense map: 32-bit counts, four empty cells of margin, its own super-row copy; the dense hint drops the gate-sized copy.
  layouts     load_src: packed xyz, float4, 32-byte rows, float4 rows at a 4-byte aligned address (scalar loads), host memory through the staging copy.
"""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

import lili_om_amd as L
from tests import dense_grid_model as G
from tests import map_index_cases as Cs
from tests import map_index_model as M
from tests.knn_brute import BruteKnn5

pytestmark = pytest.mark.gpu

DEFAULTS = dict(map_narrow_counts=1, scan_lookback=1, super_rows=1, max_cells=G.MAX_CELLS, fine_occupancy=G.FINE_OCCUPANCY, localmap_super_rows=0)
E_ARG, E_STATE = -1, -3
_brute = {}


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    c.set_debug(True)
    yield c
    c.close()


@pytest.fixture
def fresh():
    c = L.Context(0)
    c.set_debug(True)
    yield c
    c.close()


@contextmanager
def options(ctx, m, opts, focus=None, measure=True):
    """the options of one build on the shared context, put back afterwards; measure: forget the previous build's box, so that this one measures its own"""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        if measure:
            ctx.set_option("map_guess_box", 1)          # (setting it clears what the next build would guess from)
        if focus:
            m.map_focus(*focus)
        yield
    finally:
        m.map_focus(None)
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


def matcher(ctx, variant="frontend", msr=1.0):
    return L.ScanToMapMatcher(ctx, L.make_params(variant, kd_max_radius=msr, edge_gate=msr))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def check_scalars(info, I, n, reach=G.GRID_REACH):
    g = I.g
    assert (info.nx, info.ny, info.nz) == I.dims and info.n_cells == g.n_cells
    assert (info.bx0, info.by0, info.bz0, info.bnx, info.bny, info.bnz) == I.box
    got = np.array([info.ox, info.oy, info.oz, info.inv_cell, info.cell], np.float64)
    want = np.array([g.ox, g.oy, g.oz, g.inv_cell, g.cell], np.float64)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert info.n_points == n and info.reach == reach


def check_index(rb, I, src, want_super, want_narrow=None):
    """the read-back `rb` against the model `I` of the cloud `src` ((n, 3), or (n, 4) with the auxiliary float)"""
    info, n = rb["info"], src.shape[0]
    check_scalars(info, I, n)
    if want_narrow is not None:
        assert info.narrow == int(want_narrow)
    has_aux = src.shape[1] > 3
    assert info.has_aux == int(has_aux) and (rb["aux"] is not None) == has_aux
    cs = rb["cell_start"]
    assert np.array_equal(cs, I.cell_start), np.nonzero(cs != I.cell_start)[0][:8]
    assert cs[-1] == n
    base = rb["base"]
    w = base[:, 3].view(np.int32).astype(np.int64)
    assert np.array_equal(np.sort(w), np.arange(n))                                             # a permutation: no point lost, none twice
    assert np.array_equal(M.canonical(M.position_cells(cs), w), I.canonical)                    # every cell holds its own set
    assert np.array_equal(bits(base[:, :3]), bits(src[w, :3]))                                  # and the source's bits
    if has_aux:
        assert np.array_equal(bits(rb["aux"]), bits(src[w, 3]))
    assert info.has_super == int(want_super)
    if not want_super:
        assert info.n_super == 0 and rb["cell_start9"] is None and rb["super"] is None and rb["super_aux"] is None
        return
    start9, gather = M.super_rows(cs, I.dims, I.box, n)
    assert np.array_equal(rb["cell_start9"], start9), np.nonzero(rb["cell_start9"] != start9)[0][:8]
    assert info.n_super == gather.size == rb["super"].shape[0]
    assert np.array_equal(bits(rb["super"]), bits(base[gather]))
    if has_aux:
        assert np.array_equal(bits(rb["super_aux"]), bits(rb["aux"][gather]))


def check_info_call(m, I, n):
    assert m.map_info(L.KIND_SURF) == (n, I.g.n_cells, I.g.cell_used)


def check_search(m, src, msr, key):
    """every map point queried as itself: the five neighbours of every query whose fifth brute-force distance is inside the gate, bit for bit; no other accepted"""
    n = src.shape[0]
    assert n <= 4096
    if key not in _brute:
        _brute[key] = BruteKnn5(src).query(src, reach=1.01 * np.sqrt(msr))
    bi, bd = _brute[key]
    m.set_queries(0, L.KIND_SURF, src)
    m.find_corresponding_surf_features(0, [1.0, 0, 0, 0], [0.0, 0, 0])
    idx, d2 = m.neighbors(0, L.KIND_SURF, n)
    inside = bd[:, 4] < msr
    assert np.array_equal(idx[inside], bi[inside]), np.nonzero((idx != bi).any(1) & inside)[0][:8]
    assert np.array_equal(bits(d2[inside]), bits(bd[inside]))
    assert np.all(~(d2[~inside][:, 4] < msr))
    return int(inside.sum())


def model_of(c, margin_cells=0.0):
    return M.index_of(c.points, c.msr, max_cells=c.options.get("max_cells", G.MAX_CELLS), focus=c.focus, margin_cells=margin_cells)


GENERAL = [n for n in Cs.names() if Cs.cases()[n].family not in ("occupancy", "layouts")]


@pytest.mark.parametrize("name", GENERAL)
def test_index_is_the_models(ctx, name):
    c = Cs.cases()[name]
    m = matcher(ctx, c.variant, c.msr)
    I = model_of(c)
    want_super = bool(c.options.get("super_rows", 1))
    first = None
    for combo in c.combos:
        opts = dict(Cs.COMBOS[combo], **c.options)
        with options(ctx, m, opts, c.focus):
            m.set_input_cloud(L.KIND_SURF, c.points)
            rb = m.map_debug_index(L.KIND_SURF)
            check_index(rb, I, c.points, want_super, want_narrow=combo == "narrow_lookback")
            check_info_call(m, I, c.n)
            if combo == c.combos[0]:                      # the build is repeatable
                ctx.set_option("map_guess_box", 1)
                m.set_input_cloud(L.KIND_SURF, c.points)
                again = m.map_debug_index(L.KIND_SURF)
                assert np.array_equal(again["cell_start"], rb["cell_start"])
                w0, w1 = rb["base"][:, 3].view(np.int32), again["base"][:, 3].view(np.int32)
                assert np.array_equal(M.canonical(M.position_cells(rb["cell_start"]), w0), M.canonical(M.position_cells(again["cell_start"]), w1))
            check_search(m, c.points, c.msr, name)
        info = rb["info"]
        assert info.scan_fallbacks == 0 and m.map_build_stats()[2] == 0
        if first is None:
            first = info.narrow_overflows
        assert info.narrow_overflows == first                # (moves in the 256-point case alone: test_255_points_stay_narrow_256_overflow)
    if name == "super_rows_off":                              # the base arrays are what they are with the copy
        with options(ctx, m, Cs.COMBOS[c.combos[0]]):
            m.set_input_cloud(L.KIND_SURF, c.points)
            on = m.map_debug_index(L.KIND_SURF)
        assert on["info"].has_super == 1 and np.array_equal(on["cell_start"], rb["cell_start"])
        assert np.array_equal(M.canonical(M.position_cells(on["cell_start"]), on["base"][:, 3].view(np.int32)), I.canonical)


def test_255_points_stay_narrow_256_overflow(fresh):
    ctx = fresh
    m = matcher(ctx)
    c255, c256 = Cs.cases()["occupancy_255"], Cs.cases()["occupancy_256"]
    m.set_input_cloud(L.KIND_SURF, c255.points)
    rb = m.map_debug_index(L.KIND_SURF)
    I = model_of(c255)
    check_index(rb, I, c255.points, True, want_narrow=True)
    assert rb["info"].narrow_overflows == 0
    assert np.diff(rb["cell_start"])[42] == 255 and np.diff(rb["cell_start"])[43] == 3
    check_search(m, c255.points, 1.0, "occupancy_255")
    ctx.set_option("map_guess_box", 1)
    m.set_input_cloud(L.KIND_SURF, c256.points)               # one point more: the byte would wrap -> the same call comes back from the 32-bit table
    rb = m.map_debug_index(L.KIND_SURF)
    I = model_of(c256)
    check_index(rb, I, c256.points, True, want_narrow=False)
    assert rb["info"].narrow_overflows == 1
    assert np.diff(rb["cell_start"])[42] == 256 and np.diff(rb["cell_start"])[43] == 3
    check_search(m, c256.points, 1.0, "occupancy_256")
    ctx.set_option("map_guess_box", 1)
    m.set_input_cloud(L.KIND_SURF, c256.points)               # the next build of the kind starts wide: no second overflow
    rb = m.map_debug_index(L.KIND_SURF)
    check_index(rb, I, c256.points, True, want_narrow=False)
    assert rb["info"].narrow_overflows == 1 and rb["info"].scan_fallbacks == 0
    m.set_input_cloud(L.KIND_EDGE, c255.points)               # the other kind is still narrow
    assert m.map_debug_index(L.KIND_EDGE)["info"].narrow == 1


def test_measured_guessed_and_swapped_in_boxes(fresh):
    ctx = fresh
    c = Cs.cases()["box_sources"]
    m = matcher(ctx)
    m.set_input_cloud(L.KIND_SURF, c.points)                  # measured
    assert m.map_build_stats() == (0, 0, 0)
    I0 = model_of(c)
    check_index(m.map_debug_index(L.KIND_SURF), I0, c.points, True, want_narrow=True)
    m.set_input_cloud(L.KIND_SURF, c.points)                  # guessed: the first box minus / plus 0.75 cell per side
    assert m.map_build_stats() == (1, 0, 0)
    I1 = model_of(c, margin_cells=0.75)
    assert I1.dims != I0.dims and I1.g.ox == I0.g.ox - 0.75 * I0.g.cell_used
    check_index(m.map_debug_index(L.KIND_SURF), I1, c.points, True, want_narrow=True)
    check_info_call(m, I1, c.n)
    check_search(m, c.points, c.msr, c.name)
    # the index built on the side stream and swapped in
    other = Cs.cases()["super_129x33x5"]
    ctx.set_option("map_guess_box", 1)
    m.set_input_cloud_begin(L.KIND_SURF, other.points)
    before = m.map_debug_index(L.KIND_SURF)                   # still the current one
    check_index(before, I1, c.points, True)
    m.set_input_cloud_end(L.KIND_SURF)
    check_index(m.map_debug_index(L.KIND_SURF), model_of(other), other.points, True, want_narrow=True)
    check_search(m, other.points, other.msr, other.name)


def test_local_map_commit_builds_on_the_centroids_own_box(fresh):
    ctx = fresh
    ctx.set_option("map_guess_box", 0)                        # a commit that measures must not guess instead
    rng = np.random.default_rng(31)
    lm = L.api.LocalMap(ctx, L.KIND_SURF, 5, 0.4, 1.0)
    m = matcher(ctx, "livox")
    for step in range(2):
        kf = (rng.uniform(0, 1, (1500, 4)) * np.array([10.0, 8.0, 3.0, 50.0]) + np.array([step * 2.0, 0, 0, 100.0])).astype(np.float32)
        lm.push(kf, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
        ctx.set_option("localmap_super_rows", step)           # a small local map goes without the copy unless asked
        try:
            _, n_map = lm.commit()
        finally:
            ctx.set_option("localmap_super_rows", 0)
        cloud = np.ascontiguousarray(lm.get(n_map))
        assert cloud.shape == (n_map, 4) and 500 < n_map <= 4096
        I = M.index_of(cloud, 1.0)
        check_index(m.map_debug_index(L.KIND_SURF), I, cloud, bool(step))
        check_info_call(m, I, n_map)
        check_search(m, cloud, 1.0, ("localmap", step))
    assert lm.stats()[0] >= 1                                 # the second commit merged: its box was handed over, not measured


def test_fine_index_of_a_dense_blob(fresh):
    ctx = fresh
    pts = Cs.blob()
    m = matcher(ctx)
    ctx.set_option("fine_occupancy", 2)
    for build in range(2):
        m.set_input_cloud(L.KIND_SURF, pts)
        assert m.map_build_stats() == (build, 0, 0)           # measured, then guessed from the first box
        I = M.index_of(pts, 1.0, margin_cells=0.75 * build)
        assert 2 < I.mean_occupancy and I.hist.max() <= 255
        occ, fine_cell, fine_r2 = m.map_density(L.KIND_SURF)
        assert occ == I.mean_occupancy
        g = I.g
        fg, fcu, fb = G.fine_index([g.ox, g.oy, g.oz], _box_max(pts, g, build), 1.0, occ, fine_occupancy=2)
        assert fg is not None and (fine_cell, fine_r2) == (fcu, fb)
        # the gate-sized index: with its copy at first; the dense hint of the first build takes the copy away from the second
        check_index(m.map_debug_index(L.KIND_SURF, 0), I, pts, want_super=build == 0, want_narrow=True)
        F = M.Index(pts, fg)
        rb = m.map_debug_index(L.KIND_SURF, 1)
        check_index(rb, F, pts, want_super=True, want_narrow=False)
        # four cells of margin: the origin is the box minimum minus four fine cells (the scalars above, bit for bit), so the outer cells hold nothing; only a point
        # ON a face of the box — (v - o) * inv_cell = 4 or d - 4 up to the last bit — may round into the fourth cell from the edge
        mn, mx = [g.ox, g.oy, g.oz], _box_max(pts, g, build)
        coords = Cs.unravel(F.cells, F.dims)
        for k in range(3):
            v, cc, d = pts[:, k].astype(np.float64), coords[:, k], F.dims[k]
            assert cc.min() >= 3 and cc.max() <= d - 4
            assert (v[cc == 3] == mn[k]).all() and (v[cc == d - 4] == mx[k]).all()
            if build:                                         # (a guessed box has no point on its faces)
                assert cc.min() >= 4 and cc.max() <= d - 5
        assert rb["info"].scan_fallbacks == 0 and rb["info"].narrow_overflows == 0
        check_search(m, pts, 1.0, "blob")


def _box_max(pts, g, build):
    mn, mx = G.box_of(pts)
    return [v + 0.75 * build * g.cell_used for v in mx]


def test_layouts_give_the_same_index(fresh):
    import torch
    ctx = fresh
    c = Cs.cases()["layouts"]
    f4 = c.points
    n = c.n
    xyz = np.ascontiguousarray(f4[:, :3])
    rows32 = np.zeros((n, 8), np.float32)
    rows32[:, :3] = xyz; rows32[:, 4] = f4[:, 3]
    d_f4 = torch.from_numpy(f4).cuda()
    d_rows = torch.from_numpy(rows32).cuda()
    d_odd = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), f4.ravel(), np.zeros(3, np.float32)])).cuda()
    clouds = {"host packed xyz": (L.api.Cloud(xyz.ctypes.data, n, 12, -1, L.api.MEM_HOST), xyz),
              "host float4": (L.api.Cloud(f4.ctypes.data, n, 16, 12, L.api.MEM_HOST), f4),
              "host 32-byte rows, aux at 16": (L.api.Cloud(rows32.ctypes.data, n, 32, 16, L.api.MEM_HOST), f4),
              "device float4": (L.api.cloud_from_device(d_f4.data_ptr(), n, 16, 12), f4),
              "device 32-byte rows": (L.api.cloud_from_device(d_rows.data_ptr(), n, 32, 16), f4),
              "device float4 at a 4-byte aligned address": (L.api.cloud_from_device(d_odd.data_ptr() + 4, n, 16, 12), f4)}
    I = model_of(c)
    sets = {}
    for name, (cloud, src) in clouds.items():
        m = matcher(ctx, "livox" if src.shape[1] > 3 else "frontend")
        ctx.set_option("map_guess_box", 1)
        m.set_input_cloud(L.KIND_SURF, cloud)
        rb = m.map_debug_index(L.KIND_SURF)
        check_index(rb, I, src, True, want_narrow=True)
        sets[name] = M.canonical(M.position_cells(rb["cell_start"]), rb["base"][:, 3].view(np.int32))
        check_search(m, src, c.msr, ("layouts", src.shape[1]))
    for name, s in sets.items():
        assert np.array_equal(s, sets["host float4"]), name


def test_refusals_write_nothing_and_leave_the_context_usable(fresh):
    ctx = fresh
    lib = ctx.lib
    c = Cs.cases()["super_aux"]
    m = matcher(ctx, "livox")
    info = L.api.MapIndexInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    blank = bytes(C.string_at(C.byref(info), C.sizeof(info)))

    def call(h, kind, which, info_p, bufs, caps):
        args = []
        for b, cap in zip(bufs, caps):
            args += [C.c_void_p(b.ctypes.data), cap]
        return lib.lili_map_debug_index(h, kind, which, info_p, *args)

    def sentinels(sizes):
        return [np.full(max(s, 1), 0x5A5A5A5A, np.uint32) for s in sizes]

    def untouched(bufs, info_too=True):
        assert all((b == 0x5A5A5A5A).all() for b in bufs)
        if info_too:
            assert bytes(C.string_at(C.byref(info), C.sizeof(info))) == blank

    bufs = sentinels([64] * 6)
    assert call(ctx.h, L.KIND_SURF, 0, C.byref(info), bufs, [64] * 6) == E_STATE          # no map
    untouched(bufs)
    m.set_input_cloud(L.KIND_SURF, c.points)
    good = m.map_debug_index(L.KIND_SURF)
    gi = good["info"]
    n, n9, nc, nc9 = gi.n_points, gi.n_super, gi.n_cells, gi.bnx * gi.bny * gi.bnz
    need = [nc + 1, n, n, nc9 + 1, n9, n9]
    words = [nc + 1, 4 * n, n, nc9 + 1, 4 * n9, n9]
    bufs = sentinels(words)
    assert call(ctx.h, L.KIND_SURF, 1, C.byref(info), bufs, need) == E_STATE              # no fine index
    assert call(ctx.h, 2, 0, C.byref(info), bufs, need) == E_ARG                           # bad kind
    assert call(ctx.h, -1, 0, C.byref(info), bufs, need) == E_ARG
    assert call(ctx.h, L.KIND_SURF, 2, C.byref(info), bufs, need) == E_ARG                 # bad index
    assert call(ctx.h, L.KIND_EDGE, 0, C.byref(info), bufs, need) == E_STATE               # no map of that kind
    assert call(ctx.h, L.KIND_SURF, 0, None, bufs, need) == E_ARG                          # null info
    assert call(None, L.KIND_SURF, 0, C.byref(info), bufs, need) == E_ARG                  # null context
    untouched(bufs)
    for k in range(6):                                                                     # a capacity one short: the sizes come back, no buffer is written
        caps = list(need)
        caps[k] -= 1
        C.memset(C.byref(info), 0x5A, C.sizeof(info))
        assert call(ctx.h, L.KIND_SURF, 0, C.byref(info), bufs, caps) == E_ARG, k
        untouched(bufs, info_too=False)
        assert (info.n_points, info.n_cells, info.n_super, info.has_aux, info.has_super) == (n, nc, n9, 1, 1)
    # buffers one word longer than needed: the call fills exactly its arrays
    bufs = sentinels([w + 1 for w in words])
    assert call(ctx.h, L.KIND_SURF, 0, C.byref(info), bufs, need) == L.api.OK
    for b, w in zip(bufs, words):
        assert b[w] == 0x5A5A5A5A
    assert np.array_equal(bufs[0][:nc + 1].view(np.int32), good["cell_start"]) and np.array_equal(bufs[1][:4 * n], bits(good["base"]).ravel())
    assert np.array_equal(bufs[4][:4 * n9], bits(good["super"]).ravel()) and np.array_equal(bufs[5][:n9], bits(good["super_aux"]))
    # nothing in the context changed: the same index again, and it still searches and rebuilds
    again = m.map_debug_index(L.KIND_SURF)
    for key in ("cell_start", "base", "aux", "cell_start9", "super", "super_aux"):
        assert np.array_equal(bits(again[key]), bits(good[key])), key
    check_search(m, c.points, c.msr, c.name)
    m.set_input_cloud(L.KIND_SURF, c.points)
    check_index(m.map_debug_index(L.KIND_SURF), model_of(c, margin_cells=0.75), c.points, True)
    empty = np.zeros((0, 3), np.float32)
    m2 = matcher(ctx)
    m2.set_input_cloud(L.KIND_EDGE, empty)                                                 # an empty map is a map without an index
    assert call(ctx.h, L.KIND_EDGE, 0, C.byref(info), bufs, need) == E_STATE
