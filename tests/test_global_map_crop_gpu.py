"""The crop, export and import of the global map on the MI355X (lili_global_map_crop / _export / _import) against tests/map_crop_model.py: the
brute-force mask over the exported keys, applied to what lili_global_map_get returns.  Rows and counts, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd.archive import ARCHIVE_FULL, ARCHIVE_SURF
from tests import map_crop_model as M

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -3
IDENT_T, IDENT_Q = np.zeros(3), np.array([1.0, 0, 0, 0])
LEAVES = (0.3, 0.4)
INF = np.inf


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _keyframes():
    """12 keyframes in the map frame round the origin: eleven of 2 000 points and one the size of a spinning LiDAR's (30 000), a few non-finite rows among them"""
    rng = np.random.default_rng(404)
    out = []
    for k in range(12):
        n = 30_000 if k == 5 else 2_000
        c = np.array([6.0 * (k % 4) - 9.0, 5.0 * (k // 4) - 5.0, 0.5])
        p = c + rng.normal(0, 1, (n, 3)) * np.array([6.0, 6.0, 1.5])
        rows = np.concatenate([p, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
        if k == 2:
            rows[10, 0], rows[11, 2] = np.nan, np.inf
        out.append(rows)
    return out


def _push_all(arch, kfs):
    for k, rows in enumerate(kfs):
        arch.push(None, None, rows, 0.1 * k, IDENT_T, IDENT_Q)


class Built:
    def __init__(self, leaf, kfs):
        self.leaf = leaf
        self.ctx = L.Context(0)
        self.arch = L.KeyframeArchive(self.ctx)
        _push_all(self.arch, kfs)
        self.gm = L.GlobalMap(self.arch)
        self.gm.build(ARCHIVE_FULL, 1, leaf)
        self.cen, self.cnt = self.gm.get()
        self.exp = self.gm.export()
        self.keys = self.exp["keys"]

    def want(self, lo, hi):
        idx = M.crop_mask(self.keys, lo, hi, self.leaf)
        return self.cen[idx], self.cnt[idx]

    def check(self, lo, hi, tag, expect=None):
        rows, cnt = self.gm.crop(lo, hi)
        w_rows, w_cnt = self.want(lo, hi)
        assert _same(rows, w_rows) and np.array_equal(cnt, w_cnt), (tag, rows.shape, w_rows.shape)
        if expect is not None:
            assert rows.shape[0] == expect, (tag, rows.shape[0], expect)
        return rows.shape[0]


@pytest.fixture(scope="module")
def keyframes():
    return _keyframes()


@pytest.fixture(scope="module")
def built(keyframes):
    b = {leaf: Built(leaf, keyframes) for leaf in LEAVES}
    yield b
    for v in b.values():
        v.ctx.close()


def _voxel_point(key, leaf):
    """a point well inside the voxel of `key`"""
    i, j, k = (int(v[0]) for v in M.unpack(np.array([key], np.uint64)))
    p = ((np.array([i, j, k], np.float64) - M.OFFSET + 0.5) * leaf).astype(np.float32)
    assert M.point_keys(p[None, :], leaf)[0] == key
    return p


@pytest.mark.parametrize("leaf", LEAVES)
def test_export_is_the_table(built, keyframes, leaf):
    B = built[leaf]
    allp = np.concatenate(keyframes)
    fin = allp[np.isfinite(allp[:, :3]).all(1)]
    keys = M.point_keys(fin, leaf)
    uniq, counts = np.unique(keys, return_counts=True)
    assert B.keys.dtype == np.uint64 and np.array_equal(B.keys, uniq) and np.array_equal(B.exp["counts"], counts) and np.array_equal(B.exp["counts"], B.cnt)
    assert B.exp["leaf"] == np.float32(leaf) and B.exp["kind"] == ARCHIVE_FULL and B.keys.shape[0] > 10_000
    # the centroids are the exported sums over the exported counts, and every centroid lies in its voxel
    assert _same(B.cen, B.exp["sums"] / B.exp["counts"].astype(np.float32)[:, None])


@pytest.mark.parametrize("leaf", LEAVES)
def test_crop_equals_the_mask(built, leaf):
    B = built[leaf]
    n_tab = B.keys.shape[0]
    i, j, k = M.unpack(B.keys)
    lo_all = ((np.array([i.min(), j.min(), k.min()]) - M.OFFSET - 1) * leaf).astype(np.float32)
    hi_all = ((np.array([i.max(), j.max(), k.max()]) - M.OFFSET + 2) * leaf).astype(np.float32)
    # the whole table: get()
    rows, cnt = B.gm.crop(lo_all, hi_all)
    assert _same(rows, B.cen) and np.array_equal(cnt, B.cnt)
    B.check(lo_all, hi_all, "whole", n_tab)
    # nothing inside: far away; above the table (no k of the box is a k of the table); inside the table's k range but beside every point
    B.check([1000, 1000, 0], [1001, 1001, 1], "far", 0)
    B.check([lo_all[0], lo_all[1], hi_all[2] + 5], [hi_all[0], hi_all[1], hi_all[2] + 9], "above", 0)
    B.check([hi_all[0] + 2, lo_all[1], lo_all[2]], [hi_all[0] + 4, hi_all[1], hi_all[2]], "beside: every (k, j) row has its voxels below the i range", 0)
    B.check([lo_all[0] - 4, lo_all[1], lo_all[2]], [lo_all[0] - 2, hi_all[1], hi_all[2]], "beside: every (k, j) row has its voxels above the i range", 0)
    # a single voxel; the voxels of the first and of the last key
    for pos in (n_tab // 2, n_tab // 3, 0, n_tab - 1):
        p = _voxel_point(B.keys[pos], leaf)
        rows, cnt = B.gm.crop(p, p)
        assert rows.shape[0] == 1 and _same(rows, B.cen[pos:pos + 1]) and cnt[0] == B.cnt[pos], pos
        B.check(p, p, ("voxel", pos), 1)
    # faces on voxel boundaries and one f32 ulp to either side, as the low and as the high face of each axis
    sizes = set()
    for axis in range(3):
        for m in (-7, -1, 0, 1, 2, 9):
            x = np.float32(m * leaf) if axis < 2 else np.float32((m % 3) * leaf)
            for face in (np.nextafter(x, np.float32(-INF)), x, np.nextafter(x, np.float32(INF))):
                lo, hi = np.array([-8, -8, -2], np.float32), np.array([8, 8, 3], np.float32)
                lo[axis] = face
                sizes.add(B.check(lo, hi, ("low face", axis, m, face)))
                lo, hi = np.array([-8, -8, -2], np.float32), np.array([8, 8, 3], np.float32)
                hi[axis] = max(face, lo[axis])
                sizes.add(B.check(lo, hi, ("high face", axis, m, face)))
    assert len(sizes) > 20 and min(sizes) > 0
    # unbounded z faces; unbounded x faces; everything but y unbounded
    assert B.check([-5, -5, -INF], [5, 5, 0.5], "z from -inf") > 0
    assert B.check([-5, -5, 0.5], [5, 5, INF], "z to +inf") > 0
    full_z = B.check([-5, -5, -INF], [5, 5, INF], "all z")
    assert full_z == B.check([-5, -5, lo_all[2]], [5, 5, hi_all[2]], "all z, bounded")
    assert B.check([-INF, -5, -INF], [INF, 5, INF], "x and z unbounded") > full_z
    # boxes straddling the origin
    for lo, hi in (([-3, -2, -1], [2, 3, 1]), ([-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]), ([-leaf, -leaf, -leaf], [0, 0, 0]), ([0, 0, 0], [leaf, leaf, leaf])):
        assert B.check(lo, hi, ("origin", lo, hi)) > 0
    B.check([-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], "the one voxel whose low corner is the origin (-0.0 floors to 0)")
    # random boxes
    rng = np.random.default_rng(9)
    for t in range(20):
        c, h = rng.uniform(-12, 12, 3) * np.array([1, 1, 0.2]), rng.uniform(0, 10, 3) * np.array([1, 1, 0.3])
        B.check(c - h, c + h, ("random", t))


def _synthetic_table(n, seed):
    rng = np.random.default_rng(seed)
    ijk = rng.integers(M.OFFSET - 40, M.OFFSET + 40, (4 * n + 8, 3))
    keys = np.unique(M.pack(ijk[:, 0], ijk[:, 1], ijk[:, 2]))
    keys = np.sort(rng.choice(keys, n, replace=False))
    cnt = rng.integers(1, 9, n).astype(np.int32)
    sums = rng.uniform(-50, 50, (n, 4)).astype(np.float32)
    return keys, sums, cnt


def test_table_sizes_at_the_bisection_ends(gpu_ctx):
    """imported tables of 1, 2^m - 1, 2^m and 2^m + 1 voxels: the first and the last voxel, the whole table and random boxes"""
    leaf = 0.4
    gm = L.GlobalMap(L.KeyframeArchive(gpu_ctx))
    wide_lo, wide_hi = np.full(3, -50 * leaf, np.float32), np.full(3, 50 * leaf, np.float32)
    for n in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025):
        keys, sums, cnt = _synthetic_table(n, n)
        assert gm.load_table(keys, sums, cnt, leaf, ARCHIVE_SURF) == n
        cen, got_cnt = gm.get()
        assert cen.shape[0] == n and np.array_equal(got_cnt, cnt) and _same(cen, sums / cnt.astype(np.float32)[:, None])
        rows, c = gm.crop(wide_lo, wide_hi)
        assert _same(rows, cen) and np.array_equal(c, cnt), n
        for pos in (0, n - 1, n // 2):
            p = _voxel_point(keys[pos], leaf)
            rows, c = gm.crop(p, p)
            assert rows.shape[0] == 1 and _same(rows, cen[pos:pos + 1]) and c[0] == cnt[pos], (n, pos)
        rng = np.random.default_rng(n)
        for _ in range(6):
            ctr, h = rng.uniform(-16, 16, 3), rng.uniform(0, 12, 3)
            lo, hi = (ctr - h).astype(np.float32), (ctr + h).astype(np.float32)
            idx = M.crop_mask(keys, lo, hi, leaf)
            rows, c = gm.crop(lo, hi)
            assert _same(rows, cen[idx]) and np.array_equal(c, cnt[idx]), (n, lo, hi)
    # an empty table is a table
    assert gm.load_table(np.zeros(0, np.uint64), np.zeros((0, 4), np.float32), np.zeros(0, np.int32), leaf, ARCHIVE_SURF) == 0
    assert gm.get()[0].shape == (0, 4) and gm.crop(wide_lo, wide_hi)[0].shape == (0, 4) and gm.export()["keys"].shape == (0,)


def test_host_device_capacity_and_repeatability(built, keyframes):
    import torch
    B = built[0.3]
    lo, hi = np.array([-6, -7, -INF], np.float32), np.array([9, 4, INF], np.float32)
    rows, cnt = B.gm.crop(lo, hi)
    n = rows.shape[0]
    assert n > 2000
    # device output: the same bytes
    d_rows, d_cnt = B.gm.crop(lo, hi, device=True)
    assert d_rows.is_cuda and _same(d_rows.cpu().numpy(), rows) and np.array_equal(d_cnt.cpu().numpy(), cnt)
    # a capacity smaller than n: the prefix, n reported, nothing behind it written (host and device)
    cap = n // 3
    out, oc = np.full((n, 4), -7.0, np.float32), np.full(n, -7, np.int32)
    fo, got = L.api.FeatureOut(out.ctypes.data, cap, 16, L.api.MEM_HOST, 0), C.c_int64(0)
    B.ctx._chk(B.ctx.lib.lili_global_map_crop(B.ctx.h, lo.ctypes.data, hi.ctypes.data, C.byref(fo), oc.ctypes.data, C.byref(got)))
    assert got.value == n and fo.count == n and _same(out[:cap], rows[:cap]) and np.array_equal(oc[:cap], cnt[:cap]) and (out[cap:] == -7.0).all() and (oc[cap:] == -7).all()
    d_out = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    assert B.gm.crop_into(lo, hi, d_out.data_ptr(), cap) == n
    h = d_out.cpu().numpy()
    assert _same(h[:cap], rows[:cap]) and (h[cap:] == -7.0).all()
    # a strided host output
    wide = np.full((n, 6), -7.0, np.float32)
    fo = L.api.FeatureOut(wide.ctypes.data, n, 24, L.api.MEM_HOST, 0)
    B.ctx._chk(B.ctx.lib.lili_global_map_crop(B.ctx.h, lo.ctypes.data, hi.ctypes.data, C.byref(fo), None, None))
    assert _same(np.ascontiguousarray(wide[:, :4]), rows) and (wide[:, 4:] == -7.0).all()
    # a second run, and a second context that built the same map
    again = B.gm.crop(lo, hi)
    assert _same(again[0], rows) and np.array_equal(again[1], cnt)
    other = Built(0.3, keyframes)
    try:
        r2, c2 = other.gm.crop(lo, hi)
        assert _same(r2, rows) and np.array_equal(c2, cnt)
    finally:
        other.ctx.close()


def test_error_cases(built):
    B = built[0.4]
    lib, h = B.ctx.lib, B.ctx.h
    fo = L.api.FeatureOut(None, 0, 16, L.api.MEM_HOST, 0)

    def rc(lo, hi):
        lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        return lib.lili_global_map_crop(h, lo.ctypes.data, hi.ctypes.data, C.byref(fo), None, None)

    assert rc([0, 0, 0], [1, 1, 1]) == 0
    for axis in range(3):
        lo, hi = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
        lo[axis] = 2.0
        assert rc(lo, hi) == E_ARG
        lo[axis] = np.nan
        assert rc(lo, hi) == E_ARG
        lo[axis], hi[axis] = 0.0, np.nan
        assert rc(lo, hi) == E_ARG
    assert rc([INF, 0, 0], [INF, 1, 1]) == 0 and rc([-INF, 0, 0], [-INF, 1, 1]) == 0
    assert lib.lili_global_map_crop(h, None, None, C.byref(fo), None, None) == E_ARG
    # an unbounded y face: 2^21 rows per layer of the table — more than 2^24 in all, and the message says how many
    k = M.unpack(B.keys)[2]
    n_rows = (int(k.max()) - int(k.min()) + 1) << 21
    assert n_rows > 1 << 24
    with pytest.raises(L.LiliError, match=f"lili error {E_ARG}.*{n_rows}"):
        B.gm.crop([-INF, -INF, -INF], [INF, INF, INF])
    assert B.gm.crop([-INF, -INF, 0.45], [INF, INF, 0.55])[0].shape[0] == M.crop_mask(B.keys, [-INF, -INF, 0.45], [INF, INF, 0.55], 0.4).shape[0] > 0      # one layer: 2^21 rows
    # no map: a fresh context, and a context whose build failed
    ctx = L.Context(0)
    try:
        gm = L.GlobalMap(L.KeyframeArchive(ctx))
        for call in (lambda: gm.crop([0, 0, 0], [1, 1, 1]), gm.export):
            with pytest.raises(L.LiliError, match=f"lili error {E_STATE}"):
                call()
    finally:
        ctx.close()


def test_export_import_round_trip(built, tmp_path):
    B = built[0.4]
    lo, hi = np.array([-4, -9, -1], np.float32), np.array([11, 3, 2], np.float32)
    ctx = L.Context(0)
    try:
        gm = L.GlobalMap(L.KeyframeArchive(ctx))
        e = B.exp
        gm.load_table(e["keys"], e["sums"], e["counts"], e["leaf"], e["kind"])
        for a, b in ((gm.get(), B.gm.get()), (gm.crop(lo, hi), B.gm.crop(lo, hi))):
            assert _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].shape[0] > 1000
        e2 = gm.export()
        assert np.array_equal(e2["keys"], e["keys"]) and _same(e2["sums"], e["sums"]) and np.array_equal(e2["counts"], e["counts"]) and e2["leaf"] == e["leaf"] and e2["kind"] == e["kind"]
        assert gm.info()[0] > 0
        # through a file
        path = str(tmp_path / "map.npz")
        B.gm.save(path)
        with np.load(path) as f:
            assert sorted(f.files) == ["counts", "keys", "kind", "leaf", "sums", "version"] and int(f["version"]) == 1 and f["keys"].dtype == np.uint64
            fields = {k: f[k] for k in f.files}
        gm.load_table(*_synthetic_table(5, 5), 0.4, ARCHIVE_SURF)      # (something else in between)
        assert gm.load(path) == e["keys"].shape[0]
        a, b = gm.crop(lo, hi), B.gm.crop(lo, hi)
        assert _same(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert gm.export()["kind"] == ARCHIVE_FULL
        fields["version"] = np.int32(2)
        bad = str(tmp_path / "future.npz")
        np.savez(bad, **fields)
        with pytest.raises(ValueError, match="version 2"):
            gm.load(bad)
    finally:
        ctx.close()


def test_invalid_imports_leave_no_table(gpu_ctx):
    gm = L.GlobalMap(L.KeyframeArchive(gpu_ctx))
    keys, sums, cnt = _synthetic_table(300, 1)

    def swapped():
        k = keys.copy(); k[[100, 200]] = k[[200, 100]]
        return k, sums, cnt

    def duplicate():
        k = keys.copy(); k[150] = k[149]
        return k, sums, cnt

    def component():
        k = keys.copy(); k[-1] |= np.uint64(1) << np.uint64(63)       # k = 2^21 and more
        return k, sums, cnt

    def count0():
        c = cnt.copy(); c[299] = 0
        return keys, sums, c

    def first_pair():
        k = keys.copy(); k[0] = k[1]
        return k, sums, cnt

    for case in (swapped, duplicate, component, count0, first_pair):
        gm.load_table(keys, sums, cnt, 0.4, ARCHIVE_SURF)
        assert gm.get()[0].shape[0] == 300
        with pytest.raises(L.LiliError, match=f"lili error {E_ARG}"):
            gm.load_table(*case(), 0.4, ARCHIVE_SURF)
        for call in (gm.get, gm.export, lambda: gm.crop([0, 0, 0], [1, 1, 1])):      # the table is empty: there is no map
            with pytest.raises(L.LiliError, match=f"lili error {E_STATE}"):
                call()
    lib, h = gpu_ctx.lib, gpu_ctx.h
    args = (keys.ctypes.data, sums.ctypes.data, cnt.ctypes.data)
    assert lib.lili_global_map_import(h, C.c_float(0.0), ARCHIVE_SURF, 300, *args) == E_ARG
    assert lib.lili_global_map_import(h, C.c_float(0.4), 3, 300, *args) == E_ARG
    assert lib.lili_global_map_import(h, C.c_float(0.4), ARCHIVE_SURF, -1, *args) == E_ARG
    assert lib.lili_global_map_import(h, C.c_float(0.4), ARCHIVE_SURF, 300, None, sums.ctypes.data, cnt.ctypes.data) == E_ARG


def test_build_after_import_starts_from_the_archive(built, keyframes):
    """an imported table is not extended: the next lili_global_map is a rebuild over this context's archive, bit-equal to the build of a context that never imported"""
    B = built[0.3]
    ctx = L.Context(0)
    try:
        arch = L.KeyframeArchive(ctx)
        gm = L.GlobalMap(arch)
        _push_all(arch, keyframes)
        gm.build(ARCHIVE_FULL, 1, 0.3)
        assert gm.stats()[:2] == (0, 1)
        gm.load_table(*_synthetic_table(500, 2), 0.3, ARCHIVE_FULL)      # the same leaf and kind: still not extended
        assert gm.get()[0].shape[0] == 500
        n_raw, n_map = gm.build(ARCHIVE_FULL, 1, 0.3)
        assert gm.stats()[:2] == (0, 2) and n_map == B.keys.shape[0] and n_raw == sum(k.shape[0] for k in keyframes)
        cen, cnt = gm.get()
        assert _same(cen, B.cen) and np.array_equal(cnt, B.cnt)
        e = gm.export()
        assert np.array_equal(e["keys"], B.keys) and _same(e["sums"], B.exp["sums"])
        assert gm.build(ARCHIVE_FULL, 1, 0.3) == (n_raw, n_map) and gm.stats()[:2] == (1, 2)      # and from here on incremental again
    finally:
        ctx.close()
