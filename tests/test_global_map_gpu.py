"""The global map on the MI355X (lili_global_map*) against the plain numpy contract — tests/voxel_model.voxel_grid over the selected clouds placed by the
oracle's transform_cloud, concatenated in keyframe order — and, beyond what the model can check, against one lili_voxel_filter over the same placed concatenation.
Centroids, counts and order, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from lili_om_amd.archive import ARCHIVE_EDGE, ARCHIVE_SURF, ARCHIVE_FULL
from lili_om_amd.loop import LOOP_SOURCE, LOOP_TARGET
from tests import voxel_model as V
from tests.test_loop_icp_gpu import _keyframe, _path, _quat

pytestmark = pytest.mark.gpu

Q_BL = np.array([0.999, 0.01, -0.02, 0.03]) / np.linalg.norm([0.999, 0.01, -0.02, 0.03])
T_BL = np.array([0.1, -0.05, 0.2])
BAD = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [np.nan, np.nan, np.nan, np.nan]], np.float32)
ONE_BATCH, DEFAULT_BATCH = 1 << 27, 1 << 21


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _rows(xyz, seed):
    return np.concatenate([xyz, np.random.default_rng(seed).uniform(0, 1, (xyz.shape[0], 1))], 1).astype(np.float32)


def _model(O, clouds, ts_po, qs_po, ids, leaf, t_bl=T_BL, q_bl=Q_BL):
    """the contract: voxel_grid of the concatenation of the placed clouds (None / empty clouds contribute nothing)"""
    parts = []
    for k in ids:
        c = clouds[k]
        if c is None or c.shape[0] == 0:
            continue
        t, q = L.api.keyframe_map_pose(ts_po[k], qs_po[k], t_bl, q_bl)
        parts.append(O.transform_cloud(np.ascontiguousarray(c, np.float32), q, t))
    raw = np.concatenate(parts, 0) if parts else np.zeros((0, 4), np.float32)
    if not np.isfinite(raw[:, :3]).all(1).any():
        return raw.shape[0], np.zeros((0, 4), np.float32), np.zeros(0, np.int32)
    cen, cnt = V.voxel_grid(raw, leaf)
    return raw.shape[0], cen, cnt


def _check(gm, want, tag):
    n_raw, cen, cnt = want
    got, got_n = gm.get()
    assert got.shape == cen.shape, (tag, got.shape, cen.shape)
    assert _same(got, cen), tag
    assert np.array_equal(got_n, cnt), tag


def _force_rebuild(gm):
    gm.build(ARCHIVE_EDGE, 10 ** 6, 1.0)      # (another setting: whatever is built next starts from an empty table)


@pytest.fixture(scope="module")
def world():
    sc = synth.OutdoorScene()
    return sc.sample_surfaces(45.0, 45.0, 0.3, np.random.default_rng(11)).astype(np.float32)


@pytest.fixture(scope="module")
def sequence(world):
    """48 keyframes round the loop (full clouds of 10-25 k rows, one of them empty, non-finite rows here and there), then a stationary stretch: 220 keyframes of 300
    rows at one pose with millimetre jitter, 30 of which fall into ONE voxel at every leaf size tested (6600 members across the batches)"""
    rng = np.random.default_rng(31)
    ts, Rs = _path(48)
    ts_po, qs_po, edge, surf, full = [], [], [], [], []
    for k in range(48):
        e, s = _keyframe(world, ts[k], Rs[k], radius=22.0, seed=k)
        allp = np.concatenate([e, s])
        f = allp[rng.permutation(allp.shape[0])[: int(rng.integers(10_000, 25_001))]].copy()
        e, s = e[:: 2].copy(), s[:: 4].copy()
        if k % 5 == 1:
            f[100:104], s[7:11], e[2:6] = BAD, BAD, BAD
        if k == 6:
            f = np.zeros((0, 4), np.float32)
        ts_po.append(ts[k]); qs_po.append(_quat(Rs[k])); edge.append(e); surf.append(s); full.append(f)
    t_s, q_s = ts[0] + np.array([0.3, 0.2, 0.0]), _quat(Rs[0])
    t_m, q_m = L.api.keyframe_map_pose(t_s, q_s, T_BL, Q_BL)
    Rm = L.loop._matrix_from_quat(q_m / np.linalg.norm(q_m))
    centre = np.array([0.1 + 1.2 * 17, 0.1 + 1.2 * 2, 0.1 + 1.2])      # 0.1 from the voxel's low faces at leaf 0.2, 0.3 and 0.4
    base_map = np.concatenate([centre + rng.uniform(-0.02, 0.02, (30, 3)), t_m + rng.uniform(-6, 6, (270, 3))])
    for k in range(220):
        pm = base_map + rng.normal(0, 1e-3, base_map.shape)
        loc = _rows(((pm - t_m) @ Rm), 1000 + k)
        ts_po.append(t_s); qs_po.append(q_s); edge.append(None); surf.append(loc[::3].copy()); full.append(loc)
    return dict(ts=ts_po, qs=qs_po, edge=edge, surf=surf, full=full)


@pytest.fixture(scope="module")
def loaded(sequence):
    ctx = L.Context(0)
    arch = L.KeyframeArchive(ctx, q_bl=Q_BL, t_bl=T_BL)
    S = sequence
    for k in range(len(S["ts"])):
        arch.push(S["edge"][k], S["surf"][k], S["full"][k], 0.1 * k, S["ts"][k], S["qs"][k])
    yield ctx, arch, L.GlobalMap(arch)
    ctx.close()


def test_model_parity_over_kinds_intervals_leaves_and_batch_sizes(oracle, loaded, sequence):
    ctx, arch, gm = loaded
    S = sequence
    n_kf = len(S["ts"])
    clouds = {ARCHIVE_EDGE: S["edge"], ARCHIVE_SURF: S["surf"], ARCHIVE_FULL: S["full"]}
    cases = [(kind, interval, 0.3) for kind in (ARCHIVE_FULL, ARCHIVE_SURF, ARCHIVE_EDGE) for interval in (1, 3, 7, 1000)]
    cases += [(ARCHIVE_FULL, 1, 0.2), (ARCHIVE_FULL, 1, 0.4), (ARCHIVE_SURF, 3, 0.2), (ARCHIVE_EDGE, 7, 0.4)]
    batches = [ONE_BATCH, 200_000, 4096, DEFAULT_BATCH]      # one batch; a handful; smaller than one keyframe (keyframes split across batches); the default
    crowded = 0
    for ci, (kind, interval, leaf) in enumerate(cases):
        ids = list(range(0, n_kf, interval))
        want = _model(oracle, clouds[kind], S["ts"], S["qs"], ids, leaf)
        if kind == ARCHIVE_FULL and interval == 1:
            crowded = max(crowded, int(want[2].max()))
        for b in (batches if (kind, interval, leaf) == (ARCHIVE_FULL, 1, 0.3) else [batches[ci % 4], batches[(ci + 2) % 4]]):
            ctx.set_option("global_map_batch_points", b)
            _force_rebuild(gm)
            before = gm.stats()
            n_raw, n_map = gm.build(kind, interval, leaf)
            after = gm.stats()
            assert (after[0], after[1]) == (before[0], before[1] + 1) and after[2] == want[0]
            assert (n_raw, n_map) == (want[0], want[1].shape[0]), (kind, interval, leaf, b)
            _check(gm, want, (kind, interval, leaf, b))
    assert crowded > max(V.OCCUPANCY)      # a voxel fuller than the largest tier the filter's own tests cover, filled across many batches
    ctx.set_option("global_map_batch_points", DEFAULT_BATCH)
    tb, wb = gm.info()
    assert tb > 0 and wb > 0


def _small(world, n, rows=5000, seed=0):
    rng = np.random.default_rng(seed)
    ts, Rs = _path(n)
    full = []
    for k in range(n):
        e, s = _keyframe(world, ts[k], Rs[k], radius=15.0, seed=k)
        allp = np.concatenate([e, s])
        full.append(allp[rng.permutation(allp.shape[0])[:rows]].copy())
    return ts, [_quat(R) for R in Rs], full


def test_incremental_equals_fresh(oracle, world):
    ts, qs, full = _small(world, 40)
    a, b = L.Context(0), L.Context(0)
    try:
        for c in (a, b):
            c.set_option("global_map_batch_points", 60_000)
        arch_a, arch_b = L.KeyframeArchive(a, Q_BL, T_BL), L.KeyframeArchive(b, Q_BL, T_BL)
        gm_a, gm_b = L.GlobalMap(arch_a), L.GlobalMap(arch_b)
        for k in range(30):
            arch_a.push(None, None, full[k], k, ts[k], qs[k])
        r30 = gm_a.build(ARCHIVE_FULL, 1, 0.3)
        assert gm_a.stats() == (0, 1, sum(f.shape[0] for f in full[:30]))
        _check(gm_a, _model(oracle, full, ts, qs, range(30), 0.3), "30")
        for k in range(30, 40):
            arch_a.push(None, None, full[k], k, ts[k], qs[k])
        r40 = gm_a.build(ARCHIVE_FULL, 1, 0.3)
        assert gm_a.stats() == (1, 1, sum(f.shape[0] for f in full[30:]))
        for k in range(40):
            arch_b.push(None, None, full[k], k, ts[k], qs[k])
        assert gm_b.build(ARCHIVE_FULL, 1, 0.3) == r40 and r40[0] == sum(f.shape[0] for f in full) and r40[1] > r30[1]
        assert gm_b.stats() == (0, 1, r40[0])
        ga, gb = gm_a.get(), gm_b.get()
        assert _same(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])
        _check(gm_a, _model(oracle, full, ts, qs, range(40), 0.3), "40")
        # nothing new: incremental, nothing folded, the same map
        assert gm_a.build(ARCHIVE_FULL, 1, 0.3) == r40
        assert gm_a.stats() == (2, 1, 0)
        again = gm_a.get()
        assert _same(again[0], ga[0]) and np.array_equal(again[1], ga[1])
    finally:
        a.close()
        b.close()


def test_what_invalidates_the_table(oracle, world):
    ts, qs, full = _small(world, 12, rows=3000, seed=3)
    ctx = L.Context(0)
    try:
        ctx.set_option("global_map_batch_points", 10_000)
        arch = L.KeyframeArchive(ctx, Q_BL, T_BL)
        gm = L.GlobalMap(arch)
        for k in range(12):
            arch.push(full[k][::7].copy(), full[k][::2].copy(), full[k], k, ts[k], qs[k])
        gm.build(ARCHIVE_FULL, 3, 0.3)
        assert gm.stats()[:2] == (0, 1)
        # bit-equal poses: incremental; a keyframe outside the selection (interval 3, id 1): incremental
        arch.set_poses(0, ts, qs)
        gm.build(ARCHIVE_FULL, 3, 0.3)
        assert gm.stats() == (1, 1, 0)
        arch.set_poses(1, [ts[1] + 0.5], [qs[1]])
        gm.build(ARCHIVE_FULL, 3, 0.3)
        assert gm.stats() == (2, 1, 0)
        ts = list(ts)
        ts[1] = ts[1] + 0.5
        # a folded keyframe moves: rebuild, and the map is the model's at the new poses
        ts[3] = ts[3] + np.array([0.25, -0.1, 0.05])
        arch.set_poses(3, [ts[3]], [qs[3]])
        gm.build(ARCHIVE_FULL, 3, 0.3)
        assert gm.stats()[:2] == (2, 2)
        _check(gm, _model(oracle, full, ts, qs, range(0, 12, 3), 0.3), "moved")
        n_inc, n_reb = 2, 2
        # leaf, kind, interval, extrinsic: a rebuild each
        edge, surf = [f[::7] for f in full], [f[::2] for f in full]
        for kind, interval, leaf, src in ((ARCHIVE_FULL, 3, 0.4, full), (ARCHIVE_SURF, 3, 0.4, surf), (ARCHIVE_SURF, 2, 0.4, surf), (ARCHIVE_EDGE, 2, 0.4, edge)):
            gm.build(kind, interval, leaf)
            n_reb += 1
            assert gm.stats()[:2] == (n_inc, n_reb), (kind, interval, leaf)
            _check(gm, _model(oracle, src, ts, qs, range(0, 12, interval), leaf), (kind, interval, leaf))
        t_bl2 = T_BL + np.array([0.0, 0.02, 0.0])
        arch.set_extrinsic(t_bl2, Q_BL)
        gm.build(ARCHIVE_EDGE, 2, 0.4)
        n_reb += 1
        assert gm.stats()[:2] == (n_inc, n_reb)
        _check(gm, _model(oracle, edge, ts, qs, range(0, 12, 2), 0.4, t_bl=t_bl2), "extrinsic")
        gm.build(ARCHIVE_EDGE, 2, 0.4)
        n_inc += 1
        assert gm.stats() == (n_inc, n_reb, 0)
        # reset: an empty map, and the next call builds from scratch
        arch.reset()
        assert gm.build(ARCHIVE_EDGE, 2, 0.4) == (0, 0)
        n_reb += 1
        assert gm.stats() == (n_inc, n_reb, 0) and gm.get()[0].shape == (0, 4)
        arch.push(edge[0].copy(), None, None, 0.0, ts[0], qs[0])
        assert gm.build(ARCHIVE_EDGE, 2, 0.4)[0] == edge[0].shape[0]
        # bad arguments
        for bad in ((3, 1, 0.3), (-1, 1, 0.3), (ARCHIVE_FULL, 0, 0.3), (ARCHIVE_FULL, 1, 0.0)):
            assert ctx.lib.lili_global_map(ctx.h, bad[0], bad[1], C.c_float(bad[2]), None, None) == -1
    finally:
        ctx.close()


def test_int32_guard_over_everything_folded(oracle):
    (ex, ey, ez), leaf = V.OVERFLOW      # 2001 x 2001 x 601 voxels > 2^31 - 1; 2001 x 2001 x 501 fit
    ctx = L.Context(0)
    try:
        ctx.set_option("global_map_batch_points", 50_000)
        arch = L.KeyframeArchive(ctx)
        gm = L.GlobalMap(arch)
        ident_t, ident_q = np.zeros(3), np.array([1.0, 0, 0, 0])
        full = [V.box_cloud((ex, ey, ez - 10.0), 40_000, seed=k) for k in range(3)] + [V.box_cloud((ex, ey, 5.0), 3000, seed=9)]
        ts, qs = [np.zeros(3)] * 3 + [np.array([0.0, 0.0, ez - 5.0])], [ident_q] * 4      # the last keyframe alone reaches z = 60 m
        for k in range(3):
            arch.push(None, None, full[k], k, ts[k], qs[k])
        gm.build(ARCHIVE_FULL, 1, leaf)
        _check(gm, _model(oracle, full, ts, qs, range(3), leaf, ident_t, ident_q), "before")
        arch.push(None, None, full[3], 3, ts[3], qs[3])
        with pytest.raises(L.LiliError) as e_map:
            gm.build(ARCHIVE_FULL, 1, leaf)
        placed = np.concatenate(full[:3] + [oracle.transform_cloud(full[3], ident_q, ts[3])])
        with pytest.raises(L.LiliError) as e_filter:
            L.api.voxel_filter(ctx, placed, leaf)
        assert str(e_map.value) == str(e_filter.value) and "int32" in str(e_map.value)
        with pytest.raises(V.IndexOverflow):
            V.voxel_grid(placed, leaf)
        with pytest.raises(L.LiliError):
            gm.get()
        ts = ts[:3] + [np.array([0.0, 0.0, ez - 20.0])]      # back inside
        arch.set_poses(3, [ts[3]], [qs[3]])
        reb = gm.stats()[1]
        gm.build(ARCHIVE_FULL, 1, leaf)
        assert gm.stats()[1] == reb + 1
        _check(gm, _model(oracle, full, ts, qs, range(4), leaf, ident_t, ident_q), "after")
    finally:
        ctx.close()


def test_refuses_a_point_beyond_the_key_range():
    """one keyframe of 8 points within 1 cm of (2000, 0, 0) at leaf 0.001: the box is a few voxels wide (PCL's int32 guard does not fire), the voxel index 2 * 10^6
    exceeds the 2^20 the absolute key can hold — an argument error that says so"""
    ctx = L.Context(0)
    try:
        arch = L.KeyframeArchive(ctx)
        gm = L.GlobalMap(arch)
        pts = _rows(np.array([2000.0, 0.0, 0.0]) + np.random.default_rng(5).uniform(-0.005, 0.005, (8, 3)), 6)
        arch.push(None, None, pts, 0.0, np.zeros(3), np.array([1.0, 0, 0, 0]))
        with pytest.raises(L.LiliError) as e:
            gm.build(ARCHIVE_FULL, 1, 0.001)
        assert str(e.value).startswith("lili error -1:") and "2^20 voxels" in str(e.value)      # LILI_E_ARG
    finally:
        ctx.close()


def test_archive_and_map_calls_leave_the_rest_of_the_context_alone(world):
    """the same local-map / voxel-filter / loop sequence with and without archive and global-map calls interleaved: identical maps, statistics, clouds and registration"""
    ts, qs, full = _small(world, 8, rows=12_000, seed=5)
    src, tgt = full[0][::3].copy(), np.concatenate(full[:3])

    def run(with_archive):
        ctx = L.Context(0)
        try:
            lc = L.LoopClosure(ctx)
            lm = L.LocalMap(ctx, L.KIND_SURF, width=4, leaf=0.4)
            lc.set_cloud(LOOP_TARGET, tgt)
            lc.set_cloud(LOOP_SOURCE, src)
            if with_archive:
                arch = L.KeyframeArchive(ctx, Q_BL, T_BL)
                gm = L.GlobalMap(arch)
            out = []
            for k in range(8):
                out.append(L.api.voxel_filter(ctx, full[k], 0.4)[0].tobytes())
                if with_archive:
                    arch.push(full[k][::5].copy(), full[k][::2].copy(), full[k], k, ts[k], qs[k])
                    gm.build(ARCHIVE_FULL, 1, 0.3)
                    gm.get()
                    arch.get(k, ARCHIVE_SURF)
                lm.push(full[k], ts[k], qs[k])
                out.append(lm.commit())
                out.append(lm.get(400000).tobytes())
                if with_archive and k == 4:
                    arch.set_poses(2, [ts[2] + 0.1], [qs[2]])
                    gm.build(ARCHIVE_FULL, 1, 0.3)
                out.append(L.api.voxel_filter(ctx, full[k], 0.4)[0].tobytes())
                out.append(L.api.voxel_filter_stats(ctx))
            out.append(lm.stats())
            out.append(lc.get_cloud(LOOP_SOURCE).tobytes())      # the ICP source / target set before the builds are still there
            out.append(lc.get_cloud(LOOP_TARGET).tobytes())
            res = lc.align()
            out.append((res["transform"].tobytes(), res["fitness"], res["iterations"]))
            return out
        finally:
            ctx.close()

    assert run(True) == run(False)


def test_larger_than_the_model_can_check(world):
    """400 keyframes x 24 k rows at interval 1: five default-size batches and two incremental updates, against ONE lili_voxel_filter over the same placed concatenation
    (gathered by the existing lili_loop_cloud from the archive's views).  Equal rows in equal order: the table's keys ascend exactly as the filter's voxel indices do."""
    import torch
    n_kf, rows, leaf = 400, 24_000, 0.3
    rng = np.random.default_rng(77)
    ts, Rs = _path(n_kf)
    ctx = L.Context(0)
    try:
        arch = L.KeyframeArchive(ctx, Q_BL, T_BL)
        gm = L.GlobalMap(arch)
        n_finite = 0

        def push(k):
            nonlocal n_finite
            sel = world[np.linalg.norm(world[:, :2] - ts[k][:2], axis=1) < 22.0]
            sel = sel[rng.integers(0, sel.shape[0], rows)]
            loc = _rows((sel.astype(np.float64) - ts[k]) @ Rs[k], k)
            if k % 50 == 0:
                loc[10:14] = BAD
            n_finite += int(np.isfinite(loc[:, :3]).all(1).sum())
            arch.push(None, None, loc, 0.1 * k, ts[k], _quat(Rs[k]))

        for k in range(360):
            push(k)
        assert gm.build(ARCHIVE_FULL, 1, leaf)[0] == 360 * rows
        for lo, hi in ((360, 380), (380, 400)):
            for k in range(lo, hi):
                push(k)
            n_raw, n_map = gm.build(ARCHIVE_FULL, 1, leaf)
        assert gm.stats() == (2, 1, 20 * rows) and n_raw == n_kf * rows < 2 ** 31
        cen, cnt = gm.get()
        assert int(cnt.sum(dtype=np.int64)) == n_finite and cen.shape[0] == n_map
        # the parent's way to the same map: lili_loop_cloud's gather (leaf <= 0: no filter) of the views at the map poses, then one lili_voxel_filter on the device
        views = (L.api.Cloud * n_kf)(*[arch.view(k, ARCHIVE_FULL) for k in range(n_kf)])
        poses = [L.api.keyframe_map_pose(ts[k], _quat(Rs[k]), T_BL, Q_BL) for k in range(n_kf)]
        t = np.ascontiguousarray(np.array([p[0] for p in poses]).reshape(-1))
        q = np.ascontiguousarray(np.array([p[1] for p in poses]).reshape(-1))
        a, b = C.c_int64(0), C.c_int64(0)
        ctx._chk(ctx.lib.lili_loop_cloud(ctx.h, LOOP_SOURCE, views, n_kf, t.ctypes.data, q.ctypes.data, C.c_float(0.0), C.byref(a), C.byref(b)))
        assert a.value == n_kf * rows
        raw = torch.empty((n_kf * rows, 4), dtype=torch.float32, device="cuda")
        fo = L.api.FeatureOut(raw.data_ptr(), raw.shape[0], 16, L.api.MEM_DEVICE, 0)
        ctx._chk(ctx.lib.lili_icp_get_cloud(ctx.h, LOOP_SOURCE, C.byref(fo)))
        want = np.zeros((n_map + 16, 4), np.float32)
        want_n = np.zeros(n_map + 16, np.int32)
        fo = L.api.FeatureOut(want.ctypes.data, want.shape[0], 16, L.api.MEM_HOST, 0)
        ctx._chk(ctx.lib.lili_voxel_filter(ctx.h, C.byref(L.api.cloud_from_device(raw.data_ptr(), raw.shape[0], 16, 12)), C.c_float(leaf), C.byref(fo), want_n.ctypes.data))
        assert fo.count == n_map
        assert _same(cen, want[:n_map]) and np.array_equal(cnt, want_n[:n_map])
        torch.cuda.synchronize()
    finally:
        ctx.close()
