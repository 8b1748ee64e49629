"""Keyframe archive on the MI355X (lili_archive_*, lili_loop_cloud_archive): everything bit for bit against what was pushed and against the
archive-less calls (lili_loop_cloud, LoopClosure) on the same clouds and poses."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from lili_om_amd.archive import ARCHIVE_EDGE, ARCHIVE_SURF, ARCHIVE_FULL
from lili_om_amd.loop import LOOP_SOURCE, LOOP_TARGET
from tests.test_loop_icp_gpu import _keyframe, _path, _quat

pytestmark = pytest.mark.gpu

Q_BL = np.array([0.999, 0.01, -0.02, 0.03]) / np.linalg.norm([0.999, 0.01, -0.02, 0.03])
T_BL = np.array([0.1, -0.05, 0.2])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world():
    sc = synth.OutdoorScene()
    return sc.sample_surfaces(45.0, 45.0, 0.5, np.random.default_rng(11)).astype(np.float32)


def _view_rows(ctx, view):
    """a device view read back through the existing loop-state calls (a plain copy in, a plain copy out)"""
    lc = L.LoopClosure(ctx)
    lc.set_cloud(LOOP_SOURCE, view)
    return lc.get_cloud(LOOP_SOURCE).copy()


def _layouts(rows):
    """the rows (n, 4) as 16-byte rows, PointXYZI (32 bytes, intensity at 16) and PointXYZINormal (48 bytes, intensity at 32): (array, aux column)"""
    n = rows.shape[0]
    rng = np.random.default_rng(n)
    xyzi = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    xyzi[:, :3], xyzi[:, 4] = rows[:, :3], rows[:, 3]
    xyzin = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
    xyzin[:, :3], xyzin[:, 8] = rows[:, :3], rows[:, 3]
    return [(rows.copy(), 3), (xyzi, 4), (xyzin, 8)]


def test_round_trip_every_memory_and_layout(ctx):
    import torch
    rng = np.random.default_rng(2)
    arch = L.KeyframeArchive(ctx)
    want, keep = [], []
    for mem in ("pageable", "pinned", "device"):
        for li in range(3):
            clouds = []
            for n in (700 + 13 * li, 1500, 9000):
                rows = np.concatenate([rng.normal(0, 20, (n, 3)), rng.uniform(0, 255, (n, 1))], 1).astype(np.float32)
                rows[3] = [np.nan, 1, 2, 3]
                rows[5, 0] = -0.0
                arr, aux = _layouts(rows)[li]
                if mem == "pageable":
                    c = L.api.cloud_from_numpy(arr, aux_col=aux)
                elif mem == "pinned":
                    pa = L.api.PinnedArray(arr.shape)
                    pa.array[:] = arr
                    keep.append(pa)
                    c = L.api.Cloud(pa.array.ctypes.data, arr.shape[0], arr.shape[1] * 4, aux * 4, L.api.MEM_HOST)
                else:
                    d = torch.from_numpy(arr).cuda()
                    keep.append(d)
                    c = L.api.cloud_from_device(d.data_ptr(), arr.shape[0], arr.shape[1] * 4, aux * 4)
                clouds.append((c, rows))
            kid = arch.push(clouds[0][0], clouds[1][0], clouds[2][0], 1.5 * len(want), rng.normal(size=3), [1, 0, 0, 0])
            assert kid == len(want)
            want.append([c[1] for c in clouds])
    torch.cuda.synchronize()
    # a cloud without aux (12-byte rows), an absent kind and a keyframe of 0 points
    xyz = rng.normal(0, 5, (321, 3)).astype(np.float32)
    kid = arch.push(xyz, None, np.zeros((0, 4), np.float32), 99.0, [1, 2, 3], [1, 0, 0, 0])
    want.append([np.concatenate([xyz, np.zeros((321, 1), np.float32)], 1), np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)])
    n_kf, n_pts, used = arch.info()
    assert n_kf == len(want) == 10
    assert n_pts == tuple(sum(w[k].shape[0] for w in want) for k in range(3))
    assert used >= 16 * sum(n_pts)
    for kid, w in enumerate(want):
        for kind in (ARCHIVE_EDGE, ARCHIVE_SURF, ARCHIVE_FULL):
            assert _same(arch.get(kid, kind), w[kind]), (kid, kind)
            v = arch.view(kid, kind)
            assert v.n == w[kind].shape[0] and v.stride == 16 and v.aux_offset == 12 and v.mem == L.api.MEM_DEVICE
            if v.n:
                assert _same(_view_rows(ctx, v), w[kind]), (kid, kind)
    t, q, tm = arch.pose(9)
    assert tm == 99.0 and t.tolist() == [1, 2, 3] and q.tolist() == [1, 0, 0, 0]
    # argument errors leave the archive as it was
    lib, h = ctx.lib, ctx.h
    fo = L.api.FeatureOut(None, 0, 16, 0, 0)
    assert lib.lili_archive_get(h, 10, 0, C.byref(fo)) == -1 and lib.lili_archive_get(h, -1, 0, C.byref(fo)) == -1
    assert lib.lili_archive_get(h, 0, 3, C.byref(fo)) == -1
    assert lib.lili_archive_view(h, 0, 7, C.byref(L.api.Cloud())) == -1
    z = np.zeros(8)
    assert lib.lili_archive_set_poses(h, 9, 2, z.ctypes.data, z.ctypes.data) == -1
    assert lib.lili_archive_set_poses(h, 0, 1, None, z.ctypes.data) == -1
    assert lib.lili_archive_push(h, None, None, None, 0.0, None, z.ctypes.data, None) == -1
    ids = (C.c_int * 1)(10)
    assert lib.lili_loop_cloud_archive(h, 0, ids, 1, 0.4, None, None) == -1
    assert b"out of range" in lib.lili_last_error(h)
    assert arch.info() == (n_kf, n_pts, used)
    arch.reset()
    assert arch.info() == (0, (0, 0, 0), 0)


def test_push_slot_takes_the_matcher_slots_queries(ctx):
    rng = np.random.default_rng(4)
    surf = np.concatenate([rng.normal(0, 10, (2100, 3)), rng.uniform(0, 1, (2100, 1))], 1).astype(np.float32)
    edge = np.concatenate([rng.normal(0, 10, (310, 3)), rng.uniform(0, 1, (310, 1))], 1).astype(np.float32)
    full = np.concatenate([rng.normal(0, 10, (5000, 3)), rng.uniform(0, 1, (5000, 1))], 1).astype(np.float32)
    m = L.ScanToMapMatcher(ctx, L.make_params("livox"))
    m.set_queries(2, L.KIND_SURF, L.api.cloud_from_numpy(surf, aux_col=3))
    m.set_queries(2, L.KIND_EDGE, L.api.cloud_from_numpy(edge, aux_col=3))
    m.set_queries(3, L.KIND_SURF, L.api.cloud_from_numpy(surf[:40], aux_col=3))      # slot 3: no edge queries -> that kind is absent
    arch = L.KeyframeArchive(ctx)
    a = arch.push_slot(2, full, 0.0, [0, 0, 0], [1, 0, 0, 0])
    b = arch.push(edge, surf, full, 0.0, [0, 0, 0], [1, 0, 0, 0])
    c = arch.push_slot(3, None, 0.0, [0, 0, 0], [1, 0, 0, 0])
    for kind, w in ((ARCHIVE_EDGE, edge), (ARCHIVE_SURF, surf), (ARCHIVE_FULL, full)):
        assert _same(arch.get(a, kind), w) and _same(arch.get(b, kind), w), kind
    assert _same(arch.get(c, ARCHIVE_SURF), surf[:40]) and arch.get(c, ARCHIVE_EDGE).shape[0] == 0 and arch.get(c, ARCHIVE_FULL).shape[0] == 0
    assert ctx.lib.lili_archive_push_slot(ctx.h, 99, None, 0.0, np.zeros(3).ctypes.data, np.zeros(4).ctypes.data, None) == -1


def test_slabs_never_move_and_the_bound_holds(ctx):
    rng = np.random.default_rng(6)
    ctx.set_option("archive_slab_mb", 1)      # 1 MiB slabs: 20 000 rows of 16 bytes fit three times
    arch = L.KeyframeArchive(ctx)
    rows = [np.concatenate([rng.normal(0, 10, (20_000, 3)), rng.uniform(0, 1, (20_000, 1))], 1).astype(np.float32) for _ in range(14)]
    views = []
    for k, r in enumerate(rows[:12]):
        arch.push(None, None, r, float(k), [0, 0, 0], [1, 0, 0, 0])
        views.append(arch.view(k, ARCHIVE_FULL))
    n_kf, n_pts, used = arch.info()
    assert used == 4 * (1 << 20)      # three keyframes per slab
    big = np.concatenate(rows[:5])      # larger than a slab: a slab of its own
    arch.push(None, big, None, 12.0, [0, 0, 0], [1, 0, 0, 0])
    assert arch.info()[2] == used + 16 * big.shape[0]
    for k, v in enumerate(views):      # the views taken before later pushes still read their rows, at the same addresses
        assert arch.view(k, ARCHIVE_FULL).data == v.data
        assert _same(_view_rows(ctx, v), rows[k]), k
    assert _same(arch.get(12, ARCHIVE_SURF), big)
    # archive_max_mb: 7 MiB hold what is there (4 + 1.53 MiB) and one more slab, not two
    ctx.set_option("archive_max_mb", 7)
    arch.push(None, None, rows[12], 13.0, [0, 0, 0], [1, 0, 0, 0])
    before = arch.info()
    for k in range(2):
        arch.push(None, None, rows[13], 14.0 + k, [0, 0, 0], [1, 0, 0, 0])
    mid = arch.info()
    assert mid[0] == before[0] + 2 and mid[2] == before[2]      # (the slab had room for them)
    with pytest.raises(L.LiliError, match="archive_max_mb"):
        arch.push(None, None, rows[13], 16.0, [0, 0, 0], [1, 0, 0, 0])
    assert arch.info() == mid
    for k in range(12):
        assert _same(arch.get(k, ARCHIVE_FULL), rows[k]), k
    assert _same(arch.get(13, ARCHIVE_FULL), rows[12]) and _same(arch.get(15, ARCHIVE_FULL), rows[13])
    ctx.set_option("archive_max_mb", 0)
    arch.push(None, None, rows[13], 16.0, [0, 0, 0], [1, 0, 0, 0])
    assert arch.info()[0] == mid[0] + 1


def _scene(world):
    ts, Rs = _path(12)
    kfs = [_keyframe(world, ts[k], Rs[k], radius=12.0, seed=k) for k in range(12)]
    return ts, [_quat(R) for R in Rs], [k[0] for k in kfs], [k[1] for k in kfs]


def _both_ways(ctx, arch, variant, ts, qs, edge, surf, latest=9, his=2):
    """the submaps and the registration through the archive and through the caller's clouds: (clouds, counts, align result) each"""
    out = []
    for a in (arch, None):
        lc = L.LoopClosure(ctx, variant=variant, lc_map_width=3, q_bl=Q_BL, t_bl=T_BL, archive=a)
        counts = lc.assemble(latest, his) if a is not None else lc.assemble(latest, his, np.array(ts), np.array(qs), edge, surf)
        clouds = [lc.get_cloud(LOOP_SOURCE).copy(), lc.get_cloud(LOOP_TARGET).copy()]
        res = lc.align()
        out.append((clouds, counts, res))
    return out


def _assert_same_registration(a, b, tag):
    for x, y in zip(a[0], b[0]):
        assert _same(x, y), tag
    assert a[1] == b[1], tag
    ra, rb = a[2], b[2]
    assert np.array_equal(ra["transform"], rb["transform"]) and ra["fitness"] == rb["fitness"] and ra["log"] == rb["log"], tag
    assert (ra["converged"], ra["state"], ra["iterations"]) == (rb["converged"], rb["state"], rb["iterations"]), tag


def test_submaps_from_the_archive_equal_lili_loop_cloud(ctx, world):
    ts, qs, edge, surf = _scene(world)
    arch = L.KeyframeArchive(ctx, q_bl=Q_BL, t_bl=T_BL)
    for k in range(12):
        arch.push(edge[k], surf[k], None, 10.0 * k, ts[k], qs[k])
    for variant in ("livox", "rot"):
        a, b = _both_ways(ctx, arch, variant, ts, qs, edge, surf)
        assert a[1][0][0] > 0 and a[1][1][1] > 1000
        _assert_same_registration(a, b, variant)
    # correctPoses: perturbed poses for a stretch of keyframes, then the same comparison at the new poses
    rng = np.random.default_rng(8)
    ts2 = [t + rng.normal(0, 0.05, 3) if 1 <= k < 11 else t for k, t in enumerate(ts)]
    qs2 = []
    for k, q in enumerate(qs):
        q2 = q + rng.normal(0, 0.005, 4) if 1 <= k < 11 else q
        qs2.append(q2 / np.linalg.norm(q2))
    arch.set_poses(1, ts2[1:11], qs2[1:11])
    for variant in ("livox", "rot"):
        a, b = _both_ways(ctx, arch, variant, ts2, qs2, edge, surf)
        _assert_same_registration(a, b, variant + " reposed")
    old = _both_ways(ctx, None, "livox", ts, qs, edge, surf)[1]
    assert not _same(old[0][1], a[0][1])      # (the poses did move the target)


def test_perform_with_and_without_the_archive(ctx, world):
    """a revisit: keyframes 0 .. 11 around the loop, then three more near keyframes 0 .. 2 much later; the archive-backed object returns what the plain one returns"""
    ts, qs, edge, surf = _scene(world)
    ts, qs, edge, surf = ts + ts[:3], qs + qs[:3], edge + edge[:3], surf + surf[:3]
    times = np.array([2.0 * k for k in range(12)] + [200.0, 202.0, 204.0])
    arch = L.KeyframeArchive(ctx, q_bl=Q_BL, t_bl=T_BL)
    for k in range(15):
        arch.push(edge[k], surf[k], None, times[k], ts[k], qs[k])
    got = []
    for variant in ("livox", "rot"):
        kw = dict(variant=variant, lc_map_width=3, q_bl=Q_BL, t_bl=T_BL, lc_icp_thres=5.0, slide_window_width=3)
        plain = L.LoopClosure(ctx, **kw)
        with_a = L.LoopClosure(ctx, archive=arch, **kw)
        sel = np.asarray(ts[12], np.float32)
        r0 = plain.perform(np.array(ts, np.float32), times, sel, 206.0, np.array(ts), np.array(qs), edge, surf)
        r1 = with_a.perform(None, None, sel, 206.0)
        # the registration both objects ran is the same one, accepted or not (ROT's six source keyframes lie half-way round the loop: its ICP result may be refused)
        la, lb = plain.last, with_a.last
        assert np.array_equal(la["transform"], lb["transform"]) and la["fitness"] == lb["fitness"] and la["log"] == lb["log"], variant
        assert (r0 is None) == (r1 is None), variant
        if variant == "livox":
            assert r0 is not None
        if r0 is not None:
            assert r0[:2] == r1[:2] and r0[5] == r1[5]
            for x, y in zip(r0[2:5], r1[2:5]):
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
            got.append(r1[:2])
        assert with_a.detect(None, None, sel, 206.0) == plain.detect(np.array(ts, np.float32), times, sel, 206.0) == (12, 0)
    assert got[0] == (12, 0)
