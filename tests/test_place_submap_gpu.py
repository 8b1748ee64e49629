"""Levelled submap descriptors on the MI355X (lili_place_set_submap / _describe_submap / _window, PlaceRecognition(back, fwd, level)) against the
numpy referee (tests/place_submap_model.py) with the library's own relative placements: descriptors bit for bit, the rebuild rule descriptor by descriptor, the
search within 1e-12 with exact ids and shifts, and a revisit in the opposite direction through an 81.7 degree wedge, which one keyframe's descriptor cannot find."""
import ctypes as C
import math

import numpy as np
import pytest

import lili_om_amd as L
from tests import place_model as PM
from tests import place_submap_cases as CS
from tests import place_submap_model as SM

pytestmark = pytest.mark.gpu

F = np.float32
T = L.api.PLACE_TILE_ROWS


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _as_memory(rows, mem, stride, keep):
    """the rows as a lili_cloud in pageable, page-locked or device memory, 12-, 16- or 32-byte rows"""
    import torch
    if stride == 12:
        arr, aux = np.ascontiguousarray(rows[:, :3]), None
    elif stride == 16:
        arr, aux = np.ascontiguousarray(rows), 3
    else:
        arr = np.random.default_rng(rows.shape[0]).uniform(-50, 50, (rows.shape[0], 8)).astype(F)
        arr[:, :3], arr[:, 4], aux = rows[:, :3], rows[:, 3], 4
    aux_off = -1 if aux is None else aux * 4
    if mem == "pageable":
        keep.append(arr)
        return L.api.cloud_from_numpy(arr, aux_col=aux)
    if mem == "pinned":
        pa = L.api.PinnedArray(arr.shape if arr.shape[0] else (1, arr.shape[1]))
        pa.array[:arr.shape[0]] = arr
        keep.append(pa)
        return L.api.Cloud(pa.array.ctypes.data, arr.shape[0], arr.shape[1] * 4, aux_off, L.api.MEM_HOST)
    d = torch.from_numpy(arr if arr.shape[0] else np.zeros((1, arr.shape[1]), F)).cuda()
    torch.cuda.synchronize()
    keep.append(d)
    return L.api.cloud_from_device(d.data_ptr(), arr.shape[0], arr.shape[1] * 4, aux_off)


def _pose(rng, spread=20.0, tilt=0.2):
    """a LiDAR map pose: anywhere within `spread` metres, any yaw, up to `tilt` rad of roll and pitch"""
    yaw, roll, pitch = rng.uniform(-math.pi, math.pi), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)
    R = CS.rz(math.degrees(yaw)) @ CS.ry(math.degrees(pitch)) @ np.array([[1, 0, 0], [0, math.cos(roll), -math.sin(roll)], [0, math.sin(roll), math.cos(roll)]])
    return np.concatenate([rng.uniform(-spread, spread, 2), rng.uniform(-1, 1, 1), L.loop.quat_from_matrix(R)])


def _skew(angle):
    ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * ax])


# ---- 1. the plain setting is today's descriptor ---------------------------------------------------------------------------------------------------------------------

def test_plain_setting_is_todays_descriptor(ctx):
    hard = CS.hard_cloud(20, 60, 80.0, 2.0, np.random.default_rng(1020))
    clouds = [hard[:m].copy() for m in (0, 1, 65, 257)] + [hard]
    want = [PM.describe(c) for c in clouds]
    arch = L.KeyframeArchive(ctx)
    for i, c in enumerate(clouds):
        arch.push(None, None, c, float(i), [i, 0, 0], [1, 0, 0, 0])
    pr = L.PlaceRecognition(arch)
    sub = L.api.PlaceSubmap(9, 9, 9, 9)
    ctx._chk(ctx.lib.lili_place_get_submap(ctx.h, C.byref(sub)))
    assert (sub.back, sub.fwd, sub.level, sub.reserved_) == (0, 0, 0, 0)              # never called: zeros
    assert pr.update() == len(clouds)
    got_never = [pr.descriptor(i) for i in range(len(clouds))]
    ctx._chk(ctx.lib.lili_place_set_submap(ctx.h, None))                              # NULL: zeros — the same setting, nothing is dropped
    assert pr.info()[0] == len(clouds) and pr.update() == 0
    L.PlaceRecognition(arch, back=1).update()
    assert pr.update() == len(clouds)                                                 # back from another setting: all rebuilt, on the plain path
    for i, w in enumerate(want):
        assert _bits(got_never[i], w) and _bits(pr.descriptor(i), w), i
        assert pr.window(i) == (i, i)
        assert _bits(pr.describe_submap([clouds[i]]), w), i                           # one cloud, no transform, through the submap kernel
        assert _bits(pr.describe_submap([clouds[i]], rel=[None]), w), i
    arch.set_poses(0, np.ones((5, 3)), np.tile([1.0, 0, 0, 0], (5, 1)))
    assert pr.update() == 0                                                           # the plain key holds no pose


# ---- 2. describe_submap against the model -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hard():
    return {(nr, ns): CS.hard_cloud(nr, ns, 80.0, 2.0, np.random.default_rng(1000 + nr)) for nr, ns in ((20, 60), (1, 4), (32, 64))}


def _split(rel):
    if rel is None:
        return None, None
    return [None if r is None else r[0] for r in rel], [None if r is None else r[1] for r in rel]


def _check(pr, clouds, rel, params, what):
    got = pr.describe_submap(clouds, rel=rel)
    want = SM.submap_describe(clouds, *_split(rel), **params)
    assert _bits(got, want), (what, np.argwhere(got != want)[:5])
    return want


@pytest.mark.parametrize("n_ring,n_sector", [(20, 60), (1, 4), (32, 64)])
def test_describe_submap_bit_for_bit(ctx, hard, n_ring, n_sector):
    rng = np.random.default_rng(7 + n_ring)
    h = hard[(n_ring, n_sector)]
    params = dict(n_ring=n_ring, n_sector=n_sector, max_radius=80.0, lidar_height=2.0)
    pr = L.PlaceRecognition(L.KeyframeArchive(ctx), **params)
    frame = L.place_frame(_pose(rng), 1)

    def rels(n, identity=()):
        return [None if i in identity else L.place_relative(frame, _pose(rng)) for i in range(n)]

    def cut(sizes):
        return [h[rng.integers(0, 5000 - m + 1):][:m].copy() for m in sizes]

    # lists of 1, 2, 3 and 81 clouds of mixed sizes; empty clouds first, last and in the middle
    for sizes in ([5000], [0], [1], [257, 64], [0, 5000], [63, 0, 65], [1, 257, 0], [0, 1, 63, 64, 65, 257, 5000] * 11 + [0, 64, 1, 0]):
        clouds = cut(sizes)
        assert len(clouds) in (1, 2, 3, 81)
        _check(pr, clouds, rels(len(clouds)), params, sizes[:8])
        _check(pr, clouds, rels(len(clouds), identity=(0, len(clouds) // 2)), params, ("identity", sizes[:8]))
    # totals around the tile: one row short of a tile, a tile, one row more, two tiles and a row
    for total in (T - 1, T, T + 1, 2 * T + 1):
        for sizes in ([total], [total - 700, 700], [1, total - 2, 1]):
            clouds = cut(sizes)
            _check(pr, clouds, rels(len(clouds)), params, ("total", total, sizes))
    # a tile that spans three segments (and more): the second tile starts in the first cloud and ends in the fifth
    clouds = cut([T + 100, 300, 0, 200, 5000])
    _check(pr, clouds, rels(5), params, "a tile across segments")
    clouds = cut([T - 3, 1, 1, 1, 1, 1, 64])
    _check(pr, clouds, rels(7), params, "a tile boundary among one-row segments")
    # a general rotation (0.3 rad about a skew axis) and its negated quaternion: the same rotation, the same bytes
    clouds = cut([5000, 257])
    t = np.array([3.25, -1.5, 0.4])
    a = _check(pr, clouds, [(_skew(0.3), t), (_skew(-0.3), -t)], params, "skew")
    b = _check(pr, clouds, [(-_skew(0.3), t), (-_skew(-0.3), -t)], params, "skew negated")
    assert _bits(a, b) and not _bits(a, SM.describe(np.concatenate(clouds), **params))


def test_a_transform_carries_rows_across_the_boundaries(ctx):
    """rows a translation carries out of max_radius and into it, across a ring boundary and across a sector boundary; non-finite rows stay skipped"""
    params = dict(n_ring=20, n_sector=60, max_radius=80.0, lidar_height=2.0)
    pr = L.PlaceRecognition(L.KeyframeArchive(ctx), **params)
    rng = np.random.default_rng(9)
    n = 400
    rows = np.zeros((4 * n + 4, 4), F)
    rows[:n, 0] = rng.uniform(79.8, 80.2, n)                                            # about max_radius, on the x axis
    rows[n:2 * n, 1] = rng.uniform(39.9, 40.1, n)                                       # about the boundary of rings 9 and 10, on the y axis
    a = math.radians(6.0 * 7)                                                           # about the boundary of sectors 6 and 7
    r = rng.uniform(20, 60, n)
    rows[2 * n:3 * n, 0], rows[2 * n:3 * n, 1] = r * math.cos(a), r * math.sin(a)
    rows[3 * n:4 * n, :2] = rng.uniform(-60, 60, (n, 2))
    rows[:4 * n, 2] = rng.uniform(-1, 6, 4 * n)
    with np.errstate(all="ignore"):
        rows[4 * n:, :3] = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [3e38, 3e38, 0]], F)
    tab = PM.tables(20, 60, 80.0)

    def cells(p):
        return [PM.cell_of(x, y, z, 20, 60, 80.0, tab) for x, y, z in p]

    ident = (np.array([1.0, 0, 0, 0]), np.zeros(3))
    still = _check(pr, [rows], [ident], params, "the identity as a transform")
    assert _bits(still, pr.describe_submap([rows]))                                      # ... is the identity flag's bytes
    before = cells(rows[:3 * n, :3])
    for t in ([0.15, 0.0, 0.0], [-0.15, 0.0, 0.0], [0.0, 0.08, 0.0], [0.0, -0.08, 0.0], [0.05, -0.05, 0.0]):
        rel = (np.array([1.0, 0, 0, 0]), np.array(t))
        moved = _check(pr, [rows], [rel], params, t)
        after = cells(SM.place_row(rows[:3 * n], *rel))
        crossed = [sum((b is None) != (c is None) for b, c in zip(before[lo:lo + n], after[lo:lo + n])) for lo in (0,)]
        ring = sum(b is not None and c is not None and b[1] != c[1] for b, c in zip(before[n:2 * n], after[n:2 * n]))
        sector = sum(b is not None and c is not None and b[0] != c[0] for b, c in zip(before[2 * n:], after[2 * n:]))
        assert (crossed[0] > 0 or t[0] == 0.0) and (ring > 0 or t[1] == 0.0) and sector > 0, (t, crossed, ring, sector)
        assert not _bits(moved, still)
    # rows near the largest f32: finite as they are, not once a rotation's sum has been rounded to f32 — skipped by the model and by the device alike
    far = np.array([[3e38, 3e38, 1.0, 0], [10.0, 10.0, 1.0, 0]], F)
    _check(pr, [far], [(_skew(0.3), np.zeros(3))], params, "overflow")


def test_describe_submap_memory_kinds(ctx, hard):
    params = dict(n_ring=20, n_sector=60, max_radius=80.0, lidar_height=2.0)
    pr = L.PlaceRecognition(L.KeyframeArchive(ctx), **params)
    rng = np.random.default_rng(21)
    h = hard[(20, 60)]
    clouds = [h[:257].copy(), h[300:300].copy(), h[1000:3100].copy(), h[4000:4065].copy()]
    frame = L.place_frame(_pose(rng), 0)
    rel = [L.place_relative(frame, _pose(rng)) for _ in clouds]
    rel[3] = None
    want = SM.submap_describe(clouds, *_split(rel), **params)
    keep = []
    kinds = [(m, s) for m in ("pageable", "pinned", "device") for s in (12, 16, 32)]
    for mem, stride in kinds:
        got = pr.describe_submap([_as_memory(c, mem, stride, keep) for c in clouds], rel=rel)
        assert _bits(got, want), (mem, stride)
    mixed = [_as_memory(c, *kinds[(3 * i + 1) % 9], keep) for i, c in enumerate(clouds)]          # every cloud of a list in another memory
    assert _bits(pr.describe_submap(mixed, rel=rel), want)
    # argument errors: nothing is written
    lib, out = ctx.lib, np.zeros((60, 20), F)
    arr = (L.api.Cloud * 82)(*([L.api.cloud_from_numpy(clouds[0], aux_col=3)] * 82))
    q, t = np.tile([1.0, 0, 0, 0], (82, 1)), np.zeros((82, 3))
    for n_c, qq, tt in ((0, q, t), (82, q, t), (2, q, None), (2, None, t)):
        assert lib.lili_place_describe_submap(ctx.h, arr, n_c, L.api._ptr(qq), L.api._ptr(tt), C.byref(pr.params), L.api._ptr(out)) != 0
    q[1, 2] = np.nan
    assert lib.lili_place_describe_submap(ctx.h, arr, 2, L.api._ptr(q), L.api._ptr(t), C.byref(pr.params), L.api._ptr(out)) != 0
    assert lib.lili_place_describe_submap(ctx.h, None, 2, None, None, C.byref(pr.params), L.api._ptr(out)) != 0
    assert not out.any()


# ---- 3. the archive path and the rebuild rule ---------------------------------------------------------------------------------------------------------------------------

Q_BL, T_BL = L.loop.quat_from_matrix(CS.rz(2.0) @ CS.ry(1.0)), np.array([0.1, -0.05, 0.2])
SMALL = dict(n_ring=20, n_sector=60, max_radius=80.0, lidar_height=2.0)


def _keyframes(seed, n=8):
    """n keyframes: (rows, body pose t, q) — a few hundred rows each (one of them empty), tilted poses a few metres apart"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = (300, 0, 65, 700, 1, 257, 450, 64)[i % 8]
        rows = np.concatenate([rng.uniform(-70, 70, (m, 2)), rng.uniform(-2, 8, (m, 1)), rng.uniform(0, 1, (m, 1))], 1).astype(F)
        p = _pose(rng)
        p[:2] = [3.0 * i, rng.uniform(-1, 1)]
        out.append((rows, p[:3], p[3:]))
    return out


def _model(pr, clouds, back, fwd, level, params=SMALL):
    """(keys, descriptors) of the archive as it is, from the library's own frames and relative placements"""
    poses = np.array([pr.map_pose(i) for i in range(len(clouds))])
    return (SM.keys(poses, back, fwd, level, rel=L.place_relative, frm=L.place_frame),
            SM.archive_describe(clouds, poses, back, fwd, level, rel=L.place_relative, frm=L.place_frame, **params))


def _check_archive(pr, clouds, old_keys, back, fwd, level):
    keys, want = _model(pr, clouds, back, fwd, level)
    built = pr.update()
    assert built == len(SM.expected_rebuilds(old_keys, keys)), (built, SM.expected_rebuilds(old_keys, keys))
    assert pr.info()[0] == len(clouds)
    for i, w in enumerate(want):
        assert _bits(pr.descriptor(i), w), (i, np.argwhere(pr.descriptor(i) != w)[:5])
    assert [pr.window(i) for i in range(len(clouds))] == SM.windows(len(clouds), back, fwd)
    return keys


@pytest.mark.parametrize("level", [0, 1])
def test_archive_path_and_rebuild_rule(ctx, level):
    kfs = _keyframes(31 + level)
    arch = L.KeyframeArchive(ctx, q_bl=Q_BL, t_bl=T_BL)
    pr = L.PlaceRecognition(arch, back=2, fwd=1, level=level, **SMALL)
    clouds, keys = [], []
    for i, (rows, t, q) in enumerate(kfs):                                             # one push at a time: the new keyframe and those whose window it enters
        arch.push(None, None, rows, float(i), t, q)
        clouds.append(rows)
        keys = _check_archive(pr, clouds, keys, 2, 1, level)
        assert pr.update() == 0
    one_by_one = [pr.descriptor(i) for i in range(8)]
    # set_poses of one keyframe: exactly the descriptors whose windows hold it; the same bytes again: none
    ts, qs, _ = arch.poses()
    t4 = ts[4] + [0.5, -0.25, 0.1]
    arch.set_poses(4, t4[None], qs[4][None])
    assert SM.expected_rebuilds(keys, _model(pr, clouds, 2, 1, level)[0]) == [3, 4, 5, 6]
    keys = _check_archive(pr, clouds, keys, 2, 1, level)
    arch.set_poses(4, t4[None], qs[4][None])
    arch.set_poses(0, *arch.poses()[:2])
    assert pr.update() == 0
    # another extrinsic: every relative placement changes, all rebuilt
    arch.set_extrinsic(T_BL + [0.0, 0.3, 0.0], L.loop.quat_from_matrix(CS.rz(-3.0) @ CS.ry(2.0)))
    assert len(SM.expected_rebuilds(keys, _model(pr, clouds, 2, 1, level)[0])) == 8
    keys = _check_archive(pr, clouds, keys, 2, 1, level)
    # another setting: all dropped, all rebuilt
    pr2 = L.PlaceRecognition(arch, back=1, fwd=0, level=level, **SMALL)
    _check_archive(pr2, clouds, [], 1, 0, level)
    assert pr.update() == 8
    # argument errors leave the descriptors and the setting as they were
    before = [pr.descriptor(i) for i in range(8)]
    for bad in (dict(back=65), dict(fwd=17), dict(level=2), dict(back=-1), dict(fwd=-1), dict(level=-1)):
        with pytest.raises(L.LiliError):
            L.PlaceRecognition(arch, **bad, **SMALL).update()
        sub = L.api.PlaceSubmap()
        ctx._chk(ctx.lib.lili_place_get_submap(ctx.h, C.byref(sub)))
        assert (sub.back, sub.fwd, sub.level) == (2, 1, level) and pr.info()[0] == 8
    for kid in (8, -1):
        with pytest.raises(L.LiliError):
            pr.window(kid)
    assert all(_bits(pr.descriptor(i), before[i]) for i in range(8)) and pr.update() == 0
    # the archive's reset drops all
    arch.reset()
    assert pr.info()[0] == 0
    with pytest.raises(L.LiliError):
        pr.window(0)
    # the same keyframes described in ONE update: the bytes of one push at a time (at the first extrinsic and poses)
    arch.set_extrinsic(T_BL, Q_BL)
    for i, (rows, t, q) in enumerate(kfs):
        arch.push(None, None, rows, float(i), t, q)
    assert pr.update() == 8
    assert all(_bits(pr.descriptor(i), one_by_one[i]) for i in range(8))


def test_an_absent_kind_inside_a_window(ctx):
    kfs = _keyframes(41, 5)
    arch = L.KeyframeArchive(ctx)
    clouds = []
    for i, (rows, t, q) in enumerate(kfs):
        full = None if i == 2 else rows
        arch.push(rows[:10], None, full, float(i), t, q)
        clouds.append(full)
    for level in (0, 1):
        pr = L.PlaceRecognition(arch, back=2, fwd=1, level=level, **SMALL)
        _check_archive(pr, clouds, [], 2, 1, level)
        assert pr.window(2) == (0, 3) and pr.descriptor(2).any()                      # keyframe 2 has no cloud of its own: its neighbours' rows describe it


def test_same_bytes_on_two_contexts_and_two_runs(ctx):
    kfs = _keyframes(51)
    got = []
    other = L.Context(0)
    for c in (ctx, ctx, other):
        arch = L.KeyframeArchive(c, q_bl=Q_BL, t_bl=T_BL)
        arch.reset()
        for i, (rows, t, q) in enumerate(kfs):
            arch.push(None, None, rows, float(i), t, q)
        pr = L.PlaceRecognition(arch, back=2, fwd=1, level=1, **SMALL)
        assert pr.update() == 8
        got.append(b"".join(pr.descriptor(i).tobytes() for i in range(8)))
    other.close()
    assert got[0] == got[1] == got[2]


# ---- 4. the wedge scene: search and the loop end to end ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wedge():
    return CS.wedge_scene(77, 12.0)


def _push_wedge(arch, sc):
    R_bl = L.loop._matrix_from_quat(Q_BL)
    for k, (t_o, R_o) in enumerate(sc["odo"]):
        rows = sc["rows"][k]
        R_po = R_o @ R_bl.T                                                             # the body pose whose LiDAR map pose is (R_o, t_o)
        arch.push(rows[::9].copy(), np.delete(rows, np.s_[::9], 0).copy(), rows, sc["times"][k], t_o - R_po @ T_BL, L.loop.quat_from_matrix(R_po))


def _true_distance(sc, c):
    return float(np.linalg.norm(sc["true"][c][0][:2] - sc["true"][CS.QUERY][0][:2]))


def test_search_over_the_wedge_scene(ctx, wedge):
    sc = wedge
    arch = L.KeyframeArchive(ctx, q_bl=Q_BL, t_bl=T_BL)
    _push_wedge(arch, sc)
    pr = L.PlaceRecognition(arch, back=CS.BACK, fwd=CS.FWD, level=True, **CS.PARAMS)
    n = CS.N1 + CS.N2
    assert pr.update() == n
    _, descs = _model(pr, sc["rows"], CS.BACK, CS.FWD, 1, CS.PARAMS)
    for i in range(n):
        assert _bits(pr.descriptor(i), descs[i]), i
    queries, k = [CS.QUERY, 70, 30, n - 1], 4
    got = pr.search(queries, k=k, min_time_gap=25.0, max_id=list(queries))
    for q, hits in zip(queries, got):
        want = PM.search(descs, sc["times"], descs[q], k + 1, q_id=q, q_time=sc["times"][q], min_time_gap=25.0, max_id=q)
        for a, b in zip(want, want[1:]):
            assert b[2] - a[2] > 1e-9, ("the model's ranking is too close to call", q, a, b)
        want = want[:k]
        for c, s, d in want:
            ds = np.sort(PM.shift_distances(descs[q], descs[c]))
            assert ds[1] - ds[0] > 1e-9, ("the model's shift is too close to call", q, c)
        assert [(c, s) for c, s, _ in hits] == [(c, s) for c, s, _ in want], (q, hits, want)
        assert all(abs(g[2] - w[2]) <= 1e-12 for g, w in zip(hits, want)), (q, hits, want)


def test_a_reverse_revisit_through_a_wedge(ctx, wedge):
    """The assertions stop at the guess.  On this scene the ICP does not meet lc_icp_thres = 0.2 even when it starts from the TRUE transform: the sensor, pitched
    12 degrees down, sees the ground and the lowest two metres of the walls, one reverse wedge overlaps the forward-looking target keyframes only partly, and the
    registration slides along the ground.  Measured on the MI355X, fitness from the true transform / from the guess: livox (one source keyframe) 0.463 / 0.611,
    rot (six source keyframes) 0.558 / 0.417, rot with lc_map_width 25 0.502 / 0.395.  That is the scene, not the descriptor."""
    sc = wedge
    n, latest = CS.N1 + CS.N2, CS.QUERY
    arch = L.KeyframeArchive(ctx, q_bl=Q_BL, t_bl=T_BL)
    lc = L.LoopClosure(ctx, variant="livox", lc_map_width=20, q_bl=Q_BL, t_bl=T_BL, archive=arch)
    _push_wedge(arch, sc)
    assert n - lc.slide_window_width == latest
    # the model decides what is a match: max_distance lies midway between its best candidate and its best candidate more than 6 m from the truth
    pr = L.PlaceRecognition(arch, back=CS.BACK, fwd=CS.FWD, level=True, **CS.PARAMS)
    _, descs = _model(pr, sc["rows"], CS.BACK, CS.FWD, 1, CS.PARAMS)
    ranked = PM.search(descs, sc["times"], descs[latest], n, q_id=latest, q_time=sc["times"][latest], min_time_gap=lc.global_lc_time_thres, max_id=latest)
    m_his, m_shift, m_d = ranked[0]
    m_far = min(d for c, _, d in ranked if _true_distance(sc, c) > 6.0)
    max_distance = 0.5 * (m_d + m_far)
    assert abs(m_his - CS.MATCH) <= 1 and abs(m_shift - 30) <= 1 and m_far - m_d > 0.03
    # today's descriptor — one keyframe, in the LiDAR frame as it is — returns no keyframe within 6 m of the place
    plain = L.PlaceRecognition(arch, **CS.PARAMS)
    det0 = lc.detect_appearance(plain, max_distance=max_distance)
    assert det0 is None or _true_distance(sc, det0[1]) > 6.0, det0
    # the levelled submap returns the model's match
    det = lc.detect_appearance(pr, max_distance=max_distance)
    assert det is not None and det[:3] == (latest, m_his, m_shift) and abs(det[3] - m_d) <= 1e-12, (det, ranked[0])
    # the guess against the true correction D^-1: a pure yaw by construction of the levelled frames, within a sector and a half and 2.5 m at the query
    D_R, D_t = sc["D"]
    T_true = np.eye(4)
    T_true[:3, :3], T_true[:3, 3] = D_R.T, -D_R.T @ D_t
    G = pr.guess(latest, m_his, m_shift)
    assert np.abs(G[2, :3] - [0, 0, 1]).max() <= 1e-12 and np.abs(G[:3, 2] - [0, 0, 1]).max() <= 1e-12
    dR = T_true[:3, :3].T @ G[:3, :3]
    d_yaw = abs(math.degrees(math.atan2(dR[1, 0], dR[0, 0])))
    p_q = np.append(sc["odo"][latest][0], 1.0)
    d_guess = float(np.linalg.norm((G @ p_q - T_true @ p_q)[:3]))
    print(f"model: match {ranked[0]}, best far {m_far:.4f}, max_distance {max_distance:.4f}; plain detector: {det0}; guess off by {d_yaw:.3f} deg, {d_guess:.3f} m")
    assert d_yaw <= 9.0 and d_guess <= 2.5, (d_yaw, d_guess)
    # perform(detector="appearance") needs nothing beyond place.guess: it starts the ICP from G on the submaps it assembled — the same bytes as align(G) on them
    out = lc.perform(None, None, None, sc["times"][latest], detector="appearance", place=pr, max_distance=max_distance)
    T_app, fit_app = lc.last["transform"].copy(), lc.last["fitness"]
    again = lc.align(G)
    assert again["transform"].tobytes() == T_app.tobytes() and again["fitness"] == fit_app
    assert out is None or out[:2] == (latest, m_his)
    ref = lc.align(T_true)
    print(f"ICP fitness from the guess {fit_app:.5f}, from the true transform {ref['fitness']:.5f} (lc_icp_thres {lc.lc_icp_thres})")
