"""Place recognition on the MI355X (lili_place_*, PlaceRecognition, LoopClosure.detect_appearance) against the numpy restatement
(tests/place_model.py): descriptors bit for bit, distances within 1e-12, ids and shifts exactly, and a loop 25 m and 90 degrees away from where the odometry
believes it to be, which the position search cannot see."""
import ctypes as C
import math

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd.archive import ARCHIVE_EDGE, ARCHIVE_FULL, ARCHIVE_SURF
from tests import place_model as PM

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the descriptor ----------------------------------------------------------------------------------------------------------------------------------------

def _r2(x, y):
    x, y = F(x), F(y)
    return F(F(x * x) + F(y * y))


def _hard_cloud(n_ring, n_sector, max_radius, lidar_height, rng, n=5000):
    """5 000 rows (x, y, z, aux) with every edge the definition names; the single-point cell is (sector of 200.5 degrees, the outermost ring)"""
    ring_r2, _, _ = PM.tables(n_ring, n_sector, max_radius)
    R = F(max_radius)
    rows = []
    for r in (0.5, 3.0, 17.25, 41.0, 63.5):                                    # both axes, both diagonals
        for x, y in ((r, 0), (0, r), (-r, 0), (0, -r), (r, r), (-r, r), (-r, -r), (r, -r), (r, -0.0), (-0.0, r)):
            rows.append([x, y, rng.uniform(-1, 5)])
    for k in range(1, n_ring):                                                 # r2 exactly a ring boundary squared: the inner ring's
        b = F(F(R * F(k)) / F(n_ring))
        assert _r2(b, 0) == ring_r2[k]
        rows += [[b, 0.0, 1.0 + 0.1 * k], [0.0, -b, 2.0 + 0.1 * k], [np.nextafter(b, F(np.inf)), 0.0, 3.0], [-np.nextafter(b, F(0)), 0.0, 0.5]]
    rows += [[0.0, 0.0, 4.0], [0.0, 0.0, -0.5], [-0.0, -0.0, 1.0]]             # r = 0
    max_r2 = F(R * R)
    found = {}
    for target, x in ((np.nextafter(max_r2, F(np.inf)), R), (np.nextafter(max_r2, F(0)), np.nextafter(R, F(0))), (max_r2, R)):
        for y in np.arange(0, 0.2, 1e-4, dtype=np.float64):                    # r2 one ulp outside / one ulp inside / exactly max_radius^2
            if _r2(x, y) == target:
                found[float(target)] = (float(x), float(F(y)))
                break
    assert len(found) == 3, found
    for x, y in found.values():
        rows += [[x, y, 9.0], [-y, x, 9.5]]
    rows += [[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [1, 1, np.inf], [1, 1, -np.inf]]
    for _ in range(40):                                                        # heights below -lidar_height, in cells of their own: negative cell values
        a, r = rng.uniform(0, math.pi), rng.uniform(0.93, 0.96) * max_radius
        rows.append([r * math.cos(a), r * math.sin(a), -lidar_height - rng.uniform(0.5, 4)])
    a0, r0 = math.radians(33.0), 0.41 * max_radius                             # many points in one cell
    for _ in range(600):
        rows.append([r0 * math.cos(a0) + rng.uniform(-0.05, 0.05), r0 * math.sin(a0) + rng.uniform(-0.05, 0.05), rng.uniform(-3, 7)])
    single = [0.985 * max_radius * math.cos(math.radians(200.5)), 0.985 * max_radius * math.sin(math.radians(200.5)), 6.25]
    rows.append(single)
    while len(rows) < n:                                                       # the bulk: inside 0.9 max_radius, away from the single point's cell
        a, r = rng.uniform(0, 2 * math.pi), max_radius * math.sqrt(rng.uniform(0, 0.81))
        rows.append([r * math.cos(a), r * math.sin(a), rng.normal(0.5, 2.0)])
    out = np.zeros((n, 4), F)
    with np.errstate(all="ignore"):
        out[:, :3] = np.array(rows[:n], np.float64).astype(F)
    out[:, 3] = rng.uniform(0, 255, n)
    rng.shuffle(out)
    return out, PM.cell_of(*[F(v) for v in single], n_ring, n_sector, max_radius, PM.tables(n_ring, n_sector, max_radius))


def _as_memory(rows, mem, stride, keep):
    """the rows as a lili_cloud in pageable, page-locked or device memory, 16- or 32-byte rows (aux behind the point / at byte 16)"""
    import torch
    if stride == 16:
        arr, aux = np.ascontiguousarray(rows), 3
    else:
        arr = np.random.default_rng(rows.shape[0]).uniform(-50, 50, (rows.shape[0], 8)).astype(F)
        arr[:, :3], arr[:, 4], aux = rows[:, :3], rows[:, 3], 4
    if mem == "pageable":
        keep.append(arr)
        return L.api.cloud_from_numpy(arr, aux_col=aux)
    if mem == "pinned":
        pa = L.api.PinnedArray(arr.shape)
        pa.array[:] = arr
        keep.append(pa)
        return L.api.Cloud(pa.array.ctypes.data, arr.shape[0], arr.shape[1] * 4, aux * 4, L.api.MEM_HOST)
    d = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    keep.append(d)
    return L.api.cloud_from_device(d.data_ptr(), arr.shape[0], arr.shape[1] * 4, aux * 4)


@pytest.mark.parametrize("n_ring,n_sector", [(20, 60), (1, 4), (32, 64)])
def test_descriptor_bit_for_bit(ctx, n_ring, n_sector):
    rng = np.random.default_rng(1000 + n_ring)
    max_radius, h = 80.0, 2.0
    hard, single = _hard_cloud(n_ring, n_sector, max_radius, h, rng)
    clouds = [hard[:m].copy() for m in (0, 1, 63, 64, 65, 257)] + [hard]
    arch = L.KeyframeArchive(ctx)
    for i, c in enumerate(clouds):
        arch.push(None, None, c, float(i), [i, 0, 0], [1, 0, 0, 0])
    pr = L.PlaceRecognition(arch, n_ring=n_ring, n_sector=n_sector, max_radius=max_radius, lidar_height=h)
    assert pr.update() == len(clouds)
    want = [PM.describe(c, n_ring, n_sector, max_radius, h) for c in clouds]
    for i, w in enumerate(want):
        assert _bits(pr.descriptor(i), w), (i, np.argwhere(pr.descriptor(i) != w)[:5])
    w = want[-1]
    assert not want[0].any() and np.count_nonzero(want[1]) <= 1
    if n_ring > 1:
        assert (w < 0).any() and w[single] == F(6.25) + F(h)                   # cells below the sensor's foot; the single point's cell
    keep = []
    for mem in ("pageable", "pinned", "device"):
        for stride in (16, 32):
            for i in (3, 5, 6, 0):
                got = pr.describe(_as_memory(clouds[i], mem, stride, keep))
                assert _bits(got, want[i]), (mem, stride, i)
    assert _bits(pr.describe(hard[:, :3].copy()), w)                           # 12-byte rows


def test_absent_kind_and_other_kinds(ctx):
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(-60, 60, (300, 2)), rng.uniform(-2, 6, (300, 2))], 1).astype(F)
    b = np.concatenate([rng.uniform(-60, 60, (200, 2)), rng.uniform(-2, 6, (200, 2))], 1).astype(F)
    arch = L.KeyframeArchive(ctx)
    arch.push(a, b, None, 0.0, [0, 0, 0], [1, 0, 0, 0])
    arch.push(None, a, b, 1.0, [0, 0, 0], [1, 0, 0, 0])
    for kind, w0, w1 in ((ARCHIVE_FULL, None, b), (ARCHIVE_EDGE, a, None), (ARCHIVE_SURF, b, a)):
        pr = L.PlaceRecognition(arch, kind=kind)
        assert pr.update() == 2
        for i, w in enumerate((w0, w1)):
            want = np.zeros((60, 20), F) if w is None else PM.describe(w)
            assert _bits(pr.descriptor(i), want), (kind, i)


# ---- 2. bookkeeping --------------------------------------------------------------------------------------------------------------------------------------------

def _scene(rng, n_pts, n_ring=20, n_sector=60, max_radius=80.0):
    """bin-centred points in distinct random cells, as rows (x, y, z, 0)"""
    idx = rng.choice(n_ring * n_sector, n_pts, replace=False)
    pts = PM.bin_centre_points([(int(i) // n_ring, int(i) % n_ring) for i in idx], n_ring, n_sector, max_radius, rng)
    return np.concatenate([pts, np.zeros((n_pts, 1), F)], 1)


def _centred_descriptor(rows, n_ring=20, n_sector=60, max_radius=80.0, h=2.0):
    """the descriptor of bin-centred rows, written down directly: every point is alone in the cell it was made for"""
    d = np.zeros((n_sector, n_ring), F)
    for x, y, z in rows[:, :3].astype(np.float64):
        s = int(math.floor((math.atan2(y, x) % (2 * math.pi)) / (2 * math.pi) * n_sector))
        r = int(math.floor(math.hypot(x, y) / max_radius * n_ring))
        d[s, r] = F(F(z) + F(h))
    return d


def test_bookkeeping_and_argument_errors(ctx):
    rng = np.random.default_rng(4)
    lib = ctx.lib
    arch = L.KeyframeArchive(ctx)
    pr = L.PlaceRecognition(arch)
    scenes = [_scene(rng, 80) for _ in range(8)]
    assert pr.info()[0] == 0
    assert pr.search([_centred_descriptor(scenes[0])], times=0.0) == [[]]          # nothing described: no candidate
    for i in range(5):
        arch.push(None, None, scenes[i], float(i), [i, 0, 0], [1, 0, 0, 0])
    assert pr.update() == 5 and pr.update() == 0
    for i in range(5, 8):
        arch.push(None, None, scenes[i], float(i), [i, 0, 0], [1, 0, 0, 0])
    with pytest.raises(L.LiliError):
        pr.search([6])                                                             # archived, not described yet
    with pytest.raises(L.LiliError):
        pr.descriptor(6)
    assert pr.update() == 3
    for i in range(8):
        assert _bits(pr.descriptor(i), _centred_descriptor(scenes[i])), i
    n, p, used = pr.info()
    assert n == 8 and (p.n_ring, p.n_sector) == (20, 60) and used >= 8 * 4800 + 8 * 8
    assert used < 64 * 4800                                                        # (grows by half, not by slabs)
    arch_bytes = arch.info()[2]
    arch.set_poses(0, rng.normal(size=(8, 3)), np.tile([1.0, 0, 0, 0], (8, 1)))
    arch.set_extrinsic([0.1, 0.2, 0.3], [1, 0, 0, 0])
    assert pr.update() == 0 and pr.info()[2] == used and arch.info()[2] == arch_bytes      # (the store is not the archive's)
    before = [pr.descriptor(i) for i in range(8)]
    res_before = pr.search([0, 5], k=3, min_time_gap=-1.0)

    # argument errors: LILI_E_ARG, nothing changes
    def refuses(rc):
        assert rc != 0 and b"place_" in lib.lili_last_error(ctx.h)
    q = (L.api.PlaceQuery * 65)()
    m, f = (L.api.PlaceMatch * (65 * 17))(), (C.c_int * 65)()
    for i in range(65):
        q[i].id, q[i].max_id, q[i].time, q[i].min_time_gap = 0, 100, 0.0, -1.0
    refuses(lib.lili_place_search(ctx.h, q, 0, 1, m, f))
    refuses(lib.lili_place_search(ctx.h, q, 65, 1, m, f))
    refuses(lib.lili_place_search(ctx.h, q, 1, 0, m, f))
    refuses(lib.lili_place_search(ctx.h, q, 1, 17, m, f))
    refuses(lib.lili_place_search(ctx.h, None, 1, 1, m, f))
    q[1].id = 8
    refuses(lib.lili_place_search(ctx.h, q, 2, 1, m, f))
    q[1].id = -2
    refuses(lib.lili_place_search(ctx.h, q, 2, 1, m, f))
    q[1].id, q[1].desc = -1, None
    refuses(lib.lili_place_search(ctx.h, q, 2, 1, m, f))
    q[1].id, q[1].time = 1, float("nan")
    refuses(lib.lili_place_search(ctx.h, q, 2, 1, m, f))
    for n_ring, n_sector, rad in ((0, 60, 80.0), (33, 60, 80.0), (20, 62, 80.0), (20, 68, 80.0), (20, 60, -1.0)):
        bad = L.api.PlaceParams(n_ring, n_sector, rad, 2.0, ARCHIVE_FULL, 0)
        refuses(lib.lili_place_update(ctx.h, C.byref(bad), None))
        cl = L.api.cloud_from_numpy(scenes[0], aux_col=3)
        out = np.zeros((64, 32), F)
        refuses(lib.lili_place_describe(ctx.h, C.byref(cl), C.byref(bad), L.api._ptr(out)))
        assert not out.any()
    bad_kind = L.api.PlaceParams(20, 60, 80.0, 2.0, 3, 0)
    refuses(lib.lili_place_update(ctx.h, C.byref(bad_kind), None))
    cl = L.api.cloud_from_numpy(scenes[0], aux_col=3)
    cl.stride = 10
    refuses(lib.lili_place_describe(ctx.h, C.byref(cl), C.byref(pr.params), L.api._ptr(np.zeros((60, 20), F))))
    refuses(lib.lili_place_describe(ctx.h, None, C.byref(pr.params), L.api._ptr(np.zeros((60, 20), F))))
    refuses(lib.lili_place_get(ctx.h, 8, L.api._ptr(np.zeros((60, 20), F))))
    refuses(lib.lili_place_get(ctx.h, -1, L.api._ptr(np.zeros((60, 20), F))))
    assert pr.info()[0] == 8 and pr.info()[2] == used
    assert all(_bits(pr.descriptor(i), before[i]) for i in range(8))
    assert pr.search([0, 5], k=3, min_time_gap=-1.0) == res_before

    # other parameters rebuild everything
    pr2 = L.PlaceRecognition(arch, n_ring=10, n_sector=24)
    assert pr2.update() == 8 and pr2.info()[0] == 8 and pr2.info()[1].n_sector == 24
    assert pr2.descriptor(7).shape == (24, 10)
    assert pr.update() == 8 and all(_bits(pr.descriptor(i), before[i]) for i in range(8))
    arch.reset()
    assert pr.info()[0] == 0
    assert pr.search([before[0]], k=4, times=0.0) == [[]]
    with pytest.raises(L.LiliError):
        pr.descriptor(0)
    arch.push(None, None, scenes[2], 0.0, [0, 0, 0], [1, 0, 0, 0])
    assert pr.update() == 1 and _bits(pr.descriptor(0), before[2])


# ---- 3. search against the model -------------------------------------------------------------------------------------------------------------------------------

N_BIG = 300
EMPTY_ID = 10


@pytest.fixture(scope="module")
def scenes300():
    return _scenes300()


def _scenes300():
    """300 random scenes of 50 .. 600 bin-centred points (scene EMPTY_ID: no point) with their descriptors, and 17 queries: archived ids, perturbed copies of archived scenes
    and scenes of their own"""
    rng = np.random.default_rng(20260)
    rows = [_scene(rng, int(rng.integers(50, 601))) for _ in range(N_BIG)]
    rows[EMPTY_ID] = np.zeros((0, 4), F)
    descs = [_centred_descriptor(r) for r in rows]
    queries = []
    for j in range(17):
        if j % 3 == 0:
            queries.append(int(rng.integers(0, 60)) if j < 9 else int(rng.integers(66, N_BIG)))      # an archived keyframe (of the small archives too)
        elif j % 3 == 1:
            d = np.roll(descs[int(rng.integers(0, N_BIG))], int(rng.integers(0, 60)), axis=0).copy()   # a revisit: turned, some cells changed, some gone
            mask = rng.uniform(size=d.shape) < 0.15
            d[mask] = (rng.uniform(-1, 8, d.shape) * (rng.uniform(size=d.shape) < 0.5)).astype(F)[mask]
            queries.append(d)
        else:
            queries.append(_centred_descriptor(_scene(rng, int(rng.integers(50, 601)))))
    queries[1][::2] = 0                                                                              # a query with many empty sectors
    return rows, descs, queries


def _check_search(pr, descs, times, queries, k, cache, **kw):
    """device against model: ids and shifts equal, distances within 1e-12 — after the model alone has shown that the ranking and the shifts are decided by more than 1e-9"""
    n = len(descs)
    q_times = [times[q] if isinstance(q, int) else 1000.0 for q in queries]
    got = pr.search(queries, k=k, times=q_times, **kw)
    gap = kw.get("min_time_gap", 0.0)
    max_id = kw.get("max_id", None)
    for qi, q in enumerate(queries):
        qd = descs[q] if isinstance(q, int) else q
        want = PM.search(descs, times, qd, k + 1, q_id=q if isinstance(q, int) else -1, q_time=q_times[qi], min_time_gap=gap,
                         max_id=2 ** 31 - 1 if max_id is None else max_id, cache=cache)
        for a, b in zip(want, want[1:]):
            assert b[2] - a[2] > 1e-9, ("the model's ranking is too close to call", qi, a, b)
        want = want[:k]
        for c, s, d in want:
            ds = np.sort(PM.shift_distances(qd, descs[c]))
            assert ds[1] - ds[0] > 1e-9, ("the model's shift is too close to call", qi, c)
        assert len(got[qi]) == len(want), (n, qi, len(got[qi]), len(want))
        assert [(c, s) for c, s, _ in got[qi]] == [(c, s) for c, s, _ in want], (n, qi, got[qi], want)
        for g, w in zip(got[qi], want):
            assert abs(g[2] - w[2]) <= 1e-12, (n, qi, g, w)
    return got


def test_search_against_the_model(ctx, scenes300):
    rows, descs, queries = scenes300
    times = [float(i) for i in range(N_BIG)]
    arch = L.KeyframeArchive(ctx)
    pr = L.PlaceRecognition(arch)
    cache = {}
    plan = {1: [(1, 1)], 2: [(3, 16)], 63: [(17, 5)], 64: [(3, 1)], 65: [(1, 16), (17, 1)], N_BIG: [(1, 1), (3, 5), (17, 16)]}
    for i in range(N_BIG):
        arch.push(None, None, rows[i], times[i], [i, 0, 0], [1, 0, 0, 0])
        n = i + 1
        if n not in plan:
            continue
        had = pr.info()[0]
        assert pr.update() == n - had and pr.info()[0] == n
        for n_q, k in plan[n]:
            qs = [q for q in queries if not isinstance(q, int) or q < n][:n_q]
            if n <= 2:
                qs = ([0] + [q for q in queries if not isinstance(q, int)])[:n_q]      # (the archived query of a one-keyframe archive has no candidate)
            got = _check_search(pr, descs[:n], times, qs, k, cache, min_time_gap=-1.0)
            if n == 1:
                assert got == [[]]
            if n == 2:
                assert [len(g) for g in got] == [1, 2, 2]                              # k = 16 > the eligible count
    # the all-zero descriptor is never reported, whatever k
    all_hits = pr.search([q for q in queries if not isinstance(q, int)][:3], k=16, min_time_gap=-1.0, times=1000.0)
    assert all(c != EMPTY_ID for hits in all_hits for c, _, _ in hits) and not descs[EMPTY_ID].any()
    # eligibility: the time gap on both sides of the threshold (times are whole seconds: |dt| = 7 is exact), max_id, both
    q_arch = [q for q in queries if isinstance(q, int)][:3]
    for gap in (7.0, np.nextafter(7.0, 0.0), 6.5):
        got = _check_search(pr, descs, times, q_arch, 16, cache, min_time_gap=gap)
        for q, hits in zip(q_arch, got):
            assert all(abs(times[c] - times[q]) > gap for c, _, _ in hits)
    got7 = pr.search([150], k=16, min_time_gap=148.0)[0]
    assert sorted(c for c, _, _ in got7) == [0, 1, 299]                                # |dt| = 148 (ids 2, 298) is not > 148
    got7 = pr.search([150], k=16, min_time_gap=np.nextafter(148.0, 0.0))[0]
    assert sorted(c for c, _, _ in got7) == [0, 1, 2, 298, 299]
    for max_id in (0, 40, 41, N_BIG - 1, N_BIG + 5):
        got = _check_search(pr, descs, times, queries[:5], 5, cache, min_time_gap=-1.0, max_id=max_id)
        assert all(c <= max_id for hits in got for c, _, _ in hits)
    assert pr.search([41], k=16, min_time_gap=-1.0, max_id=-1) == [[]]
    got = pr.search([41, 41], k=16, min_time_gap=-1.0, max_id=[40, 41])
    assert got[0] == got[1] and len(got[0]) == 16                                      # (the query itself is no candidate)
    assert sorted(c for c, _, _ in _check_search(pr, descs, times, [3], 16, cache, min_time_gap=-1.0, max_id=5)[0]) == [0, 1, 2, 4, 5]


# ---- 4. position and batch independence -----------------------------------------------------------------------------------------------------------------------

def _raw(hits):
    return np.array([(c, s, d) for c, s, d in hits], np.dtype([("c", "i4"), ("s", "i4"), ("d", "f8")])).tobytes()


def test_position_and_batch_independence(ctx, scenes300):
    rows, descs, queries = scenes300
    arch = L.KeyframeArchive(ctx)
    pr = L.PlaceRecognition(arch)
    order = list(range(100, 171))
    order[3] = order[70] = 7                                                           # the same cloud at ids 3 and 70
    for i, s in enumerate(order):
        arch.push(None, None, rows[s], float(i), [i, 0, 0], [1, 0, 0, 0])
    assert pr.update() == 71
    ext = [q for q in queries if not isinstance(q, int)]
    turned = np.roll(descs[7], 11, axis=0).copy()
    turned[5] = 0
    for q in (turned, ext[0], 20):
        hits = pr.search([q], k=16, min_time_gap=-1.0, times=500.0)[0]
        all71 = {}
        for lo in range(0, 71, 8):                                                     # every pair's (shift, distance) by restricting the candidates to eight at a time
            for c, s, d in pr.search([q], k=16, min_time_gap=float(lo) - 0.5, max_id=lo + 7, times=0.0)[0]:
                all71[c] = (s, d)
        assert all71[3] == all71[70] and np.float64(all71[3][1]).tobytes() == np.float64(all71[70][1]).tobytes()
        for c, s, d in hits:
            assert all71[c] == (s, d)
    hits = pr.search([turned], k=2, min_time_gap=-1.0, times=500.0)[0]
    assert [c for c, _, _ in hits] == [3, 70] and hits[0][1:] == hits[1][1:] and hits[0][1] == (60 - 11) % 60      # equal distances: id order
    batch = [ext[j % len(ext)] if j % 2 else (j * 3) % 71 for j in range(17)]
    batch[9] = turned
    t_b = [500.0 if not isinstance(q, int) else float(q) for q in batch]
    together = pr.search(batch, k=16, min_time_gap=3.0, times=t_b)
    for j in (0, 9, 16):
        alone = pr.search([batch[j]], k=16, min_time_gap=3.0, times=[t_b[j]])[0]
        assert _raw(alone) == _raw(together[j])
    again = pr.search(batch, k=16, min_time_gap=3.0, times=t_b)
    assert [_raw(h) for h in again] == [_raw(h) for h in together]


# ---- 5. the shift ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_every_whole_sector_rotation_is_found_at_its_shift(ctx):
    rng = np.random.default_rng(55)
    base = _scene(rng, 240)
    arch = L.KeyframeArchive(ctx)
    arch.push(None, None, base, 0.0, [0, 0, 0], [1, 0, 0, 0])
    for s in range(60):
        a = 2 * math.pi * s / 60
        rot = base.copy()
        rot[:, :3] = (base[:, :3].astype(np.float64) @ np.array([[math.cos(a), math.sin(a), 0], [-math.sin(a), math.cos(a), 0], [0, 0, 1]])).astype(F)
        arch.push(None, None, rot, 1.0 + s, [0, 0, 0], [1, 0, 0, 0])
    pr = L.PlaceRecognition(arch)
    assert pr.update() == 61
    d0 = pr.descriptor(0)
    assert _bits(d0, _centred_descriptor(base))
    ds = np.sort(PM.shift_distances(d0, d0))
    assert ds[0] <= 1e-12 and ds[1] > 1e-3                                             # rotationally asymmetric: one shift only brings it onto itself
    for s in range(60):
        assert _bits(pr.descriptor(1 + s), np.roll(d0, s, axis=0)), s
    # every rotation as a query against the unturned scene alone: it is the query turned BACK by s sectors
    got = pr.search(list(range(1, 61)), k=1, min_time_gap=-1.0, max_id=0)
    for s, hits in enumerate(got):
        assert len(hits) == 1 and hits[0][0] == 0 and hits[0][1] == (60 - s) % 60 and hits[0][2] <= 1e-12, (s, hits)
    # and the unturned scene against every rotation: found at the rotation's own shift
    seen = {}
    for lo in range(1, 61, 12):
        for c, s, d in pr.search([0], k=16, min_time_gap=float(lo) - 0.5, max_id=lo + 11, times=0.0)[0]:
            seen[c] = (s, d)
    assert sorted(seen) == list(range(1, 61))
    for c, (s, d) in seen.items():
        assert s == c - 1 and d <= 1e-12, (c, s, d)


# ---- 6. end to end: a loop the position search cannot see ------------------------------------------------------------------------------------------------------------

def _rz(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])


def _street(rng):
    """walls (various lengths and heights) and poles along a street, every structure at least 2 m from the next, and the ground: (structures, ground sampler)"""
    walls, poles = [], []
    x = -20.0
    while x < 100.0:
        for side in (-1, 1):
            length, height, off = rng.uniform(3, 9), rng.uniform(2.5, 9), rng.uniform(7, 16)
            if rng.uniform() < 0.75:
                walls.append((x, side * off, x + length, side * off + rng.uniform(-1.5, 1.5), height))
            if rng.uniform() < 0.6:
                poles.append((x + length + 1.0 + rng.uniform(0, 1), side * (off - 3.0 - rng.uniform(0, 2)), rng.uniform(3, 10)))
        x += 12.0
    return walls, poles


def _sample_street(street, rng, spacing=0.3):
    walls, poles = street
    out = []
    for x0, y0, x1, y1, h in walls:
        n_u, n_v = int(math.hypot(x1 - x0, y1 - y0) / spacing), int(h / spacing)
        u, v = np.meshgrid((np.arange(n_u) + 0.5) / n_u, (np.arange(n_v) + 0.5) / n_v, indexing="ij")
        u, v = u.ravel() + rng.uniform(-0.3, 0.3, u.size) / n_u, v.ravel() + rng.uniform(-0.3, 0.3, v.size) / n_v
        out.append(np.stack([x0 + u * (x1 - x0), y0 + u * (y1 - y0), v * h], 1))
    for px, py, h in poles:
        n = int(h / 0.1) * 6
        a, z = rng.uniform(0, 2 * math.pi, n), rng.uniform(0, h, n)
        out.append(np.stack([px + 0.15 * np.cos(a), py + 0.15 * np.sin(a), z], 1))
    gx, gy = np.meshgrid(np.arange(-50, 130, 0.8), np.arange(-40, 40, 0.8), indexing="ij")
    g = np.stack([gx.ravel() + rng.uniform(-0.25, 0.25, gx.size), gy.ravel() + rng.uniform(-0.25, 0.25, gx.size), np.zeros(gx.size)], 1)
    out.append(g)
    return np.concatenate(out)


def _scan(world, t, R, radius=30.0, seed=0):
    """the world's points within `radius` of the LiDAR at (t, R), in its frame: rows (x, y, z, aux)"""
    sel = world[np.linalg.norm(world[:, :2] - t[:2], axis=1) < radius]
    loc = ((sel - t) @ R).astype(F)
    return np.concatenate([loc, np.random.default_rng(seed).uniform(0, 1, (loc.shape[0], 1)).astype(F)], 1)


def test_a_loop_the_position_search_cannot_see(ctx):
    rng = np.random.default_rng(77)
    street = _street(rng)
    pass1, pass2 = _sample_street(street, np.random.default_rng(1)), _sample_street(street, np.random.default_rng(2))      # a revisit never sees the same points
    R_bl, t_bl = _rz(2.0) @ np.array([[1, 0, 0], [0, math.cos(0.02), -math.sin(0.02)], [0, math.sin(0.02), math.cos(0.02)]]), np.array([0.1, -0.05, 0.2])
    q_bl = L.loop.quat_from_matrix(R_bl)
    arch = L.KeyframeArchive(ctx, q_bl=q_bl, t_bl=t_bl)
    lc = L.LoopClosure(ctx, variant="livox", lc_map_width=4, q_bl=q_bl, t_bl=t_bl, archive=arch)
    pr = L.PlaceRecognition(arch)
    h, n1 = 9, 30
    # LiDAR poses: pass 1 drives down the street; pass 2 comes back across it and stands where keyframe h stood, turned by 5 sectors (30 degrees) and 0.2 m aside
    true = [(np.array([2.5 * k, 0.3 * math.sin(k / 3.0), 1.8]), _rz(4.0 * math.sin(k / 5.0))) for k in range(n1)]
    t_h, R_h = true[h]
    back = [(t_h + np.array([4.0, 6.0, 0]), R_h @ _rz(-70.0)), (t_h + np.array([2.0, 3.0, 0]), R_h @ _rz(-40.0)),
            (t_h + np.array([0.15, -0.13, 0.0]), R_h @ _rz(30.0)), (t_h + np.array([-2.0, -1.0, 0]), R_h @ _rz(50.0)), (t_h + np.array([-4.5, -1.5, 0]), R_h @ _rz(60.0))]
    D_R, D_t = _rz(90.0), np.array([0.0, 0.0, 0.0])
    pivot = back[2][0]
    D_t = pivot + np.array([0.0, -25.0, 0.0]) - D_R @ pivot                              # the odometry of pass 2: 25 m aside (away from the street's keyframes) and 90 degrees of yaw
    poses = true + [(D_R @ t + D_t, D_R @ R) for t, R in back]                          # what the odometry believes
    worlds = [pass1] * n1 + [pass2] * len(back)
    for k, ((t_o, R_o), (t_w, R_w)) in enumerate(zip(poses, true + back)):
        rows = _scan(worlds[k], t_w, R_w, seed=k)
        R_po = R_o @ R_bl.T                                                             # body pose whose LiDAR map pose (q_po q_bl, q_po t_bl + t_po) is (R_o, t_o)
        arch.push(rows[::9].copy(), np.delete(rows, np.s_[::9], 0).copy(), rows, 2.0 * k if k < n1 else 200.0 + 2.0 * k, t_o - R_po @ t_bl, L.loop.quat_from_matrix(R_po))
    n = len(poses)
    latest = n - lc.slide_window_width
    assert latest == n1 + 2
    ts_po, _, tm = arch.poses()
    assert np.linalg.norm(ts_po[:n1] - ts_po[latest], axis=1).min() > 20.0
    # today's detector: nothing within its 10 m
    assert lc.detect(None, None, ts_po[latest], tm[latest]) is None
    assert lc.perform(None, None, ts_po[latest], tm[latest]) is None
    det = lc.detect_appearance(pr, max_distance=0.4)
    assert det is not None and det[:3] == (latest, h, 5), det                            # the candidate's scan is the query's turned by +5 sectors
    assert lc.detect_appearance(pr, max_distance=det[3] * 0.5) is None
    assert lc.detect_appearance(pr, tm[latest], max_distance=0.4) == det
    out = lc.perform(None, None, None, tm[latest], detector="appearance", place=pr, max_distance=0.4)
    assert out is not None and out[:2] == (latest, h) and out[5] <= lc.lc_icp_thres
    T_app, n_it = lc.last["transform"].copy(), lc.last["iterations"]
    # the measure: the same submaps registered from the TRUE relative transform (what undoes the odometry's error)
    T_true = np.eye(4)
    T_true[:3, :3], T_true[:3, 3] = D_R.T, -D_R.T @ D_t
    ref = lc.align(T_true)
    assert ref["converged"] and ref["fitness"] <= lc.lc_icp_thres
    dT = np.linalg.inv(ref["transform"]) @ T_app
    p_latest = np.append(poses[latest][0], 1.0)
    d_pos = np.linalg.norm((T_app @ p_latest - ref["transform"] @ p_latest)[:3])
    d_ang = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(dT[:3, :3]) - 1.0) / 2.0))))
    print(f"appearance match: distance {det[3]:.4f}, shift {det[2]}; fitness {out[5]:.5f} (from the true transform {ref['fitness']:.5f}); "
          f"corrected pose differs by {d_pos:.5f} m, {d_ang:.5f} deg; ICP iterations {n_it} / {ref['iterations']}")
    assert d_pos <= 0.05 and d_ang <= 0.5, (d_pos, d_ang)
    # the corrected body pose is where the body truly stood
    assert np.linalg.norm(out[2][0] - (back[2][0] - (back[2][1] @ R_bl.T) @ t_bl)) < 0.3
