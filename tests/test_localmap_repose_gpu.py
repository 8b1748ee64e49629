"""lili_localmap_repose: the warm-up branch of buildLocalMapWithLandMark (L/src/BackendFusion.cpp:1407-1443) — while the ring holds fewer than local_map_width
keyframes the reference clears it on every keyframe and re-transforms every stored keyframe at the pose the sliding-window solve has just rewritten.

* repose + commit is the same map, bit for bit, as a reset and pushes at the new poses (changed sets: none, suffixes, everything, a non-suffix set; both sort paths);
* a suffix change is merged back as ONE incremental step (stats), a repose with the stored poses changes nothing;
* BackendKeyframes with repose during warm-up reproduces the reference's own maps (oracle/_ref/libref_localmap.so: the reference text compiled), and without it does not;
* repose + prepare equals repose + the separate calls bit for bit, both join modes;
* bad arguments leave the ring untouched."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import lili_om_amd as L

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(G, "make_ref_golden.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

E_ARG = -1
W6 = 6               # ring width of the direct LocalMap tests
K = 3                # slide_window_width
CHECK_SLOT = 5       # matcher slot the map checks use (outside the window's slots 0 .. K-1)


def _cloud(rng, n, sz):
    return np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.normal(0, sz, (n, 1)), rng.uniform(0, 25, (n, 1))], 1).astype(np.float32)


def _pose(rng, k):
    q = np.array([1.0, *rng.normal(0, 0.05, 3)]); q /= np.linalg.norm(q)
    return np.array([0.3 * k, -0.1 * k, 0.02 * k]) + rng.normal(0, 0.05, 3), q


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _commit_get(lms):
    out = []
    for lm in lms:
        n_raw, n_map = lm.commit()
        out.append((n_raw, n_map, lm.get(n_map + 1)))
    return out


def _same_maps(a, b):
    for (ra, ma, xa), (rb, mb, xb) in zip(a, b):
        assert (ra, ma) == (rb, mb)
        assert np.array_equal(_bits(xa), _bits(xb))


def _lms(ctx, width=W6):
    return [L.LocalMap(ctx, L.KIND_SURF, width=width, leaf=0.4), L.LocalMap(ctx, L.KIND_EDGE, width=width, leaf=0.2)]


def _repose_c(ctx, mask, t, q, n=None):
    t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1, 3)); q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, 4))
    return ctx.lib.lili_localmap_repose(ctx.h, mask, t.shape[0] if n is None else n, t.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p))


def _ring(rng, sizes):
    """Keyframes of `sizes` surf points (a quarter as many edge points) and their poses."""
    surf = [_cloud(rng, n, 0.3) for n in sizes]
    edge = [_cloud(rng, max(n // 4, 1), 1.0) for n in sizes]
    poses = [_pose(rng, k) for k in range(len(sizes))]
    return surf, edge, poses


def _ring_of_seven(rng, n_pts):
    """Seven keyframes pushed into a ring of six with a commit after each (the sorted ring is live, one keyframe has been popped)."""
    return _ring(rng, [n_pts] * 7)


def _feed(lms, surf, edge, poses, ks, commit=True):
    for k in ks:
        lms[0].push(surf[k], *poses[k]); lms[1].push(edge[k], *poses[k])
        if commit:
            _commit_get(lms)


# (ring width, changed ring positions, (incremental, full) commits of the two kinds together).  A changed set extends to the suffix from its first position; the suffix is
# merged back in one step per kind while it holds at most 8 keyframes and a keyframe in front of it stays.
CASES = {"none": (W6, [], (2, 0)), "last": (W6, [5], (2, 0)), "suffix3": (W6, [3, 4, 5], (2, 0)), "all": (W6, [0, 1, 2, 3, 4, 5], (0, 2)), "gaps": (W6, [1, 4], (2, 0)),
         "suffix8of9": (9, list(range(1, 9)), (2, 0)), "all9": (9, list(range(9)), (0, 2)), "suffix9of10": (10, list(range(1, 10)), (0, 2)), "last8": (8, [7], (2, 0))}
# surf points of the width + 1 keyframes pushed, where not the same for all: the sizes at which the merge switches routes (tests/test_voxel_gpu.py, _AT_THRESHOLD) —
# 65 536 old entries and 8 192 re-posed ones (flags fused into the scan, counting sort), 65 537 and 8 193 (flags in memory, radix sort)
SIZES = {"8x8192": [8192] * 9, "7x8192+8193": [8192] * 8 + [8193]}


@pytest.mark.parametrize("case,n_pts", [(c, n) for n in (1500, 12000) for c in CASES if c != "last8"] + [("last8", s) for s in SIZES],
                         ids=lambda v: str(v))
def test_repose_equals_reset_and_repush(n_pts, case):
    width, changed, commits = CASES[case]
    sizes = SIZES[n_pts] if n_pts in SIZES else [n_pts] * (width + 1)
    rng = np.random.default_rng(11 + sizes[0])
    surf, edge, poses = _ring(rng, sizes)
    ring = range(1, width + 1)                       # ring position j holds keyframe 1 + j
    ca, cb = L.Context(0), L.Context(0)
    try:
        la = _lms(ca, width)
        _feed(la, surf, edge, poses, range(width + 1))
        new = list(poses)
        for j in changed:
            new[1 + j] = _pose(rng, 1 + j)
        inc0, full0 = la[0].stats()
        assert _repose_c(ca, L.MASK_SURF | L.MASK_EDGE, [new[k][0] for k in ring], [new[k][1] for k in ring]) == L.api.OK
        ma = _commit_get(la)
        inc1, full1 = la[0].stats()
        assert (inc1 - inc0, full1 - full0) == commits
        cb.set_option("localmap_incremental", 0)
        lb = _lms(cb, width)
        _feed(lb, surf, edge, new, ring, commit=False)
        mb = _commit_get(lb)
        _same_maps(ma, mb)
        assert ma[0][0] == sum(surf[k].shape[0] for k in ring)
    finally:
        ca.close(); cb.close()


def test_repose_then_push_is_one_incremental_step_and_a_noop_repose_changes_nothing():
    rng = np.random.default_rng(5)
    surf, edge, poses = _ring_of_seven(rng, 3000)
    surf.append(_cloud(rng, 3000, 0.3)); edge.append(_cloud(rng, 750, 1.0)); poses.append(_pose(rng, 7))
    ca, cb = L.Context(0), L.Context(0)
    try:
        la = _lms(ca)
        _feed(la, surf, edge, poses, range(7))
        new = list(poses)
        for k in (4, 5, 6):
            new[k] = _pose(rng, k)
        inc0, full0 = la[0].stats()
        la[0].repose([new[k][0] for k in range(1, 7)], [new[k][1] for k in range(1, 7)])
        la[1].repose([new[k][0] for k in range(1, 7)], [new[k][1] for k in range(1, 7)])
        _feed(la, surf, edge, new, [7], commit=False)          # the joining keyframe pops keyframe 1
        ma = _commit_get(la)
        assert la[0].stats() == (inc0 + 2, full0)
        cb.set_option("localmap_incremental", 0)
        lb = _lms(cb)
        _feed(lb, surf, edge, new, range(2, 8), commit=False)
        _same_maps(ma, _commit_get(lb))
        # the stored poses again: nothing to re-transform, the next map is the same bit for bit
        assert _repose_c(ca, L.MASK_SURF | L.MASK_EDGE, [new[k][0] for k in range(2, 8)], [new[k][1] for k in range(2, 8)]) == L.api.OK
        _same_maps(ma, _commit_get(la))
        assert la[0].stats() == (inc0 + 4, full0)
    finally:
        ca.close(); cb.close()


# ---- the back end's warm-up against the reference's own text -------------------------------------------------------------------------------------------------------

def _schedule(i, seed=3):
    """Body poses (qw qx qy qz x y z) per call: before call c every keyframe of the previous window (the poses its solve rewrote) gets a new perturbation."""
    rng = np.random.default_rng(seed)
    n_kf = len(i["poses"])
    cur = np.array(i["poses"], np.float64)
    at = [cur.copy()]
    for c in range(1, n_kf):
        cur = cur.copy()
        for j in range(max(0, c - K), c):
            q = cur[j, :4] + rng.normal(0, 0.01, 4)
            cur[j, :4] = q / np.linalg.norm(q)
            cur[j, 4:7] += rng.normal(0, 0.03, 3)
        at.append(cur.copy())
    return at


def _assoc(P, pose, ks):
    out = [L.api.assoc_transform(pose[k][4:7], pose[k][:4], P) for k in ks]
    return [a[1] for a in out], [a[0] for a in out]


def _ring_poses(i, pose, ids):
    return L.api.keyframe_map_poses(pose[ids, 4:7], pose[ids, :4], i["t_bl"], i["q_bl"])


def _map_matches(m, kind, ref_map, n_map):
    """The criterion of test_gpu_local_map_vs_reference_backend: every reference point finds itself (same index), d^2 < 1e-11, >= 75 % exactly."""
    if n_map != ref_map.shape[0]:
        return False
    m.set_queries(CHECK_SLOT, kind, np.ascontiguousarray(ref_map[:, :3]))
    find = m.find_corresponding_surf_features if kind == L.KIND_SURF else m.find_corresponding_corner_features
    find(CHECK_SLOT, np.array([1.0, 0, 0, 0]), np.zeros(3))
    idx, d2 = m.neighbors(CHECK_SLOT, kind, ref_map.shape[0])
    return bool(np.array_equal(idx[:, 0], np.arange(ref_map.shape[0])) and d2[:, 0].max() < 1e-11 and (d2[:, 0] == 0).mean() > 0.75)


def _run_backend(i, at, repose, expected):
    """BackendKeyframes over the sequence (join_slot); per call >= 1 whether both maps match the reference's."""
    P = L.make_params("rot")
    W = M.LM_WIDTH
    ctx = L.Context(0)
    hits = []
    try:
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, P)
        bk = L.BackendKeyframes(ctx, P, leaf_surf=M.LM_SURF_LEAF, leaf_edge=M.LM_EDGE_LEAF, width=W)
        for c in range(len(i["surf"])):
            pose = at[c]
            win = list(range(max(0, c - K + 1), c + 1))
            ts, qs = _assoc(P, pose, win)
            join = None
            if c > 0:
                ring = min(c - 1, W)                        # keyframes the rings hold before the join
                if repose and 0 < ring < W:                 # the reference's recent_surf_keyframes.size() < local_map_width
                    bk.repose(*_ring_poses(i, pose, list(range(c - 1 - ring, c - 1))))
                tj, qj = L.api.keyframe_map_pose(pose[c - 1][4:7], pose[c - 1][:4], i["t_bl"], i["q_bl"])
                join = ((c - 1) % K, tj, qj)
            _, info = bk.prepare(join, i["surf"][c], i["edge"][c], [j % K for j in win], ts, qs)
            if c > 0:
                e = expected[c]
                hits.append(_map_matches(m, L.KIND_SURF, e["surf_map"], info["n_map"][0]) and _map_matches(m, L.KIND_EDGE, e["edge_map"], info["n_map"][1]))
    finally:
        ctx.close()
    return hits


def _expected_maps(i, at):
    """The reference's maps per call, each from a FRESH slice: keyframe j < c enters with the body pose the reference last read for it — the schedule's at call
    max(j + 1, min(c, width)) (warm-up calls re-read every stored pose, steady-state calls only the joining one's)."""
    R = M.R
    W = M.LM_WIDTH
    out = {}
    for c in range(1, len(i["surf"])):
        sl = R.LocalMapSlice(W, M.LM_SURF_MAP_LEAF, M.LM_EDGE_MAP_LEAF, M.LM_SURF_LEAF, M.LM_EDGE_LEAF, i["q_bl"], i["t_bl"])
        for j in range(c):
            sl.keyframe(i["surf"][j], i["edge"][j])
            sl.commit(at[max(j + 1, min(c, W))][j])
        out[c] = sl.keyframe(i["surf"][c], i["edge"][c])
        sl.close()
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(M.R.REF_DIR, "libref_localmap.so")), reason="oracle/_ref not built (needs /root/reference; build container only)")
def test_backend_warmup_with_repose_matches_the_reference():
    i = M.localmap_inputs(n_kf=8)
    at = _schedule(i)
    expected = _expected_maps(i, at)
    hits = _run_backend(i, at, True, expected)
    assert all(hits), hits
    assert not all(_run_backend(i, at, False, expected))      # the perturbations are visible: without repose the warm-up maps differ


@pytest.mark.parametrize("join_from_slot", [False, True])
def test_prepare_after_repose_equals_the_separate_calls(join_from_slot):
    i = M.localmap_inputs(n_kf=8)
    at = _schedule(i)
    W = M.LM_WIDTH
    P = L.make_params("rot")
    mask = L.MASK_SURF | L.MASK_EDGE
    ca, cb = L.Context(0), L.Context(0)
    try:
        ma = L.ScanToMapMatcher(ca, P)
        lm = [L.LocalMap(ca, L.KIND_SURF, width=W, leaf=M.LM_SURF_MAP_LEAF), L.LocalMap(ca, L.KIND_EDGE, width=W, leaf=M.LM_EDGE_MAP_LEAF, max_sq_radius=P.edge_gate)]
        mb = L.ScanToMapMatcher(cb, P)
        bk = L.BackendKeyframes(cb, P, leaf_surf=M.LM_SURF_LEAF, leaf_edge=M.LM_EDGE_LEAF, width=W)
        ds_prev = None
        reposed = 0
        for c in range(len(i["surf"])):
            pose = at[c]
            win = list(range(max(0, c - K + 1), c + 1))
            slots = [j % K for j in win]
            ts, qs = _assoc(P, pose, win)
            join = None
            if c > 0:
                ring = min(c - 1, W)
                tj, qj = L.api.keyframe_map_pose(pose[c - 1][4:7], pose[c - 1][:4], i["t_bl"], i["q_bl"])
                if 0 < ring < W:
                    tr, qr = _ring_poses(i, pose, list(range(c - 1 - ring, c - 1)))
                    lm[0].repose(tr, qr); lm[1].repose(tr, qr)
                    bk.repose(tr, qr)
                    reposed += 1
                lm[0].push(ds_prev[0], tj, qj); lm[1].push(ds_prev[1], tj, qj)
                sizes_a = (lm[0].commit(), lm[1].commit())
                join = ((c - 1) % K, tj, qj) if join_from_slot else (ds_prev[0], ds_prev[1], tj, qj)
            ds = [L.api.voxel_filter(ca, i["surf"][c], M.LM_SURF_LEAF)[0], L.api.voxel_filter(ca, i["edge"][c], M.LM_EDGE_LEAF)[0]]
            ma.set_queries(slots[-1], L.KIND_SURF, ds[0]); ma.set_queries(slots[-1], L.KIND_EDGE, ds[1])
            counts_a = ma.associate_window(slots, ts, qs, mask) if c > 0 else None
            counts_b, info = bk.prepare(join, i["surf"][c], i["edge"][c], slots, ts, qs)
            assert info["n_query"] == (ds[0].shape[0], ds[1].shape[0])
            if c > 0:
                assert info["associated"] and counts_b == counts_a, (c, counts_a, counts_b)
                assert (info["n_map_raw"][0], info["n_map"][0]) == sizes_a[0] and (info["n_map_raw"][1], info["n_map"][1]) == sizes_a[1]
                for s in slots:
                    ra, rb = ma.surf_records(s, 4096), mb.surf_records(s, 4096)
                    for key in ("query_index", "cp", "n", "d", "score"):
                        assert np.array_equal(ra[key], rb[key]), (c, s, key)
                    ea, eb = ma.edge_records(s, 4096), mb.edge_records(s, 4096)
                    for key in ("query_index", "cp", "a", "b", "s"):
                        assert np.array_equal(ea[key], eb[key]), (c, s, key)
            ds_prev = ds
        assert reposed == W - 1
    finally:
        ca.close(); cb.close()


def test_repose_rejects_bad_arguments():
    rng = np.random.default_rng(9)
    surf, edge, poses = _ring_of_seven(rng, 800)
    ctx = L.Context(0)
    try:
        lms = _lms(ctx)
        _feed(lms, surf, edge, poses, range(3), commit=False)
        m0 = _commit_get(lms)
        t, q = [p[0] for p in poses[3:6]], [p[1] for p in poses[3:6]]
        assert _repose_c(ctx, L.MASK_SURF | L.MASK_EDGE, t, q, n=2) == E_ARG          # n differs from the ring size
        assert _repose_c(ctx, L.MASK_SURF, t, q, n=4) == E_ARG
        assert _repose_c(ctx, 0, t, q) == E_ARG                                        # empty mask
        assert ctx.lib.lili_localmap_repose(ctx.h, L.MASK_SURF, 3, None, None) == E_ARG   # null pointers
        _same_maps(m0, _commit_get(lms))
        # surf and edge rings of different sizes (4 and 3) under a two-kind mask
        lms[0].push(surf[3], *poses[3])
        m1 = _commit_get(lms)
        t4, q4 = [p[0] for p in poses[2:6]], [p[1] for p in poses[2:6]]
        assert _repose_c(ctx, L.MASK_SURF | L.MASK_EDGE, t4, q4) == E_ARG
        assert _repose_c(ctx, L.MASK_SURF | L.MASK_EDGE, t, q) == E_ARG
        _same_maps(m1, _commit_get(lms))
    finally:
        ctx.close()
