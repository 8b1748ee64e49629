"""CPU side of the keyframe archive / global map: the exactness argument of the accumulating voxel table on a numpy model, lili_loop_detect
against LoopClosure.detect, and the boundary of the new functions.  Everything bit for bit."""
import ctypes as C
import os
import re
import types

import numpy as np

import lili_om_amd as L
from tests import global_map_model as G
from tests import voxel_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["lili_archive_reset", "lili_archive_set_extrinsic", "lili_archive_push", "lili_archive_push_slot", "lili_archive_set_poses", "lili_archive_info", "lili_archive_pose",
       "lili_archive_get", "lili_archive_view", "lili_loop_cloud_archive", "lili_loop_detect", "lili_global_map", "lili_global_map_get", "lili_global_map_stats",
       "lili_global_map_info"]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_splits(cloud, leaf, rng, n_batches_list):
    want, want_n = V.voxel_grid(cloud, leaf)
    for nb in n_batches_list:
        cuts = np.sort(rng.integers(0, cloud.shape[0] + 1, nb - 1)) if nb > 1 else np.zeros(0, np.int64)      # (equal cuts give empty batches)
        T = G.FoldTable(leaf)
        for part in np.split(cloud, cuts):
            T.fold(part)
        got, got_n = T.result()
        assert _same(got, want), (nb, got.shape, want.shape)
        assert np.array_equal(got_n, want_n), nb
        assert (np.diff(T.keys) > 0).all()


def test_batch_fold_equals_voxel_grid_for_any_split():
    rng = np.random.default_rng(21)
    bad = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1]], np.float32)
    # a cloud whose bounding box grows on every axis in both directions as it is consumed: shells of increasing half-width, shuffled inside a shell only
    shells = []
    for k in range(1, 13):
        s = rng.uniform(-1.5 * k, 1.5 * k, (1500, 3))
        s[:6] = np.array([[-1.5 * k, 0, 0], [1.5 * k, 0, 0], [0, -1.5 * k, 0], [0, 1.5 * k, 0], [0, 0, -1.5 * k], [0, 0, 1.5 * k]]) * 0.999
        shells.append(np.concatenate([s, rng.uniform(0, 50, (1500, 1))], 1).astype(np.float32))
        shells.append(bad)
    grow = np.concatenate(shells)
    grow[5::97, 0] = -0.0
    grow[11::89, 1] = -0.0
    grow[17::83, :3] = np.float32([-0.0, 0.0, -0.0])
    for leaf in (0.2, 0.4):
        _check_splits(grow, leaf, rng, [1, 2, 3, 12, 24, 50])
    # crowded voxels (1 .. 5000 members) among sparse points and non-finite rows, shuffled
    crowd = V.cluster_cloud(V.LEAF, seed=3)
    _check_splits(crowd, V.LEAF, rng, [1, 2, 7, 50])
    # duplicates and a stationary stretch repeated across batches
    still = np.tile(V.sized_cloud(3000, seed=1), (6, 1)) + np.concatenate([rng.normal(0, 1e-3, (18000, 3)), np.zeros((18000, 1))], 1).astype(np.float32)
    _check_splits(still.astype(np.float32), 0.3, rng, [1, 6, 17, 50])
    for _ in range(10):
        n = int(rng.integers(1, 4000))
        c = np.concatenate([rng.normal(0, 8, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
        _check_splits(c, float(rng.choice([0.2, 0.3, 0.4])), rng, [int(rng.integers(1, 51)) for _ in range(3)])


def test_empty_and_all_non_finite_batches_leave_the_table_alone():
    T = G.FoldTable(0.4)
    T.fold(np.zeros((0, 4), np.float32))
    T.fold(np.full((5, 4), np.nan, np.float32))
    assert T.keys.shape[0] == 0
    c = V.sized_cloud(500)
    T.fold(c)
    k0, s0 = T.keys.copy(), T.sums.copy()
    T.fold(np.full((5, 4), np.inf, np.float32))
    assert np.array_equal(k0, T.keys) and _same(s0, T.sums)


def _detect_c(lib, pos, times, sel, t_now, variant, radius, local, glob, t_last, width):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    times = np.ascontiguousarray(times, np.float64)
    sel = np.ascontiguousarray(sel, np.float32)
    a, b = C.c_int(-7), C.c_int(-7)
    rc = lib.lili_loop_detect(pos.ctypes.data if pos.size else None, times.ctypes.data if times.size else None, pos.shape[0], sel.ctypes.data, float(t_now), variant,
                              float(radius), float(local), float(glob), float(t_last), int(width), C.byref(a), C.byref(b))
    assert rc in (0, 1), rc
    return (a.value, b.value) if rc == 1 else None


def test_loop_detect_equals_the_python_detect():
    lib = L.load_library()
    ctx = types.SimpleNamespace(lib=lib)      # LoopClosure.detect is host code: no device needed
    rng = np.random.default_rng(5)
    n_hit = {"livox": 0, "rot": 0}
    n_none = {"livox": 0, "rot": 0}
    for case in range(4000):
        variant = "livox" if case % 2 == 0 else "rot"
        n = int(rng.choice([0, 1, 2, 5, 40, 300]))
        radius = float(rng.choice([3.0, 10.0, 25.0]))
        local, glob = float(rng.uniform(1, 20)), float(rng.uniform(20, 60))
        lc = L.LoopClosure(ctx, variant=variant, lc_search_radius=radius, local_lc_time_thres=local, global_lc_time_thres=glob, lc_time_thres=glob,
                           slide_window_width=int(rng.integers(1, 5)))
        pos = rng.uniform(-15, 15, (n, 3)).astype(np.float32)
        sel = rng.uniform(-5, 5, 3).astype(np.float32)
        times = np.sort(rng.uniform(0, 120, n))
        t_now = float(rng.uniform(60, 130))
        if n >= 5:
            if case % 3 == 0:      # exact distance ties: mirrored twins and exact duplicates around the query
                pos[1] = sel + (pos[0] - sel) * np.float32(-1.0)
                pos[3] = pos[2]
                pos[4] = sel + np.float32([2.0, 0, 0])
                pos[0] = sel + np.float32([0, 2.0, 0])
            if case % 5 == 0:      # points exactly on the radius (d2 == radius^2 is outside) and just inside
                pos[2] = sel + np.float32([radius, 0, 0])
                pos[3] = sel + np.float32([0, np.nextafter(np.float32(radius), np.float32(0)), 0])
            if case % 7 == 0:      # a time exactly at a threshold
                times[2] = t_now - glob
                times[3] = t_now - local
        lc.time_last_loop = float(t_now - rng.choice([0.0, 0.1, 0.2, 0.3, 50.0]))      # ROT's 0.2 s rule
        want = lc.detect(pos, times, sel, t_now)
        got = _detect_c(lib, pos, times, sel, t_now, 0 if variant == "livox" else 1, radius, local, glob, lc.time_last_loop, lc.slide_window_width)
        assert got == want, (case, variant, got, want)
        (n_hit if want else n_none)[variant] += 1
    assert min(n_hit.values()) > 200 and min(n_none.values()) > 200, (n_hit, n_none)
    z = np.zeros(3, np.float32)
    assert lib.lili_loop_detect(None, None, 0, z.ctypes.data, 0.0, 2, 1.0, 1.0, 1.0, 0.0, 3, C.byref(C.c_int()), C.byref(C.c_int())) == -1      # unknown variant


def test_new_functions_are_declared_bound_and_exported():
    lib = L.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lili_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lili_[a-z0-9_]+)\s*\(", txt))
    for n in NEW:
        assert n in declared, n
        assert n in L.api._SIGS, n
        assert hasattr(lib, n), n
    assert lib.lili_abi_version() == 1
    assert L.KeyframeArchive is not None and L.GlobalMap is not None
    # the C prototypes and the ctypes table agree on the number of arguments
    for n in NEW:
        proto = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(L.api._SIGS[n][1]), n
