"""The referee of the levelled submap descriptors (tests/place_submap_model.py) against the plain-loop model and against the library's host functions
(lili_place_frame, lili_place_relative), and the wedge scene on the MODEL alone: what one keyframe of a narrow sensor cannot find, a levelled submap does."""
import math
import os

import numpy as np
import pytest

import lili_om_amd as L
from tests import place_model as PM
from tests import place_submap_cases as CS
from tests import place_submap_model as SM

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_ring,n_sector", [(20, 60), (1, 4), (32, 64)])
def test_vectorised_describe_is_the_loop_model_bit_for_bit(n_ring, n_sector):
    hard = CS.hard_cloud(n_ring, n_sector, 80.0, 2.0, np.random.default_rng(1000 + n_ring))
    assert hard.shape == (5000, 4)
    for rows in (hard, hard[:257], hard[:1], hard[:0]):
        a, b = SM.describe(rows, n_ring, n_sector, 80.0, 2.0), PM.describe(rows, n_ring, n_sector, 80.0, 2.0)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), np.argwhere(a != b)[:5]
    assert np.count_nonzero(PM.describe(hard, n_ring, n_sector, 80.0, 2.0)) > (n_ring * n_sector) // 2


def test_place_row_is_transform_point_in_f64_rounded_once():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-80, 80, (200, 3)).astype(F)
    ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    q, t = np.concatenate([[math.cos(0.15)], math.sin(0.15) * ax]), np.array([1.5, -2.25, 0.125])
    R = L.loop._matrix_from_quat(q)
    want = pts.astype(np.float64) @ R.T + t
    got = SM.place_row(pts, q, t)
    assert got.dtype == F and np.abs(got - want).max() <= 80 * 2.0 ** -23      # half an ulp of f32 at 80 m, and the f64 sums' own error far below it
    ident = SM.place_row(pts, [1.0, 0, 0, 0], [0.0, 0, 0])
    assert ident.tobytes() == pts.tobytes()


def _rand_pose(rng, scale=1e3):
    q = rng.normal(size=4)
    return np.concatenate([rng.uniform(-scale, scale, 3), q / np.linalg.norm(q) * rng.uniform(0.5, 2.0)])


def test_frame_and_relative_against_the_model():
    """1e-12 per entry for |t| <= 1e3 m: three rigid operations in f64 (a normalisation, a quaternion product, a rotation of a difference of up to 2e3 m: a few
    ulp of 2e3, 2.3e-13 each) — lili_place_guess's own bound and derivation."""
    rng = np.random.default_rng(11)
    for _ in range(200):
        a, b = _rand_pose(rng), _rand_pose(rng)
        for level in (0, 1):
            f = L.place_frame(a, level)
            assert np.abs(f - SM.frame(a, level)).max() <= 1e-12
            q, t = L.place_relative(f, b)
            qm, tm = SM.relative(SM.frame(a, level), b)
            assert np.abs(q - qm).max() <= 1e-12 and np.abs(t - tm).max() <= 1e-12
            # and the model against plain matrices: the member's rows land where M_F^-1 M_k puts them
            Rf, Rb = L.loop._matrix_from_quat(f[3:] / np.linalg.norm(f[3:])), L.loop._matrix_from_quat(b[3:] / np.linalg.norm(b[3:]))
            assert np.abs(L.loop._matrix_from_quat(qm) - Rf.T @ Rb).max() <= 1e-12 and np.abs(tm - Rf.T @ (b[:3] - f[:3])).max() <= 1e-9
    assert np.array_equal(L.place_frame(a, 0), a)                                       # level 0: the pose as it is


def test_levelled_frame_properties():
    rng = np.random.default_rng(12)
    for _ in range(100):
        p = _rand_pose(rng)
        f = L.place_frame(p, 1)
        assert np.array_equal(f[:3], p[:3]) and f[4] == 0.0 and f[5] == 0.0 and f[3] >= 0.0
        Rf, Rp = L.loop._matrix_from_quat(f[3:]), L.loop._matrix_from_quat(p[3:] / np.linalg.norm(p[3:]))
        assert np.array_equal(Rf[:, 2], [0.0, 0.0, 1.0]) and np.array_equal(Rf[2], [0.0, 0.0, 1.0])      # z is the map's z, exactly
        hx = Rp[:2, 0] / np.linalg.norm(Rp[:2, 0])
        assert np.abs(Rf[:2, 0] - hx).max() <= 1e-12                                                      # x: the horizontal projection of the LiDAR's x
    for yaw in (0.0, 0.3, -2.9, 1.5707, 3.1):                                                             # a yaw-only pose is its own frame
        p = np.array([1.0, 2.0, 3.0, math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)])
        f = L.place_frame(p, 1)
        assert np.abs(f - p).max() <= 1e-12, (yaw, f)
        q, t = L.place_relative(f, p)
        assert np.abs(q - [1.0, 0, 0, 0]).max() <= 1e-12 and not t.any()


def test_levelled_frame_branches():
    s = math.sqrt(0.5)
    # the x axis vertical (h < 1e-9): c = 1, s = 0 — the identity rotation
    for q in ([s, 0.0, -s, 0.0], [s, 0.0, s, 0.0], [s, 0.0, -s * (1 - 1e-12), 0.0]):
        p = np.array([4.0, 5.0, 6.0] + q)
        for f in (L.place_frame(p, 1), SM.frame(p, 1)):
            assert np.array_equal(f, [4.0, 5.0, 6.0, 1.0, 0.0, 0.0, 0.0]), (q, f)
    # a half turn about z (c = -1, s = +0 or -0): (0, 0, 0, +1) from both zeros
    for q in ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, 2.0]):
        p = np.array([0.0, 0.0, 0.0] + q)
        for f in (L.place_frame(p, 1), SM.frame(p, 1)):
            assert np.array_equal(f[3:], [0.0, 0.0, 0.0, 1.0]), (q, f)
    # just either side of the half turn: the sign of s decides
    for eps, sign in ((1e-6, -1.0), (-1e-6, 1.0)):
        yaw = math.pi + eps
        p = np.array([0.0, 0.0, 0.0, math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)])
        f, m = L.place_frame(p, 1), SM.frame(p, 1)
        assert np.sign(f[6]) == sign and np.abs(f - m).max() <= 1e-12 and abs(abs(f[6]) - 1.0) <= 1e-12
    # argument errors
    lib = L.load_library()
    out, q, t = np.zeros(7), np.zeros(4), np.zeros(3)
    good = np.array([0.0, 0, 0, 1.0, 0, 0, 0])
    for bad in (np.array([0.0, 0, 0, 0.0, 0, 0, 0]), np.array([np.nan, 0, 0, 1.0, 0, 0, 0]), np.array([0.0, 0, 0, np.inf, 0, 0, 0])):
        assert lib.lili_place_frame(L.api._ptr(bad), 1, L.api._ptr(out)) != 0
        assert lib.lili_place_relative(L.api._ptr(bad), L.api._ptr(good), L.api._ptr(q), L.api._ptr(t)) != 0
        assert lib.lili_place_relative(L.api._ptr(good), L.api._ptr(bad), L.api._ptr(q), L.api._ptr(t)) != 0
    assert lib.lili_place_frame(L.api._ptr(good), 2, L.api._ptr(out)) != 0 and lib.lili_place_frame(L.api._ptr(good), -1, L.api._ptr(out)) != 0
    assert lib.lili_place_frame(None, 1, L.api._ptr(out)) != 0 and lib.lili_place_frame(L.api._ptr(good), 1, None) != 0
    assert not out.any() and not q.any() and not t.any()


def test_windows_keys_and_rebuilds():
    assert SM.windows(5, 2, 1) == [(0, 1), (0, 2), (0, 3), (1, 4), (2, 4)]
    assert SM.windows(1, 64, 16) == [(0, 0)] and SM.windows(3, 0, 0) == [(0, 0), (1, 1), (2, 2)]
    rng = np.random.default_rng(3)
    poses = np.array([_rand_pose(rng, 50.0) for _ in range(7)])
    for level in (0, 1):
        k6, k7 = SM.keys(poses[:6], 2, 1, level), SM.keys(poses, 2, 1, level)
        assert SM.expected_rebuilds([], k6) == list(range(6))
        assert SM.expected_rebuilds(k6, k7) == [5, 6]                                   # the new keyframe and the one whose window it enters
        assert SM.expected_rebuilds(k7, k7) == []
        moved = poses.copy()
        moved[3, 0] += 0.25
        assert SM.expected_rebuilds(k7, SM.keys(moved, 2, 1, level)) == [2, 3, 4, 5]    # the windows that hold keyframe 3
        assert [e[1] for e in k7[3]] == ([0, 0, 1, 0] if level == 0 else [0, 0, 0, 0])  # the identity flag: the centre, unlevelled only
    plain = SM.keys(poses, 0, 0, 0)
    assert SM.expected_rebuilds(plain, SM.keys(poses + 1.0, 0, 0, 0)) == []             # the plain key holds no pose


def test_mirror_and_constant_match_the_header(tmp_path):
    import ctypes as C
    import subprocess
    T = L.api.PlaceSubmap
    lines = ['printf("%zu\\n", sizeof(lili_place_submap));'] + [f'printf("%zu\\n", offsetof(lili_place_submap, {f}));' for f, _ in T._fields_]
    lines.append('printf("%d\\n", LILI_PLACE_TILE_ROWS);')
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "lay")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "lay")]).split()]
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_] + [L.api.PLACE_TILE_ROWS]


# ---- the wedge scene, on the model alone -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wedge():
    sc = CS.wedge_scene(77, 12.0)
    sc["single"] = [SM.describe(r, **CS.PARAMS) for r in sc["rows"]]
    sc["submap"] = SM.archive_describe(sc["rows"], sc["poses"], CS.BACK, CS.FWD, 1, **CS.PARAMS)
    return sc


def _ranked(sc, descs):
    q = CS.QUERY
    return PM.search(descs, sc["times"], descs[q], len(descs), q_id=q, q_time=sc["times"][q], min_time_gap=25.0, max_id=q)


def _true_distance(sc, c):
    return float(np.linalg.norm(sc["true"][c][0][:2] - sc["true"][CS.QUERY][0][:2]))


def test_the_wedge_scene_on_the_model(wedge):
    """seed 77, the sensor pitched 12 degrees, back 20 / fwd 2 / levelled, max_radius 30 — the issue's hardest row, in exact f32 form"""
    sc = wedge
    assert len(sc["rows"]) == CS.N1 + CS.N2 and abs(sc["true"][CS.QUERY][0][0] - 34.0) < 1e-12 and _true_distance(sc, CS.MATCH) <= 0.5
    single, sub = _ranked(sc, sc["single"]), _ranked(sc, sc["submap"])
    assert {c for c, _, _ in sub} == set(range(CS.N1)) | set(range(CS.N1, 71))          # the eligible: all of pass 1, and pass 2 more than 25 s ago
    print("single keyframe:", single[0], "  submap:", sub[0], "  best far away:", next(r for r in sub if _true_distance(sc, r[0]) > 6.0))
    assert _true_distance(sc, single[0][0]) > 6.0                                        # one keyframe does not find the place
    c, s, d = sub[0]
    assert _true_distance(sc, c) <= 2.0 and abs(c - CS.MATCH) <= 1 and abs(s - 30) <= 1
    far = [r for r in sub if _true_distance(sc, r[0]) > 6.0]
    assert far and min(r[2] for r in far) - d > 0.03
    # what the device comparison of ids and shifts rests on (tests/test_place_gpu.py's _check_search): the model's ranking and shift decided by more than 1e-9
    assert sub[1][2] - sub[0][2] > 1e-9
    ds = np.sort(PM.shift_distances(sc["submap"][CS.QUERY], sc["submap"][c]))
    assert ds[1] - ds[0] > 1e-9
