"""Loop closure without a GPU: the numpy restatement of the registration (tests/icp_model.py), the convergence rule on crafted logs, the candidate selection
of detectLoopClosure and the ctypes mirrors of the new structures."""
import ctypes as C
import os
import subprocess

import numpy as np

import lili_om_amd as L
from lili_om_amd.loop import LoopClosure, quat_from_matrix
from tests import icp_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMAX = np.finfo(np.float64).max


def _rot(axis, deg):
    a = np.deg2rad(deg)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def test_model_recovers_an_exact_rigid_motion(oracle):
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-10, 10, (4000, 3)).astype(np.float32)
    R, t = _rot([1, 2, 3], 4.0), np.array([0.3, -0.2, 0.1])
    # the source: target points moved by (R, t)^-1, so that T = (R, t) maps it back
    src = ((tgt[::2].astype(np.float64) - t) @ R).astype(np.float32)
    res = M.align(oracle.KdTree(tgt), tgt, src)
    assert res["converged"]
    assert np.abs(res["transform"][:3, :3] - R).max() < 1e-5 and np.abs(res["transform"][:3, 3] - t).max() < 1e-5
    f, n = M.fitness(oracle.KdTree(tgt), tgt, src, res["transform"])
    assert n == src.shape[0] and f < 1e-9


def test_umeyama_reflection_rule_and_planar_case():
    rng = np.random.default_rng(4)
    P = np.concatenate([rng.uniform(-3, 3, (200, 2)), np.zeros((200, 1))], 1)       # planar: rank-2 H
    R0 = _rot([0.3, -1, 0.2], 20.0)
    R, t = M.umeyama_rotation(P, P @ R0.T + [1.0, 2.0, 3.0])
    assert np.abs(R - R0).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    assert np.abs(t - [1.0, 2.0, 3.0]).max() < 1e-12


def test_convergence_rule_every_state():
    teps, feps = 1e-6, 1e-6
    assert M.convergence_state(100, 100, 0.0, 1.0, 1.0, 2.0, teps, feps) == M.ITERATIONS      # the count first, whatever else holds
    assert M.convergence_state(3, 100, 1.0 - 1e-7, 1e-7, 1.0, 2.0, teps, feps) == M.TRANSFORM
    assert M.convergence_state(3, 100, 1.0 - 1e-5, 1e-7, 1.0, 2.0, teps, feps) == M.NOT_CONVERGED       # rotation too large
    assert M.convergence_state(3, 100, 1.0, 2e-6, 1.0, 1.0 + 5e-13, teps, feps) == M.ABS_MSE
    assert M.convergence_state(3, 100, 1.0, 2e-6, 1.0, 1.0 + 5e-7, teps, feps) == M.REL_MSE
    assert M.convergence_state(1, 100, 1.0, 2e-6, 1.0, DMAX, teps, feps) == M.NOT_CONVERGED              # prev starts at DBL_MAX
    log = [dict(mse=1.0, cos_angle=0.99, translation_sqr=1.0, n_corr=50), dict(mse=0.5, cos_angle=0.999, translation_sqr=0.1, n_corr=50),
           dict(mse=0.5 + 1e-8, cos_angle=0.9999, translation_sqr=0.01, n_corr=50)]
    assert M.replay_states(log, 100) == ([M.NOT_CONVERGED, M.NOT_CONVERGED, M.REL_MSE], 3)
    assert M.replay_states(log, 2) == ([M.NOT_CONVERGED, M.ITERATIONS], 2)
    assert M.replay_states([dict(n_corr=2)], 100) == ([M.NO_CORRESPONDENCES], 0)
    assert M.replay_states([log[0], dict(n_corr=0)], 100) == ([M.NOT_CONVERGED, M.NO_CORRESPONDENCES], 1)


class _Ctx:
    lib = None


def test_detect_livox_rules():
    lc = LoopClosure(_Ctx(), variant="livox", lc_search_radius=10.0, local_lc_time_thres=25.0, global_lc_time_thres=40.0, slide_window_width=3)
    pos = np.array([[5, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [20, 0, 0], [21, 0, 0], [22, 0, 0]], np.float32)
    times = np.array([0.0, 30.0, 45.0, 20.0, 80.0, 85.0, 90.0])
    # query at the origin, t 90: in radius 0..3 by distance: 1 (dt 60), 2 (dt 45), 3 (dt 70), 0 (dt 90) -> the first with dt > 40 is 1
    assert lc.detect(pos, times, (0, 0, 0), 90.0) == (4, 1)
    # t 60: dts 30 (1), 15 (2), 40 (3: not > 40), 60 (0) -> 0 is the first beyond 40
    assert lc.detect(pos, times, (0, 0, 0), 60.0) == (4, 0)
    # t 55: dts 25 (1: not > 25), 10, 35 (3), 55 (0) -> 0 beyond 40
    assert lc.detect(pos, times, (0, 0, 0), 55.0) == (4, 0)
    # drop keyframe 0: t 55 -> nothing beyond 40; inside (25, 40): 3 (35) -> 3
    assert lc.detect(pos[1:], times[1:], (0, 0, 0), 55.0) == (3, 2)
    # t 46: dts 16, 1, 26 -> 3 (index 2 of the cut) is the only one in (25, 40)
    assert lc.detect(pos[1:], times[1:], (0, 0, 0), 46.0) == (3, 2)
    # t 40: dts 10, 5, 20 -> none
    assert lc.detect(pos[1:], times[1:], (0, 0, 0), 40.0) is None
    # the radius is strict (d2 < r2) and f32: a keyframe at exactly 10 m is out
    assert lc.detect(np.array([[10, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32), np.array([0.0, 99, 99, 99]), (0, 0, 0), 100.0) is None


def test_detect_rot():
    lc = LoopClosure(_Ctx(), variant="rot", lc_search_radius=10.0, lc_time_thres=60.0, slide_window_width=3)
    pos = np.array([[4, 0, 0], [1, 0, 0], [2, 0, 0], [30, 0, 0], [31, 0, 0], [32, 0, 0]], np.float32)
    times = np.array([0.0, 10.0, 50.0, 80.0, 90.0, 100.0])
    # by distance: 1 (dt 90), 2 (dt 50), 0 (dt 100) -> 1
    assert lc.detect(pos, times, (0, 0, 0), 100.0) == (3, 1)
    # t 65: dts 55, 15, 65 -> 0; no second threshold in ROT
    assert lc.detect(pos, times, (0, 0, 0), 65.0) == (3, 0)
    assert lc.detect(pos, times, (0, 0, 0), 55.0) is None
    lc.time_last_loop = 99.9
    assert lc.detect(pos, times, (0, 0, 0), 100.0) is None           # within 0.2 s of the last loop
    lc.time_last_loop = 99.7
    assert lc.detect(pos, times, (0, 0, 0), 100.0) == (3, 1)
    assert lc.source_keyframes(3) == [3, 2, 1, 0] and lc.target_keyframes(3, 1) == [0, 1, 2, 3]
    lc2 = LoopClosure(_Ctx(), variant="livox", lc_map_width=2)
    assert lc2.source_keyframes(7) == [7] and lc2.target_keyframes(7, 6) == [4, 5, 6, 7]


def test_quat_from_matrix_round_trip():
    for axis, deg in (([1, 0, 0], 10), ([0, 1, 1], 170), ([1, -2, 0.5], 179.9), ([0, 0, 1], 0)):
        R = _rot(axis, deg)
        q = quat_from_matrix(R)
        w, x, y, z = q
        R2 = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert np.abs(R2 - R).max() < 1e-12


def test_loop_struct_mirrors_match_the_header(tmp_path):
    pairs = [("lili_icp_params", L.api.IcpParams), ("lili_icp_iteration", L.api.IcpIteration), ("lili_icp_result", L.api.IcpResult)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    lines.append('printf("%d\\n", LILI_ICP_MAX_LOG);')
    expect.append(L.api.ICP_MAX_LOG)
    for k, name in enumerate(["LILI_ICP_NOT_CONVERGED", "LILI_ICP_ITERATIONS", "LILI_ICP_TRANSFORM", "LILI_ICP_ABS_MSE", "LILI_ICP_REL_MSE", "LILI_ICP_NO_CORRESPONDENCES"]):
        lines.append(f'printf("%d\\n", {name});')
        expect.append(k)
    src = tmp_path / "lay_loop.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_loop"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect
    for name in ("lili_loop_cloud", "lili_icp_set_cloud", "lili_icp_get_cloud", "lili_icp_align", "lili_icp_fitness", "lili_icp_get_correspondences", "lili_icp_default_params"):
        assert name in L.api._SIGS
