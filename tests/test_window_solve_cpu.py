"""Host side of the joint-window solve (lili_window_evaluate / lili_window_solve), no GPU: the ctypes mirrors against the header, the
pre-integration packer, and the sqrt-information the calls compute once per solve in plain C++ against numpy's on the harness window."""
import ctypes as C
import os
import subprocess

import numpy as np

import lili_om_amd as L
from tests import window_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_struct_mirrors_match_the_header(tmp_path):
    pairs = [("lili_window_imu", L.api.WindowImu), ("lili_window_prior", L.api.WindowPrior), ("lili_window_problem", L.api.WindowProblem)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    src = tmp_path / "lay_win.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_win"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect
    lib = L.load_library()
    for name in ("lili_window_sqrt_info", "lili_window_evaluate", "lili_window_solve", "lili_window_state_get"):
        assert hasattr(lib, name)
    assert hasattr(L, "WindowSolver")


def test_preintegration_packer_round_trips():
    win = H.make_window(n_surf=20, n_edge=10)
    for p in win["pres"]:
        pre = p["pre"]
        w = L.api.pack_preintegration(pre)
        assert w.sum_dt == pre.sum_dt
        assert np.array_equal(np.array(w.g), pre.g_vec)
        assert np.array_equal(np.array(w.delta_p), pre.delta_p) and np.array_equal(np.array(w.delta_q), pre.delta_q) and np.array_equal(np.array(w.delta_v), pre.delta_v)
        assert np.array_equal(np.array(w.lin_ba), pre.ba) and np.array_equal(np.array(w.lin_bg), pre.bg)
        assert np.array_equal(np.array(w.jacobian).reshape(15, 15), pre.jacobian) and np.array_equal(np.array(w.covariance).reshape(15, 15), pre.covariance)

    class Other:          # the reference's attribute names, another gravity
        pass
    o = Other()
    pre = win["pres"][0]["pre"]
    for k in ("sum_dt", "delta_p", "delta_q", "delta_v", "jacobian", "covariance"):
        setattr(o, k, getattr(pre, k))
    o.linearized_ba, o.linearized_bg = pre.ba + 1.0, pre.bg - 1.0
    w = L.api.pack_preintegration(o, g=(0.0, 0.0, -9.81))
    assert np.array_equal(np.array(w.lin_ba), pre.ba + 1.0) and np.array_equal(np.array(w.lin_bg), pre.bg - 1.0) and w.g[2] == -9.81


def test_host_sqrt_info_is_the_cholesky_factor_of_the_inverse_covariance():
    """sqrt_info^T sqrt_info covariance = I, and sqrt_info = numpy.linalg.cholesky(inv(cov)).T.  No a-priori bound (the covariance's entries span 1e-10 .. 1e-4):
    measured on the CPU on the harness's two pre-integrations, the largest difference to numpy relative to the largest entry of sqrt_info is 3.83e-16 (both), and
    |S^T S cov - I|_max is 2.9e-15 / 2.8e-15 (numpy's own factor: 8.3e-15 / 7.5e-15; the library accumulates in long double).  Asserted at 100 x the measured values."""
    win = H.make_window(n_surf=20, n_edge=10)
    assert len(win["pres"]) == 2
    for p in win["pres"]:
        cov = p["pre"].covariance
        S = L.api.window_sqrt_info(cov)
        ref = np.linalg.cholesky(np.linalg.inv(cov)).T
        d_ref = np.abs(S - ref).max() / np.abs(ref).max()
        d_id = np.abs(S.T @ S @ cov - np.eye(15)).max()
        print(f"sqrt_info: vs numpy {d_ref:.3e} (relative to the largest entry), |S^T S cov - I| {d_id:.3e}, numpy's own {np.abs(ref.T @ ref @ cov - np.eye(15)).max():.3e}")
        assert np.array_equal(S, np.triu(S))
        assert d_ref <= 3.9e-14       # 100 x 3.83e-16
        assert d_id <= 2.9e-13        # 100 x 2.9e-15
    bad = win["pres"][0]["pre"].covariance.copy()
    bad[3, 3] = -bad[3, 3]
    try:
        L.api.window_sqrt_info(bad)
        raise AssertionError("a covariance that is not positive definite was accepted")
    except L.LiliError:
        pass
