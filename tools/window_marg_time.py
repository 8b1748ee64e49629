"""Wall time of the window's next prior on the device against the oracle's numpy Marginalization on the same host:
  lili_window_marginalize   the harness window (3 x (2 500 + 200) features, the reference's factor set) at the device's solved state: pack, upload, the
                            lidar launches, the single-workgroup assembly + Schur + two Jacobi eigen-decompositions, read-back;
  lili_marg_schur           a synthetic system at (m, n) = (15, 30): upload, the same kernel without the assembly, read-back;
  numpy                     oracle/lo_window.py::Marginalization (two LAPACK eigh) on the same two systems — the Schur / eigen part only, the factors'
                            evaluation not counted.
Medians of N >= 9 after 3 warm-ups; raw values to profiles/window_marg_time_<tag>.json (or --out).

    python tools/window_marg_time.py [--n 9] [--tag mi355x] [--out path]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lili_om_amd as L  # noqa: E402
from oracle import lo_window as W  # noqa: E402
from tests import marg_harness as MH  # noqa: E402
from tests import test_window_solve_gpu as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_rep = max(9, a.n)
    win, recs, block, sol, pb, M, kept, A_w, b_w, m_w = MH.first_marginalisation(3)
    ctx = L.Context(0)
    mt = S.gpu_side(ctx, win, recs)
    ws = S.window_problem(L.WindowSolver(ctx, mt), win, 3)
    final, _ = ws.solve(S.state_of(win, 3))
    sb = np.full((3, 9), np.nan)
    sb[0], sb[1] = final[0, 7:16], final[1, 7:16]
    ws.set_problem([0, 1, 2], S.MASK, imu=[p["pre"] for p in win["pres"]], sb_prior=sb)
    A_s, b_s = MH.schur_case(15, 30, None)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    ways = dict(window_marginalize_us=lambda: ws.marginalize(final),
                marg_schur_15_30_us=lambda: L.api.marg_schur(ctx, A_s, b_s, 15),
                numpy_window_15_21_us=lambda: W.Marginalization(A_w, b_w, m_w, []),
                numpy_15_30_us=lambda: W.Marginalization(A_s, b_s, 15, []))
    for _ in range(3):
        for fn in ways.values():
            fn()
    raw = {k: [] for k in ways}
    for _ in range(n_rep):
        for k, fn in ways.items():
            raw[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in raw.items()}
    out = dict(window="3 x (2500 surf + 200 edge), reference factor set, n = 21", schur="synthetic (15, 30)", n=n_rep, median=med, raw=raw)
    path = a.out or os.path.join(ROOT, "profiles", f"window_marg_time_{a.tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(median=med)))
    ctx.close()


if __name__ == "__main__":
    main()
