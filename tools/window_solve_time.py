"""Wall time of one lili_window_solve on the harness window (3 x (2 500 + 200) features) against the two ways the library offered before it:
the host loop around lili_s2m_linearize_window (one blocking device evaluation per solver evaluation — only those device calls are timed,
not the Python LM around them) and the lidar-only lili_s2m_solve_lm_window.  Medians of N >= 7 after a warm-up; raw values to
profiles/window_solve_time_<tag>.json.

    python tools/window_solve_time.py [--n 9] [--tag mi355x]
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
from tests import window_harness as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--tag", default="mi355x")
    a = ap.parse_args()
    win = H.make_window(n_surf=2500, n_edge=200)
    room, P = win["room"], win["P"]
    mask = L.MASK_SURF | L.MASK_EDGE
    ctx = L.Context(0)
    m = L.ScanToMapMatcher(ctx, P)
    m.set_input_cloud(L.KIND_SURF, np.c_[room["map_xyz"], room["map_refl"]])
    m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
    assoc = []
    for k, kf in enumerate(win["kfs"]):
        m.set_queries(k, L.KIND_SURF, np.c_[kf["q_xyz"], kf["q_refl"]])
        m.set_queries(k, L.KIND_EDGE, kf["eq_xyz"])
        assoc.append(L.api.assoc_transform(win["init"][k]["t"], win["init"][k]["q"], P))
    m.associate_window([0, 1, 2], [x[1] for x in assoc], [x[0] for x in assoc], mask)
    s0 = np.array([np.concatenate([s["t"], s["q"], s["sb"]]) for s in win["init"]])
    sb = np.full((3, 9), np.nan)
    sb[0], sb[1] = win["init"][0]["sb"], win["init"][1]["sb"]
    ws = L.WindowSolver(ctx, m).set_problem([0, 1, 2], mask, imu=[p["pre"] for p in win["pres"]], sb_prior=sb)

    # ---- the parent's way: a host LM whose lidar block is ONE blocking lili_s2m_linearize_window per evaluation; the device calls are timed
    dev = [0.0, 0]

    def gpu_joint(*tq):
        ts, qs = tq[0::2], tq[1::2]
        t0 = time.perf_counter()
        recs = m.linearize_window([0, 1, 2], ts, qs, mask)
        dev[0] += time.perf_counter() - t0
        dev[1] += 1
        res, jacs = [], [np.zeros((27, 3 if i % 2 == 0 else 4)) for i in range(6)]
        for k, (G, cost, counts) in enumerate(recs):
            r, jac = L.api.gram_to_factor(G, cost)
            res.append(r)
            jacs[2 * k][9 * k:9 * k + 9] = jac[:, :3]
            jacs[2 * k + 1][9 * k:9 * k + 9] = jac[:, 3:7]
        return np.concatenate(res), jacs

    def host_loop():
        dev[0], dev[1] = 0.0, 0
        W.ceres_lm(H.build_problem(win, None, joint_lidar=gpu_joint), max_num_iterations=15)
        return dev[0] * 1e6, dev[1]

    def joint():
        t0 = time.perf_counter()
        _, info = ws.solve(s0)
        return (time.perf_counter() - t0) * 1e6, info

    def lidar_only():
        for k in range(3):
            m.pose_set(k, win["init"][k]["t"], win["init"][k]["q"])
        ctx.sync()
        t0 = time.perf_counter()
        m.solve_lm_window([0, 1, 2], mask)
        return (time.perf_counter() - t0) * 1e6

    for _ in range(3):
        host_loop(); joint(); lidar_only()
    raw = dict(host_loop_us=[], host_loop_evaluations=[], window_solve_us=[], window_solve_evaluations=[], solve_lm_window_us=[])
    for _ in range(max(7, a.n)):
        us, n = host_loop()
        raw["host_loop_us"].append(us); raw["host_loop_evaluations"].append(n)
        us, info = joint()
        raw["window_solve_us"].append(us); raw["window_solve_evaluations"].append(1 + len(info["log"]))
        raw["solve_lm_window_us"].append(lidar_only())
    med = {k: statistics.median(v) for k, v in raw.items()}
    out = dict(window="3 x (2500 surf + 200 edge)", n=max(7, a.n), median=med, raw=raw,
               per_evaluation_us=dict(host_loop=med["host_loop_us"] / med["host_loop_evaluations"], window_solve=med["window_solve_us"] / med["window_solve_evaluations"]))
    path = os.path.join(ROOT, "profiles", f"window_solve_time_{a.tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(median=med, per_evaluation_us=out["per_evaluation_us"])))
    ctx.close()


if __name__ == "__main__":
    main()
