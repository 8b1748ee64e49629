"""Loop-closure registration timing: ms per lili_loop_cloud and per lili_icp_align at the reference's sizes — L: source 1 keyframe, target 41;
ROT: 6 and 51 — with ~20 k points per keyframe (synthetic scene, a path that returns with 0.5 m / 3 deg of drift in the revisit's poses), iterations and host synchronisations per align,
and the numpy model's CPU time for the same align beside it.  Medians over --reps runs after one warm-up.  No number here is a gate.

    python tools/loop_icp_time.py [--reps 7] [--no-model]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lili_om_amd as L  # noqa: E402
from lili_om_amd import synth  # noqa: E402


def rot(axis, deg):
    a = np.deg2rad(deg)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--per-kf", type=int, default=20000)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    W = synth.OutdoorScene().sample_surfaces(90.0, 90.0, 0.3, rng).astype(np.float32)
    n_kf = 80
    ts, qs, kfs = [], [], []
    Dr, Dt = rot([0.2, 0.3, 1.0], 3.0), np.array([0.4, -0.3, 0.05])
    for k in range(n_kf):      # a circle of radius 40 m, once round every 54 keyframes: keyframe 79 revisits keyframe 25
        ang = 2 * np.pi * k / 54
        t = np.array([40 * np.cos(ang), 40 * np.sin(ang), 1.8])
        R = rot([0, 0, 1], np.rad2deg(ang) + 90)
        sel = W[np.linalg.norm(W[:, :2] - t[:2], axis=1) < 30.0]
        sel = sel[rng.choice(sel.shape[0], min(a.per_kf, sel.shape[0]), replace=False)]
        loc = np.concatenate([((sel.astype(np.float64) - t) @ R).astype(np.float32), np.zeros((sel.shape[0], 1), np.float32)], 1)
        kfs.append((loc[::8].copy(), np.delete(loc, np.s_[::8], 0).copy()))
        if k >= n_kf - 6:      # the revisit's keyframes carry the drift in their poses, not in their points
            R, t = Dr @ R, Dr @ t + Dt
        ts.append(t)
        qs.append(L.loop.quat_from_matrix(R))
    ts, qs = np.array(ts), np.array(qs)
    ctx = L.Context(0)
    out = {}
    for variant, width in (("livox", 20), ("rot", 25)):
        lc = L.LoopClosure(ctx, variant=variant, lc_map_width=width)
        latest, his = n_kf - 1, 25
        edge, surf = [k[0] for k in kfs], [k[1] for k in kfs]
        t_asm, t_align, res = [], [], None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            sizes = lc.assemble(latest, his, ts, qs, edge, surf)
            t1 = time.perf_counter()
            res = lc.align()
            t2 = time.perf_counter()
            if r:
                t_asm.append((t1 - t0) * 1e3)
                t_align.append((t2 - t1) * 1e3)
        rec = dict(source_keyframes=len(lc.source_keyframes(latest)), target_keyframes=len(lc.target_keyframes(latest, his)), source_raw_ds=sizes[0], target_raw_ds=sizes[1],
                   loop_cloud_ms_median=float(np.median(t_asm)), icp_align_ms_median=float(np.median(t_align)), icp_align_ms_min=float(np.min(t_align)),
                   iterations=res["iterations"], state=res["state"], host_syncs=res["host_syncs"], iterations_enqueued=res["iterations_enqueued"], fitness=res["fitness"])
        if not a.no_model:
            sys.path.insert(0, ROOT)
            from oracle import oracle as O
            from tests import icp_model as M
            src, tgt = lc.get_cloud(0), lc.get_cloud(1)
            t0 = time.perf_counter()
            tree = O.KdTree(np.ascontiguousarray(tgt[:, :3]))
            M.align(tree, tgt, src)
            rec["model_cpu_ms"] = (time.perf_counter() - t0) * 1e3
        out[variant] = rec
        print(variant, json.dumps(rec), flush=True)
    ctx.close()
    return out


if __name__ == "__main__":
    main()
