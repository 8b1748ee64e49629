"""Back-end keyframe cost with and without a local-map repose (lili_localmap_repose, the warm-up branch of buildLocalMapWithLandMark, L/src/BackendFusion.cpp:1407-1443)
on the 40-keyframe rings of bench_configs._config1_backend (Livox back-end flavour, leaves 0.4 / 0.2, 3-keyframe window, joining keyframe from its slot).  Per keyframe,
host wall time from a synchronised start to the synchronised end:
  (a) steady state: lili_backend_keyframe_prepare alone;
  (b) warm-up: repose of the newest 3 ring keyframes (the sliding window moved them), then prepare — one merge step per kind;
  (c) repose of all 40 keyframes (a loop closure's kind of change), then prepare — the full rebuild;
  (d) the old workaround: lili_localmap_reset of both rings, 40 host pushes per kind at the new poses, then prepare.
Usage: python tools/kf_warmup_time.py [timed keyframes per mode, default 20]  ->  one JSON line."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime in the process, as the package expects)

import bench_configs  # noqa: E402
import lili_om_amd as L  # noqa: E402
from lili_om_amd import synth  # noqa: E402

WIDTH, K = 40, 3


def main():
    n_timed = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_kf = WIDTH + 4 + 4 * n_timed
    P = L.make_params("livox")
    ctx = L.Context(0)
    try:
        ex = L.LivoxExtractor(ctx)
        m = L.ScanToMapMatcher(ctx, P)
        m.map_focus(None)
        bk = L.BackendKeyframes(ctx, P, leaf_surf=0.4, leaf_edge=0.2, width=WIDTH)
        feats, poses = [], []
        for f in range(min(n_kf, 60)):      # 60 distinct scans along the configs[1] circuit, reused cyclically
            t, q, yaw = bench_configs._circuit(f * 2)
            o = ex.extract(synth.make_livox_scan(100 + f * 2, origin=t, yaw=yaw, inject_bad=False))
            feats.append((np.ascontiguousarray(o["surf"][:, [0, 1, 2, 7]]), np.ascontiguousarray(o["edge"][:, [0, 1, 2, 7]])))
            poses.append((np.asarray(t, np.float64), np.asarray(q, np.float64)))
        ds = [(L.api.voxel_filter(ctx, s, 0.4)[0], L.api.voxel_filter(ctx, e, 0.2)[0]) for s, e in feats]
        rng = np.random.default_rng(7)
        ring = []                       # (keyframe id, t, q) of the rings, oldest first (host record of what they hold)
        times = {"a": [], "b": [], "c": [], "d": []}

        def jitter(t, q):
            q2 = q + rng.normal(0, 1e-3, 4)
            return t + rng.normal(0, 1e-2, 3), q2 / np.linalg.norm(q2)

        def step(k, mode):
            kf = k % len(feats)
            win = list(range(max(0, k - K + 1), k + 1))
            lid = [poses[j % len(feats)] for j in win]
            body = [L.api.body_pose_from_lidar(t, q, P) for t, q in lid]
            assoc = [L.api.assoc_transform(t, q, P) for t, q in body]
            join = None
            ctx.sync()
            tic = time.perf_counter()
            if k > 0:
                if mode in ("b", "c") and ring:
                    lo = len(ring) - 3 if mode == "b" else 0
                    for j in range(max(lo, 0), len(ring)):
                        ring[j] = (ring[j][0], *jitter(ring[j][1], ring[j][2]))
                    bk.repose([r[1] for r in ring], [r[2] for r in ring])
                if mode == "d" and ring:
                    for j in range(len(ring)):
                        ring[j] = (ring[j][0], *jitter(ring[j][1], ring[j][2]))
                    lm = [L.LocalMap(ctx, L.KIND_SURF, WIDTH, 0.4), L.LocalMap(ctx, L.KIND_EDGE, WIDTH, 0.2)]      # (the constructors reset the rings)
                    for r in ring:
                        lm[0].push(ds[r[0]][0], r[1], r[2]); lm[1].push(ds[r[0]][1], r[1], r[2])
                pj = poses[(k - 1) % len(feats)]
                join = ((k - 1) % K, pj[0], pj[1])
                ring.append(((k - 1) % len(feats), pj[0], pj[1]))
                del ring[:-WIDTH]
            bk.prepare(join, feats[kf][0], feats[kf][1], [j % K for j in win], [a[1] for a in assoc], [a[0] for a in assoc])
            ctx.sync()
            return time.perf_counter() - tic

        k = 0
        while len(ring) < WIDTH:        # fill the rings (warm-up calls, untimed)
            step(k, "a"); k += 1

        def stats():
            a, b = C.c_int32(0), C.c_int32(0)
            ctx._chk(ctx.lib.lili_localmap_stats(ctx.h, C.byref(a), C.byref(b)))
            return a.value, b.value
        commits = {}
        for mode in ("a", "b", "c", "d"):
            step(k, mode); k += 1       # one untimed call per mode
            s0 = stats()
            for _ in range(n_timed):
                times[mode].append(step(k, mode)); k += 1
            s1 = stats()
            commits[mode] = {"incremental": s1[0] - s0[0], "full": s1[1] - s0[1]}
        res = {m: round(float(np.median(v)) * 1e3, 4) for m, v in times.items()}
        out = {"tool": "kf_warmup_time", "ring_keyframes": WIDTH, "timed_per_mode": n_timed, "ms_per_keyframe_median": res,
               "ms_per_keyframe_mean": {m: round(float(np.mean(v)) * 1e3, 4) for m, v in times.items()},
               "commits": commits, "b_over_a": round(res["b"] / res["a"], 3), "d_over_b": round(res["d"] / res["b"], 3),
               "ring_points": [int(sum(ds[r[0]][0].shape[0] for r in ring)), int(sum(ds[r[0]][1].shape[0] for r in ring))]}
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
