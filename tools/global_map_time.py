"""Global-map and archive timing: ms per call, medians of --reps after one warm-up, wall clock around the blocking calls.  Per sequence
(Livox-sized 24 k-row full clouds x 500 and x 2000 keyframes, ROT-sized 130 k x 500; leaf 0.3):
  a. lili_global_map from an empty table;  b. the incremental update after 10 new keyframes;  c. the rebuild after lili_archive_set_poses of everything;
  d. the one-shot way to the same map: lili_loop_cloud's gather of the archive's views followed by ONE lili_voxel_filter over the placed device cloud;
  e. the loop-closure submaps (source 1 + target 41 keyframes, edge + surf) from the archive against lili_loop_cloud x 2 from host clouds.
The keyframes cycle through --pool distinct clouds at poses along a widening spiral.  No number here is a gate.

    python tools/global_map_time.py [--reps 7] [--only livox500] [--out profiles/global_map_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lili_om_amd as L  # noqa: E402
from lili_om_amd import synth  # noqa: E402
from lili_om_amd.archive import ARCHIVE_FULL  # noqa: E402

Q_BL = np.array([0.999, 0.01, -0.02, 0.03]) / np.linalg.norm([0.999, 0.01, -0.02, 0.03])
T_BL = np.array([0.1, -0.05, 0.2])
SEQUENCES = {"livox500": (24_000, 500), "livox2000": (24_000, 2000), "rot500": (130_000, 500)}


def yaw(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def timed(fn, reps, before=None):
    ms = []
    for r in range(reps + 1):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def one_shot(ctx, arch, n_kf, ts, qs, leaf, d_raw, cap):
    """the parent commit's way: gather at the map poses (lili_loop_cloud, no filter), copy to a caller's device buffer, lili_voxel_filter over it"""
    views = (L.api.Cloud * n_kf)(*[arch.view(k, ARCHIVE_FULL) for k in range(n_kf)])
    poses = [L.api.keyframe_map_pose(ts[k], qs[k], T_BL, Q_BL) for k in range(n_kf)]
    t = np.ascontiguousarray(np.array([p[0] for p in poses]).reshape(-1))
    q = np.ascontiguousarray(np.array([p[1] for p in poses]).reshape(-1))
    a, b = C.c_int64(0), C.c_int64(0)

    def run():
        ctx._chk(ctx.lib.lili_loop_cloud(ctx.h, 0, views, n_kf, t.ctypes.data, q.ctypes.data, C.c_float(0.0), C.byref(a), C.byref(b)))
        fo = L.api.FeatureOut(d_raw, a.value, 16, L.api.MEM_DEVICE, 0)
        ctx._chk(ctx.lib.lili_icp_get_cloud(ctx.h, 0, C.byref(fo)))
        out = L.api.FeatureOut(None, 0, 16, L.api.MEM_HOST, 0)
        ctx._chk(ctx.lib.lili_voxel_filter(ctx.h, C.byref(L.api.cloud_from_device(d_raw, a.value, 16, 12)), C.c_float(leaf), C.byref(out), None))
        return out.count
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pool", type=int, default=48)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-one-shot", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(7)
    W = synth.OutdoorScene().sample_surfaces(90.0, 90.0, 0.25, rng).astype(np.float32)
    result = {}
    for name, (rows, n_kf) in SEQUENCES.items():
        if a.only and name != a.only:
            continue
        pool = []
        for k in range(a.pool):
            c = np.array([60 * np.cos(0.4 * k), 60 * np.sin(0.4 * k), 1.8])
            sel = W[np.linalg.norm(W[:, :2] - c[:2], axis=1) < 30.0]
            sel = sel[rng.integers(0, sel.shape[0], rows)]
            loc = ((sel.astype(np.float64) - c) @ yaw(23.0 * k)).astype(np.float32)
            pool.append(np.concatenate([loc, rng.uniform(0, 1, (rows, 1)).astype(np.float32)], 1))
        n_all = n_kf + 10
        ts = [np.array([(20 + 0.15 * k) * np.cos(0.05 * k), (20 + 0.15 * k) * np.sin(0.05 * k), 1.8]) for k in range(n_all)]
        qs = [L.loop.quat_from_matrix(yaw(2.9 * k)) for k in range(n_all)]
        ctx = L.Context(0)
        arch = L.KeyframeArchive(ctx, Q_BL, T_BL)
        gm = L.GlobalMap(arch)
        t0 = time.perf_counter()
        for k in range(n_kf):
            f = pool[k % a.pool]
            arch.push(f[::8].copy(), f[1::4].copy(), f, 0.1 * k, ts[k], qs[k])
        push_ms = (time.perf_counter() - t0) * 1e3 / n_kf

        def other():
            gm.build(0, 10 ** 6, 1.0)      # another setting: the next build starts from an empty table
        (n_raw, n_map), build_ms = timed(lambda: gm.build(ARCHIVE_FULL, 1, a.leaf), a.reps, before=other)
        # c. correctPoses of everything, then the rebuild
        ts2 = [t + np.array([0.01, -0.02, 0.005]) for t in ts]
        flip = [0]

        def repose():
            flip[0] ^= 1
            arch.set_poses(0, (ts2 if flip[0] else ts)[:n_kf], qs[:n_kf])
        _, rebuild_ms = timed(lambda: gm.build(ARCHIVE_FULL, 1, a.leaf), a.reps, before=repose)
        if flip[0]:
            repose()
            gm.build(ARCHIVE_FULL, 1, a.leaf)
        rec = dict(rows_per_keyframe=rows, keyframes=n_kf, points=n_raw, voxels=n_map, leaf=a.leaf, push_ms_per_keyframe=push_ms, build_ms=build_ms, rebuild_ms=rebuild_ms,
                   archive_bytes=arch.info()[2], table_work_bytes=gm.info())
        # d. the one-shot way (before the ten extra keyframes, on the same content)
        if not a.no_one_shot and n_raw < 2 ** 31:
            d_raw = torch.empty((n_raw, 4), dtype=torch.float32, device="cuda")
            n_one, one_ms = timed(one_shot(ctx, arch, n_kf, ts, qs, a.leaf, d_raw.data_ptr(), n_raw), a.reps)
            rec.update(one_shot_ms=one_ms, one_shot_voxels=n_one, one_shot_raw_bytes=n_raw * 16)
            del d_raw
        # b. ten new keyframes per update (each update is a new measurement: the table grows a little)
        inc_ms = []
        for r in range(a.reps + 1):
            if len(arch) + 10 > n_all + 10 * a.reps:
                break
            for j in range(10):
                k = len(arch)
                f = pool[k % a.pool]
                arch.push(f[::8].copy(), f[1::4].copy(), f, 0.1 * k, ts[n_kf + j], qs[n_kf + j])
            t0 = time.perf_counter()
            gm.build(ARCHIVE_FULL, 1, a.leaf)
            if r:
                inc_ms.append((time.perf_counter() - t0) * 1e3)
        rec.update(incremental_10_ms=inc_ms, stats=gm.stats())
        # e. loop-closure submaps from the archive against host clouds (Livox sizes: 1 + 41 keyframes)
        lc_a = L.LoopClosure(ctx, variant="livox", lc_map_width=20, q_bl=Q_BL, t_bl=T_BL, archive=arch)
        lc_h = L.LoopClosure(ctx, variant="livox", lc_map_width=20, q_bl=Q_BL, t_bl=T_BL)
        latest, his = n_kf - 1, 100
        edge = {k: pool[k % a.pool][::8].copy() for k in range(n_kf)}
        surf = {k: pool[k % a.pool][1::4].copy() for k in range(n_kf)}
        sa, asm_a = timed(lambda: lc_a.assemble(latest, his), a.reps)
        sh, asm_h = timed(lambda: lc_h.assemble(latest, his, np.array(ts[:n_kf]), np.array(qs[:n_kf]), edge, surf), a.reps)
        rec.update(loop_assemble_archive_ms=asm_a, loop_assemble_host_ms=asm_h, loop_sizes=sa, loop_sizes_equal=bool(sa == sh))
        for key in ("build_ms", "rebuild_ms", "one_shot_ms", "incremental_10_ms", "loop_assemble_archive_ms", "loop_assemble_host_ms"):
            if rec.get(key):
                rec[key + "_median"] = float(np.median(rec[key]))
        result[name] = rec
        print(name, json.dumps(rec), flush=True)
        ctx.close()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
