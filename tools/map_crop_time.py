"""Crop timing: ms per call, medians of --reps after one warm-up, wall clock around the blocking calls, on the tables of tools/global_map_time.py
(Livox-sized 24 k-row full clouds x 500 and x 2000 keyframes, leaf 0.3).  The box is 120 x 120 x 40 m round a pose in the middle of the trajectory.
  a. lili_global_map_crop, counting only (capacity 0);  b. into a caller's device buffer (what MapLocalizer does);  c. into host arrays;
  d. the only route before the crop: lili_global_map_get of EVERYTHING into a device buffer, then a mask over it (torch, on the device).
No number here is a gate.

    python tools/map_crop_time.py [--reps 7] [--only livox500] [--out profiles/map_crop_time_mi355x.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import global_map_time as G  # noqa: E402  (puts the repository root on sys.path)
import lili_om_amd as L  # noqa: E402
from lili_om_amd import synth  # noqa: E402
from lili_om_amd.archive import ARCHIVE_FULL  # noqa: E402

HALF = np.array([60.0, 60.0, 20.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pool", type=int, default=48)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(7)
    W = synth.OutdoorScene().sample_surfaces(90.0, 90.0, 0.25, rng).astype(np.float32)
    result = {}
    for name in ("livox500", "livox2000"):
        if a.only and name != a.only:
            continue
        rows, n_kf = G.SEQUENCES[name]
        pool = []
        for k in range(a.pool):
            c = np.array([60 * np.cos(0.4 * k), 60 * np.sin(0.4 * k), 1.8])
            sel = W[np.linalg.norm(W[:, :2] - c[:2], axis=1) < 30.0]
            sel = sel[rng.integers(0, sel.shape[0], rows)]
            loc = ((sel.astype(np.float64) - c) @ G.yaw(23.0 * k)).astype(np.float32)
            pool.append(np.concatenate([loc, rng.uniform(0, 1, (rows, 1)).astype(np.float32)], 1))
        ts = [np.array([(20 + 0.15 * k) * np.cos(0.05 * k), (20 + 0.15 * k) * np.sin(0.05 * k), 1.8]) for k in range(n_kf)]
        qs = [L.loop.quat_from_matrix(G.yaw(2.9 * k)) for k in range(n_kf)]
        ctx = L.Context(0)
        arch = L.KeyframeArchive(ctx, G.Q_BL, G.T_BL)
        gm = L.GlobalMap(arch)
        for k in range(n_kf):
            arch.push(None, None, pool[k % a.pool], 0.1 * k, ts[k], qs[k])
        n_raw, n_map = gm.build(ARCHIVE_FULL, 1, a.leaf)
        centre = ts[n_kf // 2]
        lo, hi = (centre - HALF).astype(np.float32), (centre + HALF).astype(np.float32)
        n_box, count_ms = G.timed(lambda: gm.crop_into(lo, hi, None, 0), a.reps)
        d_box = torch.empty((max(n_box, 1), 4), dtype=torch.float32, device="cuda")
        d_cnt = torch.empty(max(n_box, 1), dtype=torch.int32, device="cuda")
        _, device_ms = G.timed(lambda: gm.crop_into(lo, hi, d_box.data_ptr(), n_box, d_cnt.data_ptr()), a.reps)
        (h_rows, _), host_ms = G.timed(lambda: gm.crop(lo, hi), a.reps)
        d_all = torch.empty((n_map, 4), dtype=torch.float32, device="cuda")
        t_lo, t_hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()

        def full_copy_and_mask():
            gm.get_device(d_all.data_ptr(), n_map)
            xyz = d_all[:, :3]
            sel = d_all[((xyz >= t_lo) & (xyz <= t_hi)).all(1)]
            torch.cuda.synchronize()
            return sel
        sel, full_ms = G.timed(full_copy_and_mask, a.reps)
        rec = dict(rows_per_keyframe=rows, keyframes=n_kf, points=n_raw, voxels=n_map, leaf=a.leaf, box_lo=lo.tolist(), box_hi=hi.tolist(), voxels_in_box=n_box,
                   masked_centroids_in_box=int(sel.shape[0]), table_bytes=gm.info()[0], crop_count_ms=count_ms, crop_device_ms=device_ms, crop_host_ms=host_ms,
                   get_device_and_mask_ms=full_ms, device_rows_equal_host_rows=bool(np.array_equal(d_box.cpu().numpy().view(np.uint32), h_rows.view(np.uint32))))
        for key in ("crop_count_ms", "crop_device_ms", "crop_host_ms", "get_device_and_mask_ms"):
            rec[key + "_median"] = float(np.median(rec[key]))
        result[name] = rec
        print(name, json.dumps(rec), flush=True)
        del d_all, d_box, d_cnt, sel
        ctx.close()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
