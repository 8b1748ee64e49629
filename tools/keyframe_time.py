"""Time of the keyframe hand-over: one keyframe at the reference's sizes — Livox 24 k full / 20 k surf / ~70 edge points, ROT ~130 k full — from "the
frame's extraction is done" to three deskewed device clouds that lili_backend_keyframe_prepare and lili_archive_push take, two ways:
  device   lili_frontend_keyframe (one launch on the extractor's own lists) + a synchronisation
  host     the route without it: the three clouds to the host (16-byte rows; copied here with lili_frontend_keyframe_get at deskew 0, a caller of the earlier library
           copied the lili_extract_*_device views itself), undistortion in numpy (f64, vectorised, tests/keyframe_model.py), the three clouds uploaded again
Every route is warmed up, then repeated; median and spread (min .. max) by the host clock.
    python tools/keyframe_time.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
os.environ.setdefault("OMP_NUM_THREADS", "1")
import torch                         # noqa: E402
import lili_om_amd as L              # noqa: E402
from lili_om_amd import synth        # noqa: E402
from tests import keyframe_model as M   # noqa: E402
from tests import seq_harness as H   # noqa: E402

A = L.api
WARM, REPS = 10, 100
T_REL = np.array([0.4371, -0.0213, 0.0077])


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def device_route(ctx, flavour):
    t0 = time.perf_counter()
    A.frontend_keyframe(ctx, flavour, T_REL, None, True)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e6


def host_route(ctx, flavour, time_cols):
    """time_cols: per cloud the (n,) time channel on the host, or None where the 16-byte row carries it as its 4th float"""
    t0 = time.perf_counter()
    A.frontend_keyframe(ctx, flavour, None, None, False)
    rows = [A.frontend_keyframe_get(ctx, kind) for kind in range(3)]
    t1 = time.perf_counter()
    moved = [np.c_[M.undistort(r[:, :3], r[:, 3] if tc is None else tc, T_REL), r[:, 3]].astype(np.float32) for r, tc in zip(rows, time_cols)]
    t2 = time.perf_counter()
    dev = [torch.from_numpy(m).cuda() for m in moved]
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del dev
    return (t3 - t0) * 1e6, (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6


def measure(ctx, flavour, time_cols, label, sizes):
    for _ in range(WARM):
        device_route(ctx, flavour); host_route(ctx, flavour, time_cols)
    dev = [device_route(ctx, flavour) for _ in range(REPS)]
    host = np.array([host_route(ctx, flavour, time_cols) for _ in range(REPS)])
    row = dict(flavour=label, sizes=sizes, device_us=stats(dev), host_us=stats(host[:, 0]), host_download_us=stats(host[:, 1]), host_numpy_us=stats(host[:, 2]),
               host_upload_us=stats(host[:, 3]))
    row["ratio"] = row["host_us"]["median"] / row["device_us"]["median"]
    print(f"{label} {sizes}: device {row['device_us']['median']:.1f} us ({row['device_us']['min']:.1f} .. {row['device_us']['max']:.1f}), "
          f"host {row['host_us']['median']:.1f} us ({row['host_us']['min']:.1f} .. {row['host_us']['max']:.1f}) = download {row['host_download_us']['median']:.1f} + numpy "
          f"{row['host_numpy_us']['median']:.1f} + upload {row['host_upload_us']['median']:.1f}; ratio {row['ratio']:.1f}", flush=True)
    return row


def main():
    rows = []
    ctx = L.Context(0)
    # Livox: a scan of the front-end sequence (24 k points)
    scan = np.ascontiguousarray(H.make_frames(5)[4], np.float32)
    f = A.LivoxExtractor(ctx).extract(scan)
    sizes = dict(edge=int(f["edge"].shape[0]), surf=int(f["surf"].shape[0]), full=int(f["cutted"].shape[0]))
    time_cols = [np.ascontiguousarray(f["edge"][:, 6]), np.ascontiguousarray(f["surf"][:, 6]), None]      # edge / surf rows carry the curvature: their time channel comes from the host lists
    rows.append(measure(ctx, A.VARIANT_LIVOX, time_cols, "livox", sizes))
    # ROT: a 64-ring scan of ~130 k points
    w = synth.make_workload(n_map=200_000, n_az=2040, half_extent=(150.0, 150.0), verbose=False)
    raw = np.concatenate([w["scan_xyz"], np.full((w["scan_xyz"].shape[0], 1), 50.0, np.float32)], 1).astype(np.float32)
    d_raw = torch.from_numpy(raw).cuda()
    n_full, n_edge, n_surf = A.RotExtractor(ctx, n_scans=64, ds_rate=4).extract_device(d_raw.data_ptr(), raw.shape[0])
    rows.append(measure(ctx, A.VARIANT_ROT, [None, None, None], "rot", dict(edge=int(n_edge), surf=int(n_surf), full=int(n_full))))
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fo:
            json.dump(dict(warm=WARM, reps=REPS, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
