"""Time of the IMU pre-integration on the device (lili_imu_preintegrate): the blocking call by the host clock (it ends in a synchronisation) and its kernel
by two HIP events around the launch (option "imu_time"), n in {100, 200, 400} samples per segment x {1, 3, 64} segments; for context the reference's own
header (oracle/_ref/libref_imu.so::ref_preintegrate, where built) and the oracle's numpy restatement on one CPU thread of the same box.
Every shape is warmed up, then repeated; median and spread (min .. max) are reported.
    python tools/preint_time.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
os.environ.setdefault("OMP_NUM_THREADS", "1")
import lili_om_amd as L          # noqa: E402
from oracle import lo_window as W   # noqa: E402
from tests import preint_model as M   # noqa: E402

WARM, REPS = 10, 100


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ctx = L.Context(0)
    ctx.set_option("imu_time", 1)
    pi = L.ImuPreintegrator(ctx)
    lib = M.ref_library()
    rows = []
    for n in (100, 200, 400):
        segs_all = []
        for s in range(64):
            dt, acc, gyr, ba, bg = M._samples(1 + s, n)
            dt[0] = 0.0
            segs_all.append(dict(dt=dt, acc=acc[1:], gyr=gyr[1:], acc0=acc[0], gyr0=gyr[0], ba=ba, bg=bg))
        for n_seg in (1, 3, 64):
            segs = segs_all[:n_seg]
            for _ in range(WARM):
                pi.preintegrate(segs)
            call, kern = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                pi.preintegrate(segs)
                call.append((time.perf_counter() - t0) * 1e6)
                kern.append(pi.kernel_ms() * 1e3)
            # the C call alone (the Python wrapper packs n_seg ctypes structs per call): pack once, call REPS times
            packed, keep, flags = pi._pack(segs)
            out = (L.api.WindowImu * n_seg)()
            c_call = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                pi.lib.lili_imu_preintegrate(ctx.h, packed, n_seg, out, None)
                c_call.append((time.perf_counter() - t0) * 1e6)
            row = dict(n=n, n_seg=n_seg, python_call_us=stats(call), c_call_us=stats(c_call), kernel_us=stats(kern))
            rows.append(row)
            print(f"n {n:3d} x {n_seg:2d} segments: C call {row['c_call_us']['median']:8.1f} us ({row['c_call_us']['min']:.1f} .. {row['c_call_us']['max']:.1f})  "
                  f"kernel {row['kernel_us']['median']:8.1f} us ({row['kernel_us']['min']:.1f} .. {row['kernel_us']['max']:.1f})  through Python {row['python_call_us']['median']:8.1f} us", flush=True)
        # one CPU thread, one segment
        s = segs_all[0]
        cpu = {}
        if lib is not None:
            t = []
            for _ in range(5 + 30):
                t0 = time.perf_counter()
                M.ref_preintegrate(lib, s["dt"], s["acc"], s["gyr"], s["acc0"], s["gyr0"], s["ba"], s["bg"])
                t.append((time.perf_counter() - t0) * 1e6)
            cpu["reference_header_us"] = stats(t[5:])
        t = []
        for _ in range(1 + 3):
            t0 = time.perf_counter()
            pre = W.Preintegration(s["acc0"], s["gyr0"], s["ba"], s["bg"])
            for k in range(n):
                pre.push_back(s["dt"][k], s["acc"][k], s["gyr"][k])
            t.append((time.perf_counter() - t0) * 1e6)
        cpu["oracle_numpy_us"] = stats(t[1:])
        rows.append(dict(n=n, n_seg=1, **cpu))
        print(f"n {n:3d}, one CPU thread: " + "  ".join(f"{k} {v['median']:.1f}" for k, v in cpu.items()), flush=True)
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(dict(warm=WARM, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
