"""Time of the per-frame trajectory on the device (lili_local_graph: IMU walk + local pose graph in one launch): the blocking C call by the host clock (it
ends in a synchronisation) and its kernel by two HIP events around the launch (option "local_graph_time"), for n = 4 and n = 16 scans between two
keyframes at 200 Hz IMU and 0.1 s scans; for n = 2 as well, the most the reference's keyframe rule produces.
Every shape is warmed up, then repeated; median and spread (min .. max) are reported, with the iterations the solve took.
    python tools/local_graph_time.py [out.json]"""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import lili_om_amd as L          # noqa: E402
from lili_om_amd import api      # noqa: E402
from tests import local_graph_cases as Cs   # noqa: E402
from tests.local_graph_model import mat_to_quat   # noqa: E402

WARM, REPS = 10, 200


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ctx = L.Context(0)
    ctx.set_option("local_graph_time", 1)
    lg = L.LocalGraph(ctx)
    rows = []
    for n in (2, 4, 16):
        c = Cs._walk_case(f"time_n{n}", 900 + n, n)
        kw = Cs.walk_kwargs(c)
        _, (P, R, V), _ = lg.propagate(**kw)
        q = np.array(mat_to_quat(R.tolist()))      # the right keyframe's pose: the propagated end state, moved by centimetres as a window solve moves it
        right = np.concatenate([P + np.array([0.03, -0.02, 0.01]), q / np.linalg.norm(q)])
        for _ in range(WARM):
            poses, meas, info = lg.run(right, **kw)
        wk, _ = lg._walk(**kw)
        poses, meas, s = np.zeros((n, 7)), np.zeros((n + 1, 7)), api.LocalGraphSummary()
        call, kern = [], []
        ms = C.c_float(0)
        for _ in range(REPS):
            t0 = time.perf_counter()
            rc = lg.lib.lili_local_graph(ctx.h, C.byref(wk), n, api._ptr(right), None, api._ptr(poses), api._ptr(meas), C.byref(s))
            call.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0
            lg.lib.lili_local_graph_kernel_ms(ctx.h, C.byref(ms))
            kern.append(ms.value * 1e3)
        walk = []      # the walk alone (lili_local_graph_propagate): what of the kernel is the serial IMU chain
        end = np.zeros(15)
        for _ in range(REPS):
            assert lg.lib.lili_local_graph_propagate(ctx.h, C.byref(wk), n, api._ptr(poses), api._ptr(end), api._ptr(meas)) == 0
            lg.lib.lili_local_graph_kernel_ms(ctx.h, C.byref(ms))
            walk.append(ms.value * 1e3)
        row = dict(n=n, imu_hz=200, samples=int(wk.n_imu), iterations=int(s.lm.iterations), termination=api.LM_TERMINATION[s.lm.termination], c_call_us=stats(call), kernel_us=stats(kern),
                   walk_kernel_us=stats(walk))
        rows.append(row)
        print(f"n {n:2d}: C call {row['c_call_us']['median'] / 1e3:7.4f} ms ({row['c_call_us']['min'] / 1e3:.4f} .. {row['c_call_us']['max'] / 1e3:.4f})  "
              f"kernel {row['kernel_us']['median'] / 1e3:7.4f} ms ({row['kernel_us']['min'] / 1e3:.4f} .. {row['kernel_us']['max'] / 1e3:.4f})  "
              f"walk alone {row['walk_kernel_us']['median'] / 1e3:7.4f} ms  {row['iterations']} iterations, {row['termination']}", flush=True)
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(dict(warm=WARM, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
