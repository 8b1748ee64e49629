"""Time of the pose graph's marginal covariances (lili_pose_graph_marginals; DESIGN.md §7k "Marginal covariances"), n = every node, no pairs, on
  N = 200 with 32 loops (tests/pose_graph_cases: max_loops), N = 2048 with 3 loops (circuit_2048), N = 32 768 with 4 loops (full_size), and
  N = 8192 with 32 / 64 / 256 / 1024 loops (the graphs of tools/pose_graph_time.py; 1024 loops = 12 360 reduced unknowns, the size no test runs).
Per graph: info.kernel_ms (events around the call's launches) and the host's wall time of the call, at the solved estimates; next to them the device time of ONE
solve iteration of the same graph from its given poses (max_iterations = 1): the work the call's front half repeats.  Warmed up, then repeated; median (min .. max).
    python tools/pose_graph_marginals_time.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
os.environ.setdefault("OMP_NUM_THREADS", "1")
import lili_om_amd as L              # noqa: E402
from tests import pose_graph_cases as Cs   # noqa: E402
from tests import pose_graph_many_loops_cases as Ms   # noqa: E402

A = L.api
WARM, REPS = 2, 7


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def circuit_8192(n_loops):
    h = n_loops // 2
    return Cs._looped(f"loops_{n_loops}", 8192, 64, Ms.burst(4200, 100, h, stride=3) + Ms.burst(6500, 2300, h, stride=3), var=0.1, ftol=1e-9, laps=3.0)


def graphs():
    by = {c["name"]: c for c in Cs.solve_cases()}
    yield by["max_loops"]
    yield by["circuit_2048"]
    yield Cs.full_size()
    for n_loops in (32, 64, 256, 1024):
        yield circuit_8192(n_loops)


def load(pg, c):
    pg.reset()
    pg.append(c["poses"])
    for a, b, m, v in c["loops"]:
        pg.add_loop(a, b, m, v)
    if c["estimates"] is not None:
        pg.set_poses(c["estimates"])


def one_iteration(pg, c):
    load(pg, c)
    pg.solve(pg.options(**dict(c["options"], max_iterations=1)))
    return pg.kernel_ms()


def marginals(pg):
    t0 = time.perf_counter()
    pg.marginals()
    return pg.last_marginals["kernel_ms"], 1e3 * (time.perf_counter() - t0)


def main():
    ctx = L.Context(0)
    pg = L.PoseGraph(ctx, max_loops=A.PG_MAX_LOOPS_EXT)
    rows = []
    for c in graphs():
        for _ in range(WARM):
            one_iteration(pg, c)
        it = [one_iteration(pg, c) for _ in range(REPS)]
        load(pg, c)
        s = pg.solve(pg.options(**c["options"]))
        for _ in range(WARM):
            marginals(pg)
        m = [marginals(pg) for _ in range(REPS)]
        info = pg.last_marginals
        row = dict(name=c["name"], nodes=info["n_nodes"], loops=info["n_loops"], reduced=info["reduced_unknowns"], blocked=info["reduced_unknowns"] > A.PG_MAX_REDUCED,
                   termination=s["termination"], kernel_ms=stats([v[0] for v in m]), wall_ms=stats([v[1] for v in m]), solve_iteration_ms=stats(it))
        rows.append(row)
        print(f"{c['name']}: N {row['nodes']}, {row['loops']} loops, {row['reduced']} reduced unknowns ({'blocked' if row['blocked'] else 'one workgroup'}): marginals kernels "
              f"{row['kernel_ms']['median']:.2f} ms ({row['kernel_ms']['min']:.2f} .. {row['kernel_ms']['max']:.2f}), wall {row['wall_ms']['median']:.2f} ms "
              f"({row['wall_ms']['min']:.2f} .. {row['wall_ms']['max']:.2f}); one solve iteration {row['solve_iteration_ms']['median']:.2f} ms "
              f"({row['solve_iteration_ms']['min']:.2f} .. {row['solve_iteration_ms']['max']:.2f})", flush=True)
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fo:
            json.dump(dict(warm=WARM, reps=REPS, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
