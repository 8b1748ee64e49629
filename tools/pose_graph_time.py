"""Device time of the global pose graph's solve as the loop count grows: one drifting circuit of 8192 nodes (three laps), two bursts of loops at
stride 3 — the pattern of tests/pose_graph_many_loops_cases.loops_1024 — with 32 (the default cap), 64, 256 and 1024 loops.  32 loops leave the reduced system with
the single-workgroup solve (<= 768 unknowns); the others take the blocked Cholesky.  Per size: separators, reduced unknowns, iterations, and the device time of
lili_pose_graph_kernel_ms (events around every launch of the solve), two ways:
  solve      max_iterations = 10, the default: the launches of the iterations behind the last one return at their first instruction, but are launched
  iteration  max_iterations = the iterations the solve takes, divided by them
Every solve starts from reset; warmed up, then repeated; median and spread (min .. max).
    python tools/pose_graph_time.py [out.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
os.environ.setdefault("OMP_NUM_THREADS", "1")
import lili_om_amd as L              # noqa: E402
from tests import pose_graph_cases as Cs   # noqa: E402
from tests import pose_graph_many_loops_cases as Ms   # noqa: E402

A = L.api
WARM, REPS = 2, 7
SIZES = (32, 64, 256, 1024)


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def case(n_loops):
    h = n_loops // 2
    return Cs._looped(f"loops_{n_loops}", 8192, 64, Ms.burst(4200, 100, h, stride=3) + Ms.burst(6500, 2300, h, stride=3), var=0.1, ftol=1e-9, laps=3.0)


def solve(pg, c, **kw):
    pg.reset()
    pg.append(c["poses"])
    for a, b, m, v in c["loops"]:
        pg.add_loop(a, b, m, v)
    s = pg.solve(pg.options(**dict(c["options"], **kw)))
    return s, pg.kernel_ms()


def main():
    ctx = L.Context(0)
    pg = L.PoseGraph(ctx, max_loops=A.PG_MAX_LOOPS_EXT)
    rows = []
    for n_loops in SIZES:
        c = case(n_loops)
        n_sep = len(Ms.separators(c))
        s, _ = solve(pg, c)
        its = s["iterations"]
        for _ in range(WARM):
            solve(pg, c); solve(pg, c, max_iterations=its)
        full = [solve(pg, c)[1] for _ in range(REPS)]
        exact = [solve(pg, c, max_iterations=its)[1] / its for _ in range(REPS)]
        row = dict(loops=n_loops, nodes=8192, separators=n_sep, reduced=6 * n_sep, blocked=6 * n_sep > A.PG_MAX_REDUCED, tile=A.PG_REDUCED_TILE, iterations=its,
                   termination=s["termination"], solve_ms=stats(full), iteration_ms=stats(exact))
        rows.append(row)
        print(f"{n_loops} loops: {n_sep} separators, {6 * n_sep} reduced unknowns ({'blocked' if row['blocked'] else 'one workgroup'}), {its} iterations, termination "
              f"{s['termination']}: solve {row['solve_ms']['median']:.2f} ms ({row['solve_ms']['min']:.2f} .. {row['solve_ms']['max']:.2f}), per iteration "
              f"{row['iteration_ms']['median']:.2f} ms ({row['iteration_ms']['min']:.2f} .. {row['iteration_ms']['max']:.2f})", flush=True)
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fo:
            json.dump(dict(warm=WARM, reps=REPS, rows=rows), fo, indent=1)


if __name__ == "__main__":
    main()
