"""Wall time of one keyframe's solve + sign unification + next prior + hand-over of that prior, two ways, on the harness windows (3 x (2 500 + 200) features):
  chain   the separate calls: WindowSolver.set_problem(IMU records, prior = the previous keyframe's prior as host arrays) + lili_window_solve + the host's unification +
          lili_window_marginalize — two uploads, two synchronisations, the prior read back and uploaded again with J0^T J0 recomputed on the host;
  cycle   WindowSolver.set_problem(the same IMU records, no prior) + lili_window_cycle with use_resident_prior = 1 — one upload, one synchronisation, the prior handed
          over on the device.
Both ways build their problem inside the timed region, once per keyframe, from the same pre-packed lili_window_imu records (a keyframe has new IMU factors either way); the
chain's first window moves its speed-bias means in place between solve and marginalisation instead of building the problem a second time.
Both on the SECOND window of the chain of tests/marg_harness.py (keyframes 1-3, the marginalisation-prior branch: the keyframe whose hand-over is the point), and on the
first (keyframes 0-2, speed-bias priors, no prior to hand over) for comparison.  3 warm-up rounds, then N >= 9 rounds with the ways alternating; medians and ranges, raw
values to profiles/window_cycle_time_<tag>.json (or --out).  --ways chain runs on a commit that has no lili_window_cycle yet.

    python tools/window_cycle_time.py [--n 9] [--tag mi355x] [--out path] [--ways chain,cycle]
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
from tests import marg_harness as MH  # noqa: E402
from tests import test_window_solve_gpu as S  # noqa: E402


def unify(state):
    s = np.array(state, np.float64)
    for k in range(s.shape[0]):
        if s[k, 3] < 0:
            s[k, 3:7] = -s[k, 3:7]
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ways", default="chain,cycle")
    a = ap.parse_args()
    n_rep = max(9, a.n)
    which = a.ways.split(",")
    win = S.cut(MH.win4(), 0, 3)
    nxt = MH.second_window()[0]
    ctx = L.Context(0)
    # one context per window: each keeps its own slots' associations, as two consecutive keyframes of a run would after their prepare
    ctx2 = L.Context(0)
    mt1, mt2 = S.gpu_side(ctx, win), S.gpu_side(ctx2, nxt)
    ws1 = S.window_problem(L.WindowSolver(ctx, mt1), win, 3)
    ws2 = L.WindowSolver(ctx2, mt2)
    pres2 = [p["pre"] for p in nxt["pres"]]
    s1, s2 = S.state_of(win, 3), S.state_of(nxt, 3)
    sb_init = np.full((3, 9), np.nan)
    sb_init[0], sb_init[1] = win["init"][0]["sb"], win["init"][1]["sb"]
    # the IMU records packed once: both ways get the same WindowImu objects, so every timed set_problem below costs the same on that side
    imu1 = [L.api.pack_preintegration(p["pre"]) for p in win["pres"]]
    imu2 = [L.api.pack_preintegration(p["pre"]) for p in nxt["pres"]]

    def chain_first():
        ws1.set_problem([0, 1, 2], S.MASK, imu=imu1, sb_prior=sb_init)
        final, _ = ws1.solve(s1)
        uni = unify(final)
        sb = np.ctypeslib.as_array(ws1.problem.sb_prior, shape=(3, 9))
        sb[0], sb[1] = uni[0, 7:16], uni[1, 7:16]                        # the first marginalisation's speed-bias priors: mean = the solved speed-bias (L:1045-1057), in place
        return ws1.marginalize(uni)

    prior1 = chain_first()

    def chain_second():
        ws2.set_problem([0, 1, 2], S.MASK, imu=imu2, prior=prior1)       # the hand-over: the prior goes in as host arrays, J0^T J0 is recomputed, everything is uploaded
        final, _ = ws2.solve(s2)
        return ws2.marginalize(unify(final))

    ways = {}
    if "chain" in which:
        ways["chain_first_us"] = chain_first
        ways["chain_second_us"] = chain_second
    if "cycle" in which:
        ws1c, ws2c = L.WindowSolver(ctx, mt1), L.WindowSolver(ctx2, mt2)
        ws2c.set_resident_prior(prior1)

        def cycle_first():
            ws1c.set_problem([0, 1, 2], S.MASK, imu=imu1, sb_prior=sb_init)      # a keyframe has new IMU factors: the same problem construction as the chain's
            return ws1c.cycle(s1)

        def cycle_second():
            ws2c.set_problem([0, 1, 2], S.MASK, imu=imu2)                        # the same, without the prior: it is on the device
            return ws2c.cycle(s2, use_resident_prior=True)

        def reseed():
            # every round starts from the FIRST window's prior, as chain_second does; re-seeding is not part of a keyframe (the previous cycle leaves the prior there)
            ws2c.set_resident_prior(prior1)

        ways["cycle_first_us"] = cycle_first
        ways["cycle_second_us"] = cycle_second
    else:
        reseed = None

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    for _ in range(3):
        for fn in ways.values():
            fn()
            if reseed:
                reseed()
    raw = {k: [] for k in ways}
    for _ in range(n_rep):
        for k, fn in ways.items():
            raw[k].append(timed(fn))
            if reseed:
                reseed()
    med = {k: statistics.median(v) for k, v in raw.items()}
    rng = {k: (min(v), max(v)) for k, v in raw.items()}
    out = dict(window="3 x (2500 surf + 200 edge); first = keyframes 0-2 with speed-bias priors, second = keyframes 1-3 with the first's prior", n=n_rep, ways=which,
               median=med, range=rng, raw=raw)
    path = a.out or os.path.join(ROOT, "profiles", f"window_cycle_time_{a.tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(median=med, range=rng)))
    ctx2.close()
    ctx.close()


if __name__ == "__main__":
    main()
