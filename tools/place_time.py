"""Place-recognition timing: medians of --reps after one warm-up, wall clock around the blocking calls.
  a. lili_place_update per keyframe, for Livox-sized (24 k rows) and ROT-sized (130 k rows) full clouds: every call rebuilds the descriptors of the whole archive
     (two parameter sets that differ in lidar_height alternate), so a call's time over the keyframe count is the cost of one keyframe inside a large update; and the
     update of ONE new keyframe, which is what a running session pays;
  b. lili_place_search at 1 000 and 10 000 described keyframes, with 1 and 64 queries, k = 10;
  c. for comparison the same exact search (all candidates, all shifts) in numpy on the host: unit columns, one batched matrix product per query, the wrapped
     diagonals gathered by index.
No number here is a gate.

    python tools/place_time.py [--reps 7] [--out profiles/place_time.json]
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


def cloud(rng, rows):
    """a street-like scan: ground, and structures of random height at random bearings"""
    a, r = rng.uniform(0, 2 * np.pi, rows), 80.0 * np.sqrt(rng.uniform(0, 1, rows))
    z = np.where(rng.uniform(size=rows) < 0.6, -1.8, rng.uniform(-1.8, 9.0, rows))
    return np.stack([r * np.cos(a), r * np.sin(a), z, rng.uniform(0, 1, rows)], 1).astype(np.float32)


def host_search(descs, query, k):
    """the exact search in numpy: (ids, shifts, distances) of the k best"""
    n, ns, _ = descs.shape
    B = descs.astype(np.float64)
    nb = np.sqrt((B * B).sum(2))
    Bu = np.divide(B, nb[:, :, None], out=np.zeros_like(B), where=nb[:, :, None] > 0)
    A = query.astype(np.float64)
    na = np.sqrt((A * A).sum(1))
    Au = np.divide(A, na[:, None], out=np.zeros_like(A), where=na[:, None] > 0)
    cos = np.matmul(Au[None], Bu.transpose(0, 2, 1))                          # [c, j, l]
    valid = (na > 0)[None, :, None] & (nb > 0)[:, None, :]
    j = np.arange(ns)
    l = (j[None, :] + j[:, None]) % ns                                        # l[s, j]
    total, count = cos[:, j[None, :], l].sum(2), valid[:, j[None, :], l].sum(2)
    d = np.where(count > 0, 1.0 - total / np.maximum(count, 1), np.inf)       # [c, s]
    shift = d.argmin(1)
    best = d[np.arange(n), shift]
    order = np.lexsort((np.arange(n), best))[:k]
    return order, shift[order], best[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(9)
    result = {}
    # a. update
    for name, rows, n_kf in (("livox_24k", 24_000, 400), ("rot_130k", 130_000, 100)):
        ctx = L.Context(0)
        arch = L.KeyframeArchive(ctx)
        pool = [cloud(rng, rows) for _ in range(8)]
        for k in range(n_kf):
            arch.push(None, None, pool[k % 8], 0.1 * k, [k, 0, 0], [1, 0, 0, 0])
        pr = [L.PlaceRecognition(arch, lidar_height=h) for h in (2.0, 1.9)]
        flip = [0]

        def rebuild():
            flip[0] ^= 1
            return pr[flip[0]].update()
        built, all_ms = timed(rebuild, a.reps)
        assert built == n_kf
        one_ms = []
        for r in range(a.reps + 1):
            arch.push(None, None, pool[r % 8], 0.1 * (n_kf + r), [0, 0, 0], [1, 0, 0, 0])
            t0 = time.perf_counter()
            assert pr[flip[0]].update() == 1
            if r:
                one_ms.append((time.perf_counter() - t0) * 1e3)
        result["update_" + name] = dict(rows_per_keyframe=rows, keyframes=n_kf, update_all_ms=all_ms, update_all_ms_median=float(np.median(all_ms)),
                                        us_per_keyframe_in_a_full_update=float(np.median(all_ms)) * 1e3 / n_kf, update_one_ms=one_ms,
                                        update_one_ms_median=float(np.median(one_ms)), store_bytes=pr[0].info()[2])
        print("update", name, json.dumps(result["update_" + name]), flush=True)
        ctx.close()
    # b. / c. search
    ctx = L.Context(0)
    arch = L.KeyframeArchive(ctx)
    pr = L.PlaceRecognition(arch)
    for n_kf in (1_000, 10_000):
        while len(arch) < n_kf:
            k = len(arch)
            arch.push(None, None, cloud(rng, 400), float(k), [k, 0, 0], [1, 0, 0, 0])
        t0 = time.perf_counter()
        pr.update()
        rec = dict(keyframes=n_kf, update_ms=(time.perf_counter() - t0) * 1e3)
        for n_q in (1, 64):
            qs = [int(q) for q in rng.integers(0, n_kf, n_q)]
            hits, ms = timed(lambda: pr.search(qs, k=10, min_time_gap=30.0), a.reps)
            rec[f"search_{n_q}q_ms"] = ms
            rec[f"search_{n_q}q_ms_median"] = float(np.median(ms))
        descs = np.stack([pr.descriptor(k) for k in range(n_kf)])
        q0 = qs[0]
        (ids, shifts, dist), hms = timed(lambda: host_search(descs, descs[q0], 12), min(a.reps, 3))
        keep = [(int(c), int(s), float(d)) for c, s, d in zip(ids, shifts, dist) if abs(c - q0) > 30][:10]      # (the host search ignores the time gap: drop those rows here)
        dev = pr.search([q0], k=10, min_time_gap=30.0)[0]
        rec.update(host_search_1q_ms=hms, host_search_1q_ms_median=float(np.median(hms)), host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_agrees=bool([(c, s) for c, s, _ in dev][:len(keep)] == [(c, s) for c, s, _ in keep]),
                   host_max_distance_difference=float(max([abs(x[2] - y[2]) for x, y in zip(dev, keep)] or [0.0])))
        result[f"search_{n_kf}"] = rec
        print("search", n_kf, json.dumps(rec), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
