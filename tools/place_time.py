"""Place-recognition timing: medians of --reps after one warm-up, wall clock around the blocking calls.
  a. lili_place_update per keyframe, for Livox-sized (24 k rows) and ROT-sized (130 k rows) full clouds: every call rebuilds the descriptors of the whole archive
     (two parameter sets that differ in lidar_height alternate), so a call's time over the keyframe count is the cost of one keyframe inside a large update; and the
     update of ONE new keyframe, which is what a running session pays;
  b. lili_place_search at 1 000 and 10 000 described keyframes, with 1 and 64 queries, k = 10;
  c. for comparison the same exact search (all candidates, all shifts) in numpy on the host: unit columns, one batched matrix product per query, the wrapped
     diagonals gathered by index.
  d. (--submap) levelled submap descriptors at back 20 / fwd 2: the update of the whole archive (two parameter sets alternate, as in a.), the steady-state update of
     one new keyframe (fwd + 1 descriptors), and the full rebuild after every pose of a 1 000-keyframe archive changed.  --build-probe compiles the library once more
     with k_place_cells_sub replaced by the global-atomic form (a tool-only build, never shipped) into tools/_probe/place_global/; run --submap with
     LILI_HIP_LIBRARY pointing there to time that form on the same segment tables.
No number here is a gate.

    python tools/place_time.py [--reps 7] [--out profiles/place_time.json]
    python tools/place_time.py --build-probe
    python tools/place_time.py --submap [--out FILE]
    LILI_HIP_LIBRARY=tools/_probe/place_global/liblili_hip.so python tools/place_time.py --submap [--out FILE]
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


def build_probe():
    """the library with lili_place.hip compiled under -DLILI_PLACE_PROBE_GLOBAL, every other object as built -> tools/_probe/place_global/liblili_hip.so"""
    import glob
    import subprocess
    cs, out = os.path.join(ROOT, "lili_om_amd", "csrc"), os.path.join(ROOT, "tools", "_probe", "place_global")
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(out, "lili_place_global.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                           "-DLILI_PLACE_PROBE_GLOBAL", "-c", os.path.join(cs, "lili_place.hip"), "-o", obj])
    others = [o for o in sorted(glob.glob(os.path.join(cs, "*.o"))) if os.path.basename(o) != "lili_place.o"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out, "liblili_hip.so"), obj] + others)
    print(os.path.join(out, "liblili_hip.so"))


def submap_times(a):
    """d.: keyframes 2 m apart down a street, a few degrees of roll and pitch each, described at back 20 / fwd 2, levelled"""
    rng = np.random.default_rng(9)
    form = "global" if "place_global" in os.environ.get("LILI_HIP_LIBRARY", "") else "lds"
    result = dict(form=form, back=20, fwd=2, level=1)

    def pose(k):
        r, p = np.radians(rng.uniform(-3, 3, 2))
        q = np.array([1.0, r / 2, p / 2, np.radians(rng.uniform(-5, 5)) / 2])
        return [2.0 * k, rng.uniform(-0.5, 0.5), 0.0], q / np.linalg.norm(q)

    for name, rows, n_kf in (("livox_24k", 24_000, 400), ("rot_130k", 130_000, 100), ("livox_24k_1000", 24_000, 1000)):
        ctx = L.Context(0)
        arch = L.KeyframeArchive(ctx)
        pool = [cloud(rng, rows) for _ in range(8)]
        for k in range(n_kf):
            arch.push(None, None, pool[k % 8], 0.1 * k, *pose(k))
        pr = [L.PlaceRecognition(arch, lidar_height=h, back=20, fwd=2, level=True) for h in (2.0, 1.9)]
        flip = [0]
        rec = dict(rows_per_keyframe=rows, keyframes=n_kf, rows_binned_in_a_full_update=int(sum(min(n_kf - 1, i + 2) - max(0, i - 20) + 1 for i in range(n_kf))) * rows)
        if n_kf < 1000:
            def rebuild():
                flip[0] ^= 1
                return pr[flip[0]].update()
            built, all_ms = timed(rebuild, a.reps)
            assert built == n_kf
            one_ms = []
            for r in range(a.reps + 1):
                arch.push(None, None, pool[r % 8], 0.1 * (n_kf + r), *pose(n_kf + r))
                t0 = time.perf_counter()
                assert pr[flip[0]].update() == 3
                if r:
                    one_ms.append((time.perf_counter() - t0) * 1e3)
            rec.update(update_all_ms=all_ms, update_all_ms_median=float(np.median(all_ms)), update_one_ms=one_ms, update_one_ms_median=float(np.median(one_ms)),
                       g_rows_per_s_in_a_full_update=rec["rows_binned_in_a_full_update"] / float(np.median(all_ms)) * 1e-6)
        else:
            assert pr[0].update() == n_kf
            ts, qs, _ = arch.poses()

            def correct():
                ts[:, 1] += 0.01 * np.arange(n_kf) / n_kf      # a pose correction that grows along the trajectory: every relative placement changes
                arch.set_poses(0, ts, qs)
            built, ms = timed(pr[0].update, a.reps, before=correct)
            assert built == n_kf
            rec.update(rebuild_after_set_poses_ms=ms, rebuild_after_set_poses_ms_median=float(np.median(ms)))
        result["submap_" + name] = rec
        print("submap", form, name, json.dumps(rec), flush=True)
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--submap", action="store_true")
    ap.add_argument("--build-probe", action="store_true")
    a = ap.parse_args()
    if a.build_probe:
        return build_probe()
    if a.submap:
        return submap_times(a)
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
