#!/usr/bin/env python
"""bench.py — scan-to-map iterations/s on MI355X (BASELINE.json metric, config 2/3).

One STEP = one outer scan-to-map iteration over one 200 k-point scan against the 5 M-point local map:
re-associate (transform + exact 5-NN + plane fit + gates) -> linearise (residual + Jacobian + Cauchy
corrector + Gram reduction) -> [all-reduce of counts and Gram when --gpus > 1] -> Gauss-Newton update
of the pose, all on the device, inputs resident in HBM before the timed region starts.

    python bench.py                      # 1 GPU: set-up, warm-up, the timed steps, the result line
    python bench.py --full               # + roofline, CPU baseline and pose parity, extras (other configs, stages, regions)
    python bench.py --dump-outputs DIR   # + what the last timed step computed, as DIR/<name>.npy
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (see DESIGN.md §6 for the roofline / cpu_baseline definitions).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_MAP = 5_000_000
N_AZ = 3125            # x 64 rings = 200 000 rays
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md §Chip-level parameters)
POSE_TOL_M, POSE_TOL_RAD = 1e-4, 1e-4   # north star: pose deltas within 1e-4 m / 1e-4 rad of the reference CPU path
BYTES_PER_QUERY = 96   # algorithmic bytes of one outer iteration per query: 16 B query + 5 x 16 B neighbours


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def body_pose_for_lidar(L, P, lidar_t):
    """Body pose (T, Q) whose LiDAR frame coincides with the generator's LiDAR frame."""
    qlb = np.array(list(P.q_lb))
    qb = qlb / np.linalg.norm(qlb)
    _, T2 = L.api.assoc_transform([0.0, 0.0, 0.0], qb, P)
    return np.asarray(lidar_t) - T2, qb


def ring_major(scan_xyz, ring):
    """Order the extractor hands features over in: ring by ring (R/src/Preprocessing.cpp:377-382,401)."""
    order = np.argsort(ring, kind="stable")
    return scan_xyz[order]


def single_socket_cpus():
    """One logical CPU per physical core of socket 0 (the north star asks for a single-socket CPU baseline); None if the
    topology cannot be read."""
    try:
        base = "/sys/devices/system/cpu"
        seen, cpus = set(), []
        allowed = sorted(os.sched_getaffinity(0))
        for c in allowed:
            pkg = int(open(f"{base}/cpu{c}/topology/physical_package_id").read())
            core = int(open(f"{base}/cpu{c}/topology/core_id").read())
            if pkg != int(open(f"{base}/cpu{allowed[0]}/topology/physical_package_id").read()):
                continue
            if (pkg, core) not in seen:
                seen.add((pkg, core)); cpus.append(c)
        return cpus or None
    except Exception:   # noqa: BLE001
        return None


def dump_outputs(out_dir, m, n_q):
    """What the last timed step handed back through slot 0, one float32 / float64 .npy per array (about 9 MB at 200 k queries): the pose
    after its Gauss-Newton update, that step (dt, rotation vector) and its status, and the surf correspondences of its association in
    query order (the library copies them out ordered, so equal inputs give equal files)."""
    os.makedirs(out_dir, exist_ok=True)
    t, q, st = m.pose_get(0)
    delta, _, _ = m.last_step(0)
    rec = m.surf_records(0, n_q)
    arrays = {"pose_t": t, "pose_q": q, "gn_status": np.array([st], np.float64), "last_step_delta": delta,
              "surf_query_index": rec["query_index"].astype(np.float64), "surf_cur_pt": rec["cp"], "surf_normal": rec["n"],
              "surf_neg_oa_dot_norm": rec["d"], "surf_score": rec["score"]}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def cpu_baseline(w, queries, t0, q0):
    """The oracle (CPU restatement of the reference path) on the host cores of ONE socket, threads pinned to its physical cores: kd-tree build once, then whole
    registrations of 10 outer iterations, each ONE C call (oracle/lo_s2m.cpp::lo_register_surf: association, linearisation and Gauss-Newton step on a persistent
    thread pool that hands out 1 k-query chunks dynamically — round 5; rounds 1-4 spawned the threads per stage with static ranges and went through Python between
    the stages: 9x on 64 cores).  The rate is the MEDIAN of 5 registrations; beside it the single-thread figure of the same call, the parallel efficiency
    value / (cores x single thread), and — where the prebuilt oracle/_ref travelled along — the reference's own association + residual-block functions on one
    thread (serial, like the reference runs them).  Reported baseline only."""
    from oracle import oracle as O
    import lili_om_amd as L
    PO = O.params("rot")
    P = L.make_params("rot")
    import bench_configs as BC
    cpus = single_socket_cpus()
    quota = BC.cpu_quota_cores()
    if cpus and quota and quota < len(cpus):
        cpus = cpus[:quota]                 # the container's CPU quota (cgroup): more threads than that are throttled, not run
    old_aff = os.sched_getaffinity(0)
    n_threads = len(cpus) if cpus else min(os.cpu_count() or 1, quota or (os.cpu_count() or 1))
    if cpus:
        os.sched_setaffinity(0, cpus)       # BEFORE the map copy and the tree build: their pages are first touched by this thread, i.e. land on the socket whose cores will
                                            # search them (round 5: with the map on the other socket four of five registrations ran at 100 it/s and one at 255)
    map_local = np.array(w["map_xyz"], dtype=np.float32, order="C", copy=True)
    t_build = time.perf_counter()
    tree = O.KdTree(map_local)
    t_build = time.perf_counter() - t_build
    q32 = np.array(queries, dtype=np.float32, order="C", copy=True)

    def run(nth, iters):
        tic = time.perf_counter()
        t, q, applied, _ = O.register_surf(tree, q32, t0, q0, PO, 1000.0, iters, nth)
        return (time.perf_counter() - tic) / iters, t, q, applied

    try:
        O.pool_reset()                                      # workers are created under the socket's affinity mask, one pinned per core (cores 1 .. n-1 of the mask)
        run(n_threads, 2); run(n_threads, 2)                # warm-up (page-in, thread start and placement)
        if cpus:
            os.sched_setaffinity(0, {cpus[0]})              # the calling thread works too: on the one core of the mask that has no worker
        rates, t_fin, q_fin = [], None, None
        for _ in range(5):
            it, t_fin, q_fin, _ = run(n_threads, 10)
            rates.append(1.0 / it)
        runs_in_order = [round(r, 2) for r in rates]
        it1 = min(run(1, 2)[0] for _ in range(2))
    finally:
        O.pool_reset()
        os.sched_setaffinity(0, old_aff)
    rates.sort()
    ref = None
    try:
        from oracle import ref as R
        if R.available():
            z4 = np.zeros((0, 4), np.float32)
            map4 = np.concatenate([w["map_xyz"], np.zeros((w["map_xyz"].shape[0], 1), np.float32)], 1)
            q4 = np.concatenate([queries, np.zeros((queries.shape[0], 1), np.float32)], 1)
            Q2, T2 = L.api.assoc_transform(t0, q0, P)
            tic = time.perf_counter()
            srec, erec = R.backend_associate("rot", map4, z4, q4, z4, Q2, T2, PO.kd_max_radius, PO.surf_dist_thres, PO.lidar_const, 0.0)
            R.backend_rows("rot", srec, erec, list(P.q_lb), list(P.t_lb), t0, q0)
            t_ref = time.perf_counter() - tic - t_build      # its setInputCloud builds the same kd-tree once more
            ref = dict(value=round(1.0 / max(t_ref, 1e-9), 3), unit="scan-to-map iterations/s", cores=1, kind="reference",
                       correspondences=int(len(srec)),
                       sample="ONE iteration through the reference's own transformPoint / findCorrespondingSurfFeatures / LidarPlaneNormFactor "
                              "(oracle/_ref: BackendFusion.cpp text compiled as is; kd-tree and QR are the oracle's stand-ins), serial like the reference")
    except Exception as e:      # noqa: BLE001
        ref = dict(error=repr(e))
    med = rates[len(rates) // 2]
    host_logical = os.cpu_count() or 0
    try:      # physical cores of the first socket, whether this process may run on them or not
        socket_cores = len({open(f"/sys/devices/system/cpu/{d}/topology/core_id").read().strip() for d in os.listdir("/sys/devices/system/cpu")
                            if d[3:].isdigit() and d.startswith("cpu") and os.path.exists(f"/sys/devices/system/cpu/{d}/topology/physical_package_id")
                            and open(f"/sys/devices/system/cpu/{d}/topology/physical_package_id").read().strip() == "0"})
    except Exception:   # noqa: BLE001
        socket_cores = 0
    eff = med * it1 / n_threads
    extrap = None
    if socket_cores > n_threads:      # say what a whole socket would give if it kept this efficiency (upper) or lost a third of it (lower) — not measured
        extrap = dict(socket_physical_cores=socket_cores, iterations_per_s_range=[round(socket_cores / it1 * eff * 0.67, 1), round(socket_cores / it1 * eff, 1)],
                      note="extrapolation: (cores of one socket) x (single-thread rate) x (measured parallel efficiency, and 2/3 of it); the container cannot run more threads than its quota")
    return dict(value=round(med, 3), unit="scan-to-map iterations/s", cores=n_threads, kind="port", host_logical_cpus=host_logical,
                cores_note=(f"{n_threads} of the host's {host_logical} logical CPUs: the container's cgroup CPU quota, not a socket — a full-socket figure cannot be measured here"
                            if quota and quota < host_logical else f"{n_threads} physical cores of one socket"),
                full_socket_extrapolation=extrap,
                runs=[round(r, 2) for r in rates], runs_in_order=runs_in_order, pinned=bool(cpus), cpu_quota_cores=quota, single_thread_value=round(1.0 / it1, 3),
                parallel_efficiency=round(med * it1 / n_threads, 3),
                kdtree_build_s=round(t_build, 3), reference_1thread=ref,
                sample=(f"oracle (g++ -O3, no -march, exact kd-tree): median of 5 registrations x 10 full outer iterations of the same 200k-query / "
                        f"5M-point workload, each registration one C call on a persistent pool of {n_threads} threads (dynamic 256-query chunks) pinned to physical "
                        f"cores of one socket (as many as the container's CPU quota allows: {quota if quota else 'no quota'}); kd-tree build excluded (once per keyframe)")), t_fin, q_fin


def secondary_stages(L, ctx, w, torch):
    """Stages either side of the matcher, each as units/s with its algorithmic-byte roofline
    (ROT extraction 20 B/point, Livox 48 B/point + the 6 x 4000 grid, map build 36 B/point).  Wall time of the C-ABI
    call on an idle stream; device-resident variants where the ABI takes device clouds.  Secondary figures, never the headline."""
    import ctypes as C
    from lili_om_amd import synth
    out = {}

    def rate(fn, reps, warm=2):
        """Steady-state time per call: the timed loop runs twice and the faster pass counts — the first pass of a transfer-heavy stage after other work still
        pays for the PCIe link / clocks ramping up (ROT from page-locked buffers: 0.36 ms in the first 50 calls, 0.22 ms from then on; tools/rot_host_time.py)."""
        for _ in range(warm):
            fn()
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            tic = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            sec = (time.perf_counter() - tic) / reps
            best = sec if best is None else min(best, sec)
        return best

    def entry(sec, alg_bytes, unit, note):
        return {"value": round(1.0 / sec, 1), "unit": unit, "ms": round(sec * 1e3, 4), "algorithmic_bytes": int(alg_bytes),
                "hbm_frac": round(alg_bytes / sec / 1e9 / HBM_PEAK_GBS, 6), "note": note}

    # --- ROT extractor on the raw 200 k-point scan (R/src/Preprocessing.cpp:277-527)
    raw = np.concatenate([w["scan_xyz"], np.full((w["scan_xyz"].shape[0], 1), 10.0, np.float32)], 1)
    ex = L.RotExtractor(ctx, n_scans=64, ds_rate=4)
    r = ex.extract(raw)
    n_e, n_s = len(r["edge"]), len(r["surf"])
    praw = L.api.PinnedArray(raw.shape, np.float32)
    praw.array[...] = raw
    ex.extract(praw.array, reuse=True)
    sec = rate(lambda: ex.extract(praw.array, reuse=True), 50)
    out["extract_rot"] = entry(sec, 20 * raw.shape[0], "scans/s", f"host buffers in and out, page-locked like a driver's DMA buffers (H2D of {raw.nbytes >> 10} KiB + D2H of the "
                               f"three clouds included); {raw.shape[0]} points -> {n_e} edge / {n_s} surf features")
    sec = rate(lambda: ex.extract(raw), 20)
    out["extract_rot_pageable"] = entry(sec, 20 * raw.shape[0], "scans/s", "the same from / into freshly allocated pageable numpy arrays (Python allocation included)")
    d_raw = torch.from_numpy(raw).cuda()
    ex.extract_device(d_raw.data_ptr(), raw.shape[0])
    sec = rate(lambda: ex.extract_device(d_raw.data_ptr(), raw.shape[0]), 50)
    out["extract_rot_device_resident"] = entry(sec, 20 * raw.shape[0], "scans/s", "scan already in HBM, features stay in HBM (lili_extract_rot with device clouds); blocking call")
    praw.close()
    # --- Livox extractor on a Horizon-like scan (L/src/Preprocessing.cpp:219-401)
    ls = synth.make_livox_scan(3, inject_bad=False)
    lx = L.LivoxExtractor(ctx)
    rl = lx.extract(ls)
    n_le, n_ls = len(rl["edge"]), len(rl["surf"])
    pls = L.api.PinnedArray(ls.shape, np.float32)
    pls.array[...] = ls
    lx.extract(pls.array, reuse=True)
    sec = rate(lambda: lx.extract(pls.array, reuse=True), 50)
    out["extract_livox"] = entry(sec, 48 * ls.shape[0] + 48 * 24000, "scans/s", f"page-locked host buffers in and out; {ls.shape[0]} points -> {n_le} edge / {n_ls} surf features")
    pls.close()
    # --- VoxelGrid of a keyframe-sized cloud and of the 5 M-point map; map index build (K7) with the cloud resident in HBM
    kf = np.concatenate([w["scan_xyz"], np.zeros((w["scan_xyz"].shape[0], 1), np.float32)], 1)
    sec = rate(lambda: L.api.voxel_filter(ctx, kf, 0.4), 10)
    out["voxel_filter_200k"] = entry(sec, 36 * kf.shape[0], "clouds/s", "pcl::VoxelGrid(0.4) of the 200 k-point scan, host in / host out")
    # --- the reference's per-keyframe local map (f-1: buildLocalMapWithLandMark + downSampleCloud + setInputCloud, L/src/BackendFusion.cpp:1387-1528,
    #     839-840): a ring of 50 keyframes of ~20 k surf features each (local_map_width = 50), moved by their poses on push; commit = concatenate +
    #     VoxelGrid(0.4) + map index, all on the device.  One keyframe = one push + one commit.
    try:
        rng = np.random.default_rng(77)
        feats = np.ascontiguousarray(np.concatenate([w["scan_xyz"][::10], np.zeros((w["scan_xyz"][::10].shape[0], 1), np.float32)], 1))
        lm = L.api.LocalMap(ctx, L.KIND_SURF, width=50, leaf=0.4, max_sq_radius=1.0)
        for k in range(50):
            lm.push(feats, [0.8 * k, 0.1 * k, 0.0], [1.0, 0.0, 0.0, 0.0])
        n_raw, n_map = lm.commit()
        kf = [0]

        def one_keyframe():
            kf[0] += 1
            lm.push(feats, [0.8 * (50 + kf[0]), 0.1 * (50 + kf[0]), 0.0], [1.0, 0.0, 0.0, 0.0])
            lm.commit()
        sec = rate(one_keyframe, 10)
        out["localmap_commit"] = entry(sec, 36 * n_raw + 36 * n_map, "keyframes/s",
                                       f"push of a {feats.shape[0]}-point keyframe (host in) + commit of the 50-keyframe ring: {n_raw} points -> VoxelGrid(0.4) -> {n_map}-point map + index, on the device")
    except Exception as e:      # noqa: BLE001
        out["localmap_commit_error"] = repr(e)
    P = L.make_params("rot")
    m = L.ScanToMapMatcher(ctx, P)
    d_map = torch.from_numpy(np.ascontiguousarray(w["map_xyz"])).cuda()
    cloud = L.api.cloud_from_device(d_map.data_ptr(), w["map_xyz"].shape[0], 12, -1)
    focus_r = float(np.linalg.norm(w["scan_xyz"], axis=1).max()) + 3.0
    m.map_focus(w["lidar_t"], focus_r)
    sec = rate(lambda: m.set_input_cloud(L.KIND_SURF, cloud), 10)
    g0, miss0, _ = m.map_build_stats()
    out["map_index_build"] = entry(sec, 36 * w["map_xyz"].shape[0], "maps/s", f"lili_map_set on {w['map_xyz'].shape[0]} points resident in HBM (K7: cell sort, index, super-row copy within {focus_r:.0f} m of the sensor), blocking call; "
                                   "STEADY STATE of a pipeline that re-indexes an unchanged map: every timed build starts from the previous build's bounding box (no box pass, no host round trip before the kernels) "
                                   "and the guess holds — see map_index_build_measured_box for a build that measures its box, and box_guesses / box_guess_misses")
    out["map_index_build"]["box_guesses"], out["map_index_build"]["box_guess_misses"] = int(g0), int(miss0)
    ctx.set_option("map_guess_box", 0)
    sec = rate(lambda: m.set_input_cloud(L.KIND_SURF, cloud), 10)
    out["map_index_build_measured_box"] = entry(sec, 36 * w["map_xyz"].shape[0], "maps/s", "option map_guess_box = 0: every build measures its bounding box first (a first build, or a map that moved by more than the margin: "
                                                "box pass + one host round trip before the grid); a guess that MISSES costs this plus the discarded guessed build")
    ctx.set_option("map_guess_box", 1)
    # a map that jumps by more than the guess's margin (40 m along x): the guessed build is discarded and the map is measured and built again before the call returns
    d_shift = d_map.clone()
    d_shift[:, 0] += 40.0
    cloud_shift = L.api.cloud_from_device(d_shift.data_ptr(), w["map_xyz"].shape[0], 12, -1)
    m.set_input_cloud(L.KIND_SURF, cloud)
    ga, ma, _ = m.map_build_stats()
    torch.cuda.synchronize()
    tic = time.perf_counter()
    m.set_input_cloud(L.KIND_SURF, cloud_shift)
    torch.cuda.synchronize()
    sec_miss = time.perf_counter() - tic
    gb, mb, _ = m.map_build_stats()
    out["map_index_build_guess_miss"] = entry(sec_miss, 36 * w["map_xyz"].shape[0], "maps/s", f"ONE build of the same map shifted by 40 m (box_guesses +{gb - ga}, box_guess_misses +{mb - ma}): guessed build discarded, box measured, built again")
    m.set_input_cloud(L.KIND_SURF, cloud)
    del d_shift
    m.map_focus(None)
    sec = rate(lambda: m.set_input_cloud(L.KIND_SURF, cloud), 10)
    out["map_index_build_whole_map_super_rows"] = entry(sec, 36 * w["map_xyz"].shape[0] + 9 * 32 * w["map_xyz"].shape[0], "maps/s", "the same without lili_map_focus: the 9x super-row copy of all 5 M points (720 MB written)")
    ctx.set_option("super_rows", 0)
    sec = rate(lambda: m.set_input_cloud(L.KIND_SURF, cloud), 10)
    out["map_index_build_base_only"] = entry(sec, 36 * w["map_xyz"].shape[0], "maps/s", "option super_rows = 0: the cell-sorted index alone")
    ctx.set_option("super_rows", 1)
    m.map_focus(w["lidar_t"], focus_r)
    # A keyframe of a pipeline that rebuilds its local map every keyframe (L/src/BackendFusion.cpp:839-840): new index of the 5 M-point map +
    # 30 outer iterations (3 registrations of 10).  Blocking build before the iterations vs the NEXT keyframe's build started on a side stream
    # under this keyframe's iterations (lili_map_set_begin / _end).
    try:
        scan_q = np.ascontiguousarray(w["scan_xyz"])
        m.set_queries(0, L.KIND_SURF, scan_q)
        t_body, q_body = body_pose_for_lidar(L, P, w["lidar_t"])
        tp, qp = synth.perturbed_pose(t_body, q_body, np.random.default_rng(synth.SEED_POSE), 0.3, 2.0)
        m.pose_set(1, tp, qp)
        n_kf = 12

        def keyframes(pipelined):
            m.set_input_cloud(L.KIND_SURF, cloud)
            ctx.sync()
            tic = time.perf_counter()
            for k in range(n_kf):
                m.iterate_restart(0, 30, 10, 1, L.MASK_SURF)
                if pipelined:
                    m.set_input_cloud_begin(L.KIND_SURF, cloud)
                    m.set_input_cloud_end(L.KIND_SURF)
                else:
                    m.set_input_cloud(L.KIND_SURF, cloud)
            ctx.sync()
            return (time.perf_counter() - tic) / n_kf
        keyframes(True)
        s_seq, s_pipe = keyframes(False), keyframes(True)
        tq = m.pose_get(0)
        out["keyframe_pipeline"] = {"value": round(1.0 / s_pipe, 1), "unit": "keyframes/s", "ms": round(s_pipe * 1e3, 4), "blocking_build_ms": round(s_seq * 1e3, 4),
                                    "gn_status": int(tq[2]),
                                    "note": "per keyframe: index of the 5 M-point map (focused super-row copy) + 30 outer iterations of the 200 k-point scan; "
                                            "the next keyframe's build runs on a side stream under the iterations (lili_map_set_begin / _end) vs blocking lili_map_set"}
    except Exception as e:      # noqa: BLE001
        out["keyframe_pipeline_error"] = repr(e)
    # the same from HOST memory: pageable (the runtime stages it page by page) and page-locked (lili_host_alloc: straight DMA)
    hmap = np.ascontiguousarray(w["map_xyz"])
    sec = rate(lambda: m.set_input_cloud(L.KIND_SURF, hmap), 3)
    out["map_index_build_from_pageable_host"] = entry(sec, 36 * hmap.shape[0], "maps/s", f"lili_map_set incl. the H2D of {hmap.nbytes >> 20} MiB from pageable memory")
    pin = L.api.PinnedArray(hmap.shape, np.float32)
    pin.array[...] = hmap
    sec = rate(lambda: m.set_input_cloud(L.KIND_SURF, pin.array), 5)
    out["map_index_build_from_pinned_host"] = entry(sec, 36 * hmap.shape[0], "maps/s", f"lili_map_set incl. the H2D of {hmap.nbytes >> 20} MiB from page-locked memory (lili_host_alloc)")
    pin.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="strong (default, BASELINE configs[3]): the 200k queries of ONE scan are block-sharded over the ranks; "
                         "weak: every rank matches its own 200k-point shard of an (N x 200k)-point scan (with N > 1 the strong run "
                         "also reports the weak figure under extras)")
    ap.add_argument("--n-map", type=int, default=N_MAP)
    ap.add_argument("--n-az", type=int, default=N_AZ)
    ap.add_argument("--iters-per-scan", type=int, default=10,
                    help="one scan registration = this many outer GN iterations from the perturbed initial pose (BASELINE configs[1]: 10); "
                         "the pose is re-initialised on the device every this-many steps")
    ap.add_argument("--assoc-only", type=int, default=0, help="profiling aid: only this many association launches at a fixed pose, then exit")
    ap.add_argument("--assoc-after", type=int, default=0, help="with --assoc-only: run this many GN iterations first (pose then stays fixed)")
    ap.add_argument("--window", type=int, default=0, help="extra measurement (not the headline): K independent registrations of the same "
                    "scan in K slots advanced concurrently with lili_s2m_iterate_window; prints window iterations/s and exits")
    ap.add_argument("--config", type=int, default=2, choices=[0, 1, 2, 4],
                    help="BASELINE config to run: 2 (default) = the headline workload (with --gpus N: configs[3]); 0 / 1 / 4 = that config's own figure alone "
                         "(bench_configs.py; the default run also reports them under extras.configs)")
    ap.add_argument("--preheat-ms", type=float, default=60.0,
                    help="untimed device pre-heat before the W warm-up steps: registrations of the same loop until this many milliseconds have passed, so that the K timed "
                         "steps do not start on a GPU that idled at low clocks while the host generated the workload (0 = none; reported in config.device_preheat_ms)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary measurements (window of 3 slots, ROT extractor)")
    ap.add_argument("--collective", choices=["auto", "p2p", "rccl", "torch"], default="auto",
                    help="N > 1: who does the two tiny all-reduces per iteration — auto = lili_p2p, else RCCL from C, else torch.distributed")
    ap.add_argument("--no-native-rccl", action="store_true", help="same as --collective torch (A/B: the two all-reduces stay in the Python loop)")
    ap.add_argument("--split-path", action="store_true", help="use the multi-GPU code path (export/import counts, separate GN kernel) even at N=1")
    ap.add_argument("--opt", action="append", default=[], help="A/B: lili_set_option name=value (repeatable), e.g. --opt warm=0")
    ap.add_argument("--no-focus", action="store_true", help="A/B: build the super-row copy for the whole map instead of the sensor's surroundings (lili_map_focus)")
    ap.add_argument("--reach", type=int, default=0, help="map grid reach (1 = cells of the gate radius, 2 = half-size cells); 0 = library default")
    ap.add_argument("--cell-pct", type=int, default=0, help="reach-2 cell edge in %% of the gate radius (50..100); 0 = library default")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: roofline replay, CPU baseline and pose parity, headline regions, inner "
                         "iteration, extras (other configs, stages, window modes), multi-GPU self-checks.  Without it a run only sets up, warms up, "
                         "times the steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (pose, last GN step, the surf correspondences of its "
                         "association) as DIR/<name>.npy in float32 / float64")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.config != 2 or args.window or args.assoc_only or os.environ.get("LILI_PHASES")):
        ap.error("--dump-outputs covers the headline workload only (--config 2, no --window / --assoc-only / LILI_PHASES)")
    if args.no_native_rccl:
        args.collective = "torch"

    import torch
    import lili_om_amd as L
    from lili_om_amd import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    dist = None
    if world > 1 or os.environ.get("LILI_BENCH_FORCE_DIST"):    # the env switch exercises the collective path on ONE rank
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("LILI_BENCH_SHARE_GPU"):      # test aid: all ranks on GPU 0 (one-GPU box), gloo for the control plane;
            local_rank = 0                              # RCCL refuses two ranks on one device, the p2p exchange does not care
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if args.config != 2:
        # one of the other BASELINE configs on its own (single GPU): same JSON contract, the config's own metric
        import bench_configs as BC
        tstream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(tstream)
        ctx = L.Context(local_rank, stream=tstream.cuda_stream)
        fn = {0: BC.config0, 1: BC.config1, 4: BC.config4}[args.config]
        r = fn(L, ctx, torch, synth, cpu=not args.no_cpu_baseline)
        ms = r.get("ms_per_scan") or r.get("ms_per_frame") or (r.get("us_per_window_evaluation", 0.0) * 1e-3)
        line = {"metric": {0: "configs[0] scans/s (130k-pt scan: ROT extraction + 1 GN iteration vs 500k-pt map)", 1: "configs[1] frames/s (24k-pt Livox frames: extraction + scan-to-map)",
                           4: "configs[4] window evaluations/s (3 keyframes, lidar blocks)"}[args.config],
                "value": r["value"], "unit": r["unit"], "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 5), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic", "config": {"workload": r["workload"]},
                "roofline": dict(r["roofline"], achieved=round(r["algorithmic_bytes"] / (ms * 1e-3) / 1e9, 3), traffic=None, kernel="whole step (all kernels)"),
                "cpu_baseline": r.get("cpu"), "details": {k: v for k, v in r.items() if k not in ("roofline", "cpu", "workload", "value", "unit")}}
        line["parity_failures"] = BC.parity_failures(r)
        print(json.dumps(line), flush=True)
        ctx.close()
        if line["parity_failures"]:
            log("[bench] PARITY / STATUS FAILURES: " + "; ".join(line["parity_failures"]))
            sys.exit(3)
        return

    # ---------------- workload (synthetic, fixed seeds; identical on every rank) ----------------
    t_gen = time.perf_counter()
    half = (460.0, 380.0) if args.n_map >= 4_000_000 else (150.0, 150.0)
    w = synth.make_workload(n_map=args.n_map, n_az=args.n_az, half_extent=half, verbose=(rank == 0))
    P = L.make_params("rot")
    t_body, q_body = body_pose_for_lidar(L, P, w["lidar_t"])
    rng = np.random.default_rng(synth.SEED_POSE)
    t0, q0 = synth.perturbed_pose(t_body, q_body, rng, 0.3, 2.0)
    scan = ring_major(w["scan_xyz"], w["scan_ring"])
    n_scan = scan.shape[0]
    def queries_for(mode):
        if world > 1 and mode == "strong":
            from lili_om_amd import sharding
            lo, hi = sharding.shard_bounds(n_scan, world, rank)
            return np.ascontiguousarray(scan[lo:hi])
        if world > 1:
            # weak: rank r holds the r-th 200k-point shard of an (N x 200k)-point scan (same rays, independent range noise)
            d = scan / np.linalg.norm(scan, axis=1, keepdims=True)
            noise = np.random.default_rng(w["seed"] + 100 + rank).normal(0, 0.02, n_scan)
            return (scan + d * noise[:, None]).astype(np.float32) if rank > 0 else scan
        return scan

    queries = queries_for(args.scaling)
    if rank == 0:
        log(f"[bench] workload generated in {time.perf_counter() - t_gen:.1f} s; {queries.shape[0]} queries/rank, world {world}, scaling {args.scaling}")

    # ---------------- device setup (untimed): map index + queries resident in HBM ----------------
    # a non-default torch stream: the lili context, the RCCL collectives and the timing events all run on it
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    assert tstream.cuda_stream != 0
    ctx = L.Context(local_rank, stream=tstream.cuda_stream)
    if args.reach:
        ctx.set_option("grid_reach", args.reach)
    if args.cell_pct:
        ctx.set_option("cell_pct", args.cell_pct)
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    m = L.ScanToMapMatcher(ctx, P)
    # the scan reaches ~1/10 of the 920 m x 760 m map: the super-row copy is built around the sensor only (a hint: results do not depend on it)
    focus_r = float(np.linalg.norm(w["scan_xyz"], axis=1).max()) + 3.0
    if not args.no_focus:
        m.map_focus(w["lidar_t"], focus_r)
    tic = time.perf_counter()
    m.set_input_cloud(L.KIND_SURF, w["map_xyz"])
    ctx.sync()
    t_map = time.perf_counter() - tic
    m.set_queries(0, L.KIND_SURF, queries)
    gram = torch.zeros(L.api.GRAM_DOUBLES, dtype=torch.float64, device=dev)
    m.pose_set(0, t0, q0)
    m.pose_set(1, t0, q0)       # slot 1 only holds the initial guess; slot 0 is restarted from it on the device
    ips = max(1, args.iters_per_scan)

    if args.window:
        K = args.window
        for k in range(1, K):
            m.set_queries(k, L.KIND_SURF, queries)
        assert 1 <= K <= 7
        m.pose_set(7, t0, q0)          # every slot restarts its registrations from this copy of the initial guess
        def run(n):
            for _ in range(n // ips):
                for k in range(K):
                    m.pose_copy(k, 7)
                m.iterate_window(list(range(K)), ips, L.MASK_SURF)
        run(args.warmup)
        torch.cuda.synchronize()
        tic = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - tic
        n_it = (args.steps // ips) * ips
        print(json.dumps({"window_slots": K, "us_per_window_iteration": el / n_it * 1e6, "slot_iterations_per_s": K * n_it / el}), flush=True)
        ctx.close()
        return
    if os.environ.get("LILI_PHASES"):
        if os.environ["LILI_PHASES"] == "waves":
            os.environ["LILI_DEBUG"] = "512"
            m.iterate(0, 8, L.MASK_SURF)
            tp = m.debug_times(0)
            print("wave gram-done times (us after block start):", [round((x - tp[15]) * 0.01, 2) for x in tp[:13]], file=sys.stderr)
            ctx.close()
            return
        os.environ["LILI_DEBUG"] = "256"
        m.iterate(0, 8, L.MASK_SURF)
        tp = m.debug_times(0)
        names = {0: "lin start", 1: "lin counts+loads done", 2: "lin math done", 3: "lin gram done", 4: "lin partial stored",
                 8: "red start", 9: "red loads done", 10: "red record built", 11: "red gn done",
                 13: "PREVIOUS red start", 14: "PREVIOUS red record built", 5: "assoc workgroup 0 start", 6: "assoc workgroup 0 holds the pose"}
        base = tp[13] if tp[13] else tp[0]
        for k in sorted(names, key=lambda k: tp[k]):
            print(f"{names[k]:26s} {(tp[k] - base) * 0.01:8.2f} us", file=sys.stderr)
        ctx.close()
        return
    if args.assoc_only:
        m.iterate(0, args.assoc_after, L.MASK_SURF)
        torch.cuda.synchronize()
        if os.environ.get("LILI_DEBUG_AFTER"):
            os.environ["LILI_DEBUG"] = os.environ["LILI_DEBUG_AFTER"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.associate_dev(0, L.MASK_SURF)
        e0.record()
        for _ in range(args.assoc_only):
            m.associate_dev(0, L.MASK_SURF)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"assoc_only_us": e0.elapsed_time(e1) * 1e3 / args.assoc_only, "after_iters": args.assoc_after}), flush=True)
        ctx.close()
        return

    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    exit_code = 0

    def step_multi():
        # the sharded iteration: two tiny all-reduces (counts, Gram record) between the three device stages
        m.associate_dev(0, L.MASK_SURF)
        m.counts_export(0, counts.data_ptr())
        if dist is not None:
            dist.all_reduce(counts)
        m.counts_import(0, counts.data_ptr())
        m.linearize_dev(0, gram.data_ptr(), L.MASK_SURF)
        if dist is not None:
            dist.all_reduce(gram)
        m.gn_update(0, gram.data_ptr())

    # Native collectives: lili_s2m_iterate_sharded enqueues the two all-reduces from C between the kernels (no host code on the
    # critical path).  Candidates, in order: the library's own peer-to-peer exchange (lili_p2p: hipIpc-mapped mailboxes, one small
    # kernel per all-reduce, sums in rank order = rank-identical bits), then RCCL's ncclAllReduce (communicator created next to
    # torch's).  A candidate is used only if EVERY rank could set it up and one native iteration reproduces the torch.distributed
    # iteration from the same pose — otherwise the Python loop above stays.
    native, native_kind = None, "torch.distributed from the Python loop"
    p2p_round_trip = None
    if dist is not None and args.collective != "torch":
        def flag_all(ok):
            f = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(f, op=dist.ReduceOp.MIN)
            return int(f.item()) == 1

        def make_p2p():
            from lili_om_amd import p2p
            return p2p.Communicator(ctx, rank, world, dist)

        def make_rccl():
            from lili_om_amd import rccl
            return rccl.Communicator(rank, world, device=local_rank)

        cands = [("lili_p2p (hipIpc mailboxes, rank-order sums) enqueued from C", make_p2p), ("RCCL ncclAllReduce enqueued from C", make_rccl)]
        if args.collective == "rccl":
            cands = cands[1:]
        elif args.collective == "p2p":
            cands = cands[:1]
        for kind, make in cands:
            comm = None
            try:
                comm = make()
            except Exception as e:          # noqa: BLE001
                log(f"[bench] rank {rank}: {kind}: unavailable ({e!r})")
            if not flag_all(comm is not None):
                continue
            if hasattr(comm, "all_reduce"):
                # lili_p2p only: a mailbox round trip with a known pattern BEFORE anything depends on it — every rank contributes
                # rank * 1000 + i + 0.5 (exact in f64, so is the sum), one exchange on the bench's stream, and every rank must read back exactly
                # world * (i + 0.5) + 1000 * world * (world - 1) / 2 for all 72 words.  A link that does not carry the stores (or carries stale
                # ones) fails here instead of in the middle of a registration.
                rt_ok = False
                try:
                    torch.cuda.synchronize(); dist.barrier()
                    pat = torch.arange(L.api.GRAM_DOUBLES, dtype=torch.float64, device=dev) + 0.5 + 1000.0 * rank
                    comm.all_reduce(pat.data_ptr(), L.api.GRAM_DOUBLES, 8, tstream.cuda_stream)
                    torch.cuda.synchronize()
                    want = world * (torch.arange(L.api.GRAM_DOUBLES, dtype=torch.float64, device=dev) + 0.5) + 1000.0 * world * (world - 1) / 2
                    rt_ok = bool(torch.equal(pat, want)) and comm.status() == 0
                except Exception as e:          # noqa: BLE001
                    log(f"[bench] rank {rank}: {kind}: mailbox round trip failed ({e!r})")
                p2p_round_trip = flag_all(rt_ok)
                if not p2p_round_trip:
                    if rank == 0:
                        log(f"[bench] {kind}: the mailbox round trip did not return the written bits on every rank, skipped")
                    continue
            m.pose_copy(0, 1); step_multi(); torch.cuda.synchronize()
            ta, qa, _ = m.pose_get(0)
            m.pose_copy(0, 1)
            same = False
            # The validation iteration is the communicator's FIRST exchange, which has to absorb the ranks' start-up skew (lazy code-object
            # loads, first-touch of the mapped mailboxes — lili_p2p.hip): all ranks meet at a control-plane barrier with their queues
            # drained first, and the communicator keeps its default timeout (a 2 s cut here made a spurious, sticky and
            # contagious timeout drop the native candidate for good).
            try:        # an exchange that does not work on this box (a record that never becomes visible over the link: the communicator times out and
                        # fails, lili_s2m_iterate_sharded returns LILI_E_STATE) must cost this candidate, not the run
                torch.cuda.synchronize()
                dist.barrier()
                m.iterate_sharded(0, 1, counts.data_ptr(), gram.data_ptr(), comm.allreduce_fn, comm.handle)
                torch.cuda.synchronize()
                tb, qb, _ = m.pose_get(0)
                same = bool(np.abs(ta - tb).max() <= 1e-12 and np.abs(qa - qb).max() <= 1e-12)
            except Exception as e:          # noqa: BLE001
                log(f"[bench] rank {rank}: {kind}: validation iteration failed ({e!r})")
            if flag_all(same):
                native, native_kind = comm, kind
                break
            if rank == 0:
                log(f"[bench] {kind}: did not reproduce the torch.distributed iteration, skipped")
    if rank == 0 and dist is not None:
        log(f"[bench] collectives: {native_kind}")

    def run_steps(k):
        # every `ips` steps a new registration starts from the initial guess (async device-to-device pose copy)
        if world == 1 and not args.split_path and dist is None:
            m.iterate_restart(0, k, ips, 1, L.MASK_SURF)   # one C call enqueues k x (associate, linearise, reduce+GN update)
        elif native is not None:
            m.iterate_sharded(0, k, counts.data_ptr(), gram.data_ptr(), native.allreduce_fn, native.handle, restart_every=ips, restart_slot=1)
        else:
            for i in range(k):
                if i % ips == 0:
                    m.pose_copy(0, 1)
                step_multi()

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n_warm, n_steps):
        run_steps(n_warm)
        fence()
        # every timed run starts a fresh registration at step 0, so N=1,2,4,8 do identical work per step
        fence()
        tic = time.perf_counter()
        run_steps(n_steps)
        t_enq = time.perf_counter() - tic
        fence()
        el = time.perf_counter() - tic
        if dist is not None:
            tmax = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el = float(tmax.item())
        return el, t_enq

    # Device pre-heat (round 5): the host has just spent seconds generating the workload while the GPU idled; the K-step region of the driver's command (20 steps =
    # 0.7 ms) would otherwise be measured on clocks that are still ramping (the 200-step regions of extras.headline_regions run 10 % faster on the same code).
    # Whole registrations of the SAME loop, untimed, then the contract's W warm-up steps and the K timed steps as before.
    preheat_steps = 0
    if args.preheat_ms > 0:
        # a FIXED number of steps (every rank must enqueue the same collectives): the milliseconds asked for at ~30 us per step, in whole blocks of 10 registrations
        blk = 10 * ips
        preheat_steps = max(1, int(math.ceil(args.preheat_ms * 1e3 / 30.0 / blk))) * blk
        for _ in range(preheat_steps // blk):
            run_steps(blk)
        fence()
    elapsed, t_enqueue = timed(args.warmup, args.steps)
    if rank == 0:
        log(f"[bench] host enqueue {t_enqueue / args.steps * 1e6:.1f} us/step, wall {elapsed / args.steps * 1e6:.1f} us/step")
    t_fin, q_fin, gn_status = m.pose_get(0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, m, queries.shape[0])
    # Pose-parity registration: ONE registration of `ips` outer iterations from the EXPLICIT start pose (t0, q0) — written
    # into slot 0 here, never read from a slot a later helper could have touched — taken right after the timed region, before any secondary
    # measurement runs.  Compared with the oracle's registration from the same start once cpu_baseline() has produced it.
    reg_pose = None
    if world == 1 and dist is None and args.full:
        m.pose_set(0, t0, q0)
        m.iterate(0, ips, L.MASK_SURF)
        t_reg, q_reg, st_reg = m.pose_get(0)
        reg_pose = (np.asarray(t_reg, np.float64).copy(), np.asarray(q_reg, np.float64).copy(), int(st_reg))
        m.pose_set(1, t0, q0)
    # Run-to-run spread of the headline (a 20-step region is two registrations): five more regions of >= 200 steps each, same
    # schedule; `value` stays the K-step region the contract asks for, the regions go to extras.headline_regions.
    regions = None
    if args.full and world == 1 and dist is None and not args.no_extras:
        n_reg = max(200, args.steps)
        regs = sorted(n_reg / timed(0, n_reg)[0] for _ in range(5))
        regions = {"steps_per_region": n_reg, "iterations_per_s": [round(r, 1) for r in regs], "median": round(regs[2], 1),
                   "spread_pct": round(100.0 * (regs[-1] - regs[0]) / regs[2], 2)}
        m.pose_set(1, t0, q0)
        m.pose_copy(0, 1)
        m.iterate_restart(0, args.warmup + args.steps, ips, 1, L.MASK_SURF)      # leave slot 0 where the K-step region left it (final_pose below)
        t_fin, q_fin, gn_status = m.pose_get(0)

    # ---------------- roofline of the dominant kernel (k_associate_surf), HIP events on its stream ----------------
    roofline = None
    if args.full and rank == 0:
        # The poses the association kernel sees over the timed schedule (restart every `ips` steps) are logged first;
        # then exactly those launches are replayed back to back on the context's stream between ONE pair of HIP events,
        # so the per-launch figure carries no inter-kernel event overhead and is comparable with rocprofv3's average.
        reps = max(2 * ips, min(args.steps, 200))
        poses = []
        for it in range(reps):
            if it % ips == 0:
                m.pose_copy(0, 1)
            tl, ql, _ = m.pose_get(0)
            poses.append(L.api.assoc_transform(tl, ql, P))
            m.iterate(0, 1, L.MASK_SURF)
        for Q2, T2 in poses[:5]:
            m.find_corresponding_surf_features(0, Q2, T2, want_count=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for Q2, T2 in poses:
            m.find_corresponding_surf_features(0, Q2, T2, want_count=False)
        e1.record()
        torch.cuda.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3 / reps
        alg_bytes = BYTES_PER_QUERY * queries.shape[0]
        achieved = alg_bytes / dt / 1e9
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc):
            try:
                traffic = json.load(open(pmc)).get("k_associate_surf", {}).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        roofline = dict(bound="hbm", kernel="k_associate_surf", achieved=round(achieved, 3), peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=round(achieved / HBM_PEAK_GBS, 6), traffic=traffic, us_per_launch=round(dt * 1e6, 2),
                        algorithmic_bytes_per_launch=alg_bytes,
                        traffic_source=("profiles/pmc_traffic.json: rocprofv3 --pmc passes of this command collected by tools/make_profiles.sh (2 x FETCH_SIZE + WRITE_SIZE per the "
                                        "guide's gfx950 correction) and committed — NOT measured inside this run") if traffic is not None else None)
    if dist is not None:
        dist.barrier()

    # ---------------- secondary timed figures that need every rank (collective paths) ----------------
    weak_extra = None
    if args.full and world > 1 and args.scaling == "strong":
        # the flattering variant, kept out of `value`: every rank matches its OWN 200k-point shard of an (N x 200k)-point scan
        qw = queries_for("weak")
        m.set_queries(0, L.KIND_SURF, qw)
        el_w, _ = timed(args.warmup, args.steps)
        weak_extra = {"weak_scaling_iterations_per_s": round(args.steps * world / el_w, 3), "weak_scaling_ms_per_step": round(el_w / args.steps * 1e3, 5),
                      "weak_scaling_note": f"{world} x {qw.shape[0]}-point shards of an (N x 200k)-point scan, value = steps x N / time"}
        m.set_queries(0, L.KIND_SURF, queries)

    # Replica mode (what scales for a 35 us iteration is independent work): EVERY rank registers the whole 200 k-point scan
    # against its replica of the map with the single-GPU loop — no collective anywhere in the timed region — value = steps x N / max-over-ranks time.
    # Self-check: the ranks run the same deterministic code on the same data, so their final poses must be identical bit for bit (and equal to
    # the N = 1 run's final_pose for the same --steps / --warmup).
    replica_extra, replica_pose = None, None
    if args.full and world > 1:
        m.set_queries(0, L.KIND_SURF, scan)
        m.pose_set(1, t0, q0)

        def run_replica(k):
            m.iterate_restart(0, k, ips, 1, L.MASK_SURF)
        run_replica(args.warmup)
        fence(); fence()
        tic = time.perf_counter()
        run_replica(args.steps)
        fence()
        el_r = time.perf_counter() - tic
        tmax = torch.tensor([el_r], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        el_r = float(tmax.item())
        tr, qr, str_ = m.pose_get(0)
        rb = torch.from_numpy(np.concatenate([np.asarray(tr, np.float64), np.asarray(qr, np.float64)]).view(np.int64).copy()).to(dev)
        lo_r, hi_r = rb.clone(), rb.clone()
        dist.all_reduce(lo_r, op=dist.ReduceOp.MIN); dist.all_reduce(hi_r, op=dist.ReduceOp.MAX)
        st_r = torch.tensor([int(str_)], dtype=torch.int32, device=dev)
        dist.all_reduce(st_r, op=dist.ReduceOp.MAX)
        replica_extra = {"replicas_iterations_per_s": round(args.steps * world / el_r, 3), "replicas_ms_per_step": round(el_r / args.steps * 1e3, 5),
                         "replicas_note": f"{world} ranks x the whole {n_scan}-pt scan each (one scan per GPU, map replicated), single-GPU loop, NO collective in the timed region; "
                                          "value = steps x N / max-over-ranks time",
                         "replicas_final_pose_bit_identical_on_all_ranks": bool(torch.equal(lo_r, hi_r)), "replicas_max_gn_status": int(st_r.item()),
                         "replicas_final_pose": {"t": [float(x) for x in tr], "q": [float(x) for x in qr]}}
        m.set_queries(0, L.KIND_SURF, queries)

    # Slot-per-rank window (round 5; configs[4]'s split that scales): N keyframes = N registrations of the whole 200 k-point scan, keyframe i at FULL size on
    # rank i, every iteration ONE exchange of the N x 72 doubles (an all-gather carried by the rank-order sum) and the Gauss-Newton update of every slot on every rank.
    # value = N slot-iterations per window iteration / max-over-ranks time.  Self-check: all ranks hold bit-identical poses for all slots.
    gather_extra = None
    if args.full and world > 1 and world <= 8 and native is not None:
        try:
            from lili_om_amd import sharding
            owner = sharding.window_owners(world, world)
            slots_g = list(range(world))
            m.set_queries(rank, L.KIND_SURF, scan)                      # this rank's keyframe: the whole scan, no shard
            wgram = torch.zeros(world * L.api.GRAM_DOUBLES, dtype=torch.float64, device=dev)
            starts = [synth.perturbed_pose(t_body, q_body, np.random.default_rng(synth.SEED_POSE + 17 * k), 0.3, 2.0) for k in range(world)]

            def reset_slots():
                for k in range(world):
                    m.pose_set(k, starts[k][0], starts[k][1])
            reset_slots()
            m.iterate_window_gather(slots_g, args.warmup, owner, rank, wgram.data_ptr(), native.allreduce_fn, native.handle, kind_mask=L.MASK_SURF)
            reset_slots()
            fence(); fence()
            tic = time.perf_counter()
            m.iterate_window_gather(slots_g, ips, owner, rank, wgram.data_ptr(), native.allreduce_fn, native.handle, kind_mask=L.MASK_SURF)
            fence()
            el_g = time.perf_counter() - tic
            tmax = torch.tensor([el_g], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el_g = float(tmax.item())
            fin_g = [m.pose_get(k) for k in range(world)]
            gb = torch.from_numpy(np.concatenate([np.r_[np.asarray(t, np.float64), np.asarray(q, np.float64)] for t, q, _ in fin_g]).view(np.int64).copy()).to(dev)
            lo_g, hi_g = gb.clone(), gb.clone()
            dist.all_reduce(lo_g, op=dist.ReduceOp.MIN); dist.all_reduce(hi_g, op=dist.ReduceOp.MAX)
            st_g = torch.tensor([max(int(st) for _, _, st in fin_g)], dtype=torch.int32, device=dev)
            dist.all_reduce(st_g, op=dist.ReduceOp.MAX)
            gather_extra = {"window_gather_slot_iterations_per_s": round(world * ips / el_g, 3), "window_gather_us_per_window_iteration": round(el_g / ips * 1e6, 2),
                            "window_gather_poses_bit_identical_on_all_ranks": bool(torch.equal(lo_g, hi_g)), "window_gather_max_gn_status": int(st_g.item()),
                            "window_gather_dt_truth_m": float(max(np.abs(np.asarray(t) - t_body).max() for t, _, _ in fin_g)),
                            "window_gather_note": f"slot-per-rank window (lili_s2m_iterate_window_gather): {world} keyframes = {world} registrations of the whole {n_scan}-pt scan from {world} start poses, keyframe i at full "
                                                  f"size on rank i; per iteration every rank associates + linearises ITS keyframe, ONE exchange of {world} x 72 doubles, GN update of every slot on every rank; "
                                                  f"one registration of {ips} iterations timed; value = {world} x iterations / max-over-ranks time"}
            m.set_queries(0, L.KIND_SURF, queries)
        except Exception as e:      # noqa: BLE001
            gather_extra = {"window_gather_error": repr(e)}

    # Multi-GPU self-check: every rank must hold the SAME final pose, bit for bit (strong split: one scan, all ranks apply the same
    # update to the same reduced record).  all-reduce MIN and MAX of the pose bit patterns: equal <=> identical on every rank.
    multi = None
    if args.full and dist is not None and args.scaling == "strong":
        bits = torch.from_numpy(np.concatenate([np.asarray(t_fin, np.float64), np.asarray(q_fin, np.float64)]).view(np.int64).copy()).to(dev)
        lo, hi = bits.clone(), bits.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        st_all = torch.tensor([int(gn_status)], dtype=torch.int32, device=dev)
        dist.all_reduce(st_all, op=dist.ReduceOp.MAX)
        multi = {"ranks": world, "rccl_ranks": world if dist.get_backend() == "nccl" else 0, "backend": dist.get_backend(),
                 "final_pose_bit_identical_on_all_ranks": bool(torch.equal(lo, hi)), "max_gn_status": int(st_all.item()),
                 "p2p_mailbox_round_trip": p2p_round_trip}
        if replica_extra:
            multi["replicas_final_pose_bit_identical_on_all_ranks"] = replica_extra["replicas_final_pose_bit_identical_on_all_ranks"]
            multi["replicas_max_gn_status"] = replica_extra["replicas_max_gn_status"]
    if rank == 0:
        units = args.steps * (world if args.scaling == "weak" else 1)
        value = units / elapsed
        out = {
            "metric": "scan-to-map iterations/s (200k-pt scan vs 5M-pt map)",
            "value": round(value, 3), "unit": "iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 5), "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"configs[{2 if world == 1 else 3}]: synthetic 64-ring {n_scan}-pt scan vs {w['map_xyz'].shape[0]}-pt local map "
                                   f"(variant A, seed {hex(w['seed'])}), ROT back-end matcher (surf), 1 outer GN iteration per step, a new registration from the perturbed pose every {ips} steps, "
                                   f"{'the 200k queries of the scan block-sharded over the ranks' if args.scaling == 'strong' else 'one 200k-pt shard per rank'}",
                       "queries_per_rank": int(queries.shape[0]), "map_points": int(w["map_xyz"].shape[0]),
                       "parallelism": f"queries sharded x{world}, map replicated, all-reduce(counts, Gram)" if world > 1 else "single GPU",
                       "collectives": native_kind if dist is not None else "none",
                       "map_index_build_s": round(t_map, 4),
                       "device_preheat_ms": args.preheat_ms, "device_preheat_steps": preheat_steps,
                       "map_focus_m": None if args.no_focus else round(focus_r, 1)},
            "roofline": (dict(roofline, whole_step_frac=round(roofline["algorithmic_bytes_per_launch"] / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 6),
                              whole_step_note="algorithmic bytes of one outer iteration's association / ms_per_step: the fraction of the HBM peak the WHOLE step (association + linearise + "
                                              "reduce + three kernel boundaries) reaches on the same byte count; `frac` is the dominant kernel alone")
                         if roofline and world == 1 else roofline),
            "final_pose": {"t": [float(x) for x in t_fin], "q": [float(x) for x in q_fin], "gn_status": int(gn_status)},
        }
        failures = []       # parity / solver-status violations: the JSON line is still printed, then the run exits with status 3
        if int(gn_status) != 0:
            failures.append(f"headline gn_status {int(gn_status)}")
        if multi:
            out["multi_gpu_check"] = multi
            if not multi["final_pose_bit_identical_on_all_ranks"] or multi["max_gn_status"] != 0 or multi.get("replicas_final_pose_bit_identical_on_all_ranks") is False \
                    or multi.get("replicas_max_gn_status", 0) != 0:
                failures.append(f"multi_gpu_check {multi}")
        extras = dict(weak_extra or {})
        extras.update(replica_extra or {})
        extras.update(gather_extra or {})
        if args.full and world > 1:      # which mode a SCALE record's `value` has to be read against
            extras["scaling_modes_note"] = ("`value` is the " + ("STRONG split of ONE 200k-pt scan over the ranks (configs[3]): per-rank work shrinks with N while three dependent "
                                            "kernel chains per iteration do not, so ~1.1-1.2x at 8 GPUs is the expected ceiling (DESIGN §5)" if args.scaling == "strong" else
                                            "weak split (one 200k-pt shard per rank)") + "; the modes that scale by construction are printed beside it: replicas_iterations_per_s "
                                            "(one whole scan per GPU, no collective) and window_gather_slot_iterations_per_s (one full-size keyframe of the sliding window per GPU, one "
                                            "exchange per iteration)")
        if gather_extra and "window_gather_error" not in gather_extra and (not gather_extra["window_gather_poses_bit_identical_on_all_ranks"] or gather_extra["window_gather_max_gn_status"] != 0):
            failures.append(f"window_gather {gather_extra}")
        if regions:
            extras["headline_regions"] = regions
        if args.full and world == 1 and dist is None:
            # ---- the reference back-end's INNER iteration ("report it separately, never mix the two"): fixed correspondences,
            # linearise (residual + Jacobian + Cauchy corrector + cost) + reduce + 6x6 solve + pose update = ONE launch each
            try:
                m.pose_copy(0, 1)
                m.iterate(0, ips, L.MASK_SURF)              # converge, then associate once at that pose
                m.associate_dev(0, L.MASK_SURF)
                m.iterate_inner(0, 20, L.MASK_SURF, want_cost=True)
                n_in = 400
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                m.iterate_inner(0, n_in, L.MASK_SURF, want_cost=True)
                e1.record()
                torch.cuda.synchronize()
                us_in = e0.elapsed_time(e1) * 1e3 / n_in
                _, _, st_in = m.pose_get(0)
                if int(st_in) != 0:
                    failures.append(f"inner_iteration gn_status {int(st_in)}")
                out["inner_iteration"] = {"value": round(1e6 / us_in, 1), "unit": "inner iterations/s", "us_per_iteration": round(us_in, 3), "gn_status": int(st_in),
                                          "definition": "fixed correspondences (200k surf records of one association): linearise incl. robust cost + reduce + 6x6 solve + pose "
                                                        "update, one launch per iteration (lili_s2m_iterate_inner); the loop ceres::Solve runs up to 15x per keyframe, "
                                                        "L/src/BackendFusion.cpp:984-992",
                                          "algorithmic_bytes": 41 * int(queries.shape[0]),
                                          "hbm_frac": round(41 * queries.shape[0] / (us_in * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)}
            except Exception as e:      # noqa: BLE001
                out["inner_iteration"] = {"error": repr(e)}
        if args.full and world == 1 and dist is None and not args.no_extras:
            # Secondary measurements (NOT the headline).  Every block runs in ITS OWN lili context (pose slots, options, map focus and map
            # indices are per context): nothing here can touch the headline context `ctx` / matcher `m` (VERDICT r3 #1 — the shared
            # context let three helpers overwrite pose slot 1, which the parity check then started from).
            def own_ctx():
                return L.Context(local_rank, stream=tstream.cuda_stream)

            def headline_matcher(c, params=P):
                mm = L.ScanToMapMatcher(c, params)
                if not args.no_focus:
                    mm.map_focus(w["lidar_t"], focus_r)
                mm.set_input_cloud(L.KIND_SURF, w["map_xyz"])
                return mm
            cx = None
            try:
                # the 3-keyframe window of configs[4] advanced concurrently (lili_s2m_iterate_window)
                cx = own_ctx()
                mw = headline_matcher(cx)
                K = 3
                for k in range(K):
                    mw.set_queries(k, L.KIND_SURF, queries)
                mw.pose_set(7, t0, q0)

                def run_window(n):
                    for _ in range(n // ips):
                        for k in range(K):
                            mw.pose_copy(k, 7)
                        mw.iterate_window(list(range(K)), ips, L.MASK_SURF)
                run_window(ips)
                torch.cuda.synchronize()
                tw = time.perf_counter()
                run_window(10 * ips)
                torch.cuda.synchronize()
                el = time.perf_counter() - tw
                extras["window3_slot_iterations_per_s"] = round(K * 10 * ips / el, 1)
                extras["window3_us_per_window_iteration"] = round(el / (10 * ips) * 1e6, 2)
            except Exception as e:      # noqa: BLE001  (secondary numbers must never cost the headline line)
                extras["window_error"] = repr(e)
            finally:
                if cx is not None:
                    cx.close(); cx = None
            try:
                # The same scan and map through the FRONT-END flavour (plain point-to-plane, no count scaling, L/src/LidarOdometry.cpp:352-413):
                # flavours whose weights do not depend on the scan's correspondence count linearise inside the association launch
                # (k_associate_lin: 2 launches per iteration); A/B against the three-launch path (option fuse_lin = 0).
                cx = own_ctx()
                Pf = L.make_params("frontend")
                mf = headline_matcher(cx, Pf)
                q_small = np.ascontiguousarray(queries[::10])          # 20 k queries: the size of a Livox scan's feature cloud
                mf.set_queries(0, L.KIND_SURF, q_small)
                tl = np.asarray(w["lidar_t"], np.float64)
                ql = np.array([1.0, 0.0, 0.0, 0.0])
                tp, qp = synth.perturbed_pose(tl, ql, np.random.default_rng(synth.SEED_POSE), 0.3, 2.0)
                mf.pose_set(1, tp, qp)
                fr = {}
                for fuse in (1, 0):
                    cx.set_option("fuse_lin", fuse)
                    mf.iterate_restart(0, 2 * ips, ips, 1, L.MASK_SURF)
                    torch.cuda.synchronize()
                    tw = time.perf_counter()
                    mf.iterate_restart(0, 20 * ips, ips, 1, L.MASK_SURF)
                    torch.cuda.synchronize()
                    el = time.perf_counter() - tw
                    tf_, qf_, stf = mf.pose_get(0)
                    fr[fuse] = (20 * ips / el, el / (20 * ips) * 1e6, float(np.linalg.norm(tf_ - tl)), int(stf))
                extras["frontend_flavour"] = {"value": round(fr[1][0], 1), "unit": "iterations/s", "us_per_iteration": round(fr[1][1], 2),
                                              "three_launch_path_us_per_iteration": round(fr[0][1], 2), "dt_truth_m": round(fr[1][2], 6), "gn_status": fr[1][3],
                                              "queries": int(q_small.shape[0]),
                                              "note": "front-end matcher flavour, every 10th point of the scan (a Livox scan's size) vs the 5 M-point map: association + linearisation in ONE launch, then reduce + GN (scans above ~100 k queries keep three launches)"}
                if fr[1][3] != 0:
                    failures.append(f"frontend_flavour gn_status {fr[1][3]}")
            except Exception as e:      # noqa: BLE001
                extras["frontend_flavour_error"] = repr(e)
            finally:
                if cx is not None:
                    cx.close(); cx = None
            try:
                cx = own_ctx()
                extras.update(secondary_stages(L, cx, w, torch))
            except Exception as e:      # noqa: BLE001
                extras["stages_error"] = repr(e)
            finally:
                if cx is not None:
                    cx.close(); cx = None
            # one timed figure per BASELINE config, the blocking seam calls, the small launch sizes (bench_configs.py)
            import bench_configs as BC
            try:
                cx = own_ctx()
                mb = headline_matcher(cx)
                mb.set_queries(0, L.KIND_SURF, queries)
                extras["blocking_seam"] = BC.blocking_seam(L, cx, torch, mb, P, queries, t_body, q_body)
            except Exception as e:      # noqa: BLE001
                extras["blocking_seam_error"] = repr(e)
            finally:
                if cx is not None:
                    cx.close(); cx = None
            try:
                cx = own_ctx()
                extras["small_launches"] = BC.small_launches(L, cx, torch, synth, w, scan, focus_r)
                for row in extras["small_launches"]:
                    if row.get("gn_status", 0) != 0:
                        failures.append(f"small_launches {row['flavour']} {row['queries']}: gn_status {row['gn_status']}")
            except Exception as e:      # noqa: BLE001
                extras["small_launches_error"] = repr(e)
            finally:
                if cx is not None:
                    cx.close(); cx = None
            try:
                cx = own_ctx()
                extras["scan_pipeline_200k"] = BC.scan_pipeline_200k(L, cx, torch, synth, w, focus_r, cpu=not args.no_cpu_baseline, ips=ips)
                failures.extend(f"scan_pipeline_200k: {f}" for f in BC.parity_failures(extras["scan_pipeline_200k"]))
                if (extras["scan_pipeline_200k"].get("one_call") or {}).get("pose_equals_separate_calls_bit_for_bit") is False:
                    failures.append("scan_pipeline_200k: the one-call pose differs from the separate calls")
            except Exception as e:      # noqa: BLE001
                extras["scan_pipeline_200k"] = {"error": repr(e)}
            try:
                extras["scan_pipeline_200k_concurrent"] = BC.scan_pipeline_200k_concurrent(L, torch, synth, w, focus_r, device=local_rank, ips=ips)
                if extras["scan_pipeline_200k_concurrent"].get("gn_status", 0) != 0:
                    failures.append("scan_pipeline_200k_concurrent: poses differ between the contexts / gn_status")
            except Exception as e:      # noqa: BLE001
                extras["scan_pipeline_200k_concurrent"] = {"error": repr(e)}
            try:
                extras["keyframe_real_size"] = BC.keyframe_real_size(L, cpu=not args.no_cpu_baseline)
                if extras["keyframe_real_size"].get("parity", {}).get("pass") is False:
                    failures.append("keyframe_real_size: the one-call keyframe differs from the separate calls")
            except Exception as e:      # noqa: BLE001
                extras["keyframe_real_size"] = {"error": repr(e)}
            finally:
                if cx is not None:
                    cx.close(); cx = None
            cfgs = {}
            for key, fn in (("0", BC.config0), ("1", BC.config1), ("2B", BC.config2b), ("4", BC.config4)):
                try:
                    cx = own_ctx()
                    cfgs[key] = fn(L, cx, torch, synth, cpu=not args.no_cpu_baseline)
                    failures.extend(f"configs[{key}]: {f}" for f in BC.parity_failures(cfgs[key]))
                    if isinstance(cfgs[key].get("cpp_loop"), dict) and cfgs[key]["cpp_loop"].get("poses_equal_bit_for_bit") is False:
                        failures.append(f"configs[{key}]: the C++ program's one-call pose differs from its separate calls")
                except Exception as e:      # noqa: BLE001
                    cfgs[key] = {"error": repr(e)}
                finally:
                    if cx is not None:
                        cx.close(); cx = None
            extras["configs"] = cfgs
        if extras:
            out["extras"] = extras
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb, t_cpu, q_cpu = cpu_baseline(w, queries, t0, q0)
            out["cpu_baseline"] = cb
            out["gpu_over_cpu"] = round(value / cb["value"], 1)
            # pose parity at the bench workload (north star: 1e-4 m / 1e-4 rad): the registration taken right after the timed region
            # (reg_pose: `ips` outer iterations from the explicit start t0, q0) against the oracle's registration from the same start.
            if reg_pose is not None:
                t_g, q_g, st_g = reg_pose
                dqv = synth.quat_mul(np.asarray(q_g) * np.array([1, -1, -1, -1]), np.asarray(q_cpu))
                pd = {"dt_m": float(np.abs(np.asarray(t_g) - np.asarray(t_cpu)).max()),
                      "dang_rad": float(2 * np.arcsin(min(1.0, np.linalg.norm(dqv[1:])))),
                      "iterations": ips, "tolerance": "1e-4 m / 1e-4 rad (north star)", "gn_status": st_g,
                      "dt_truth_m": float(np.abs(np.asarray(t_g) - t_body).max()),
                      "start": "explicit (t0, q0) written into slot 0 right after the timed region; oracle from the same (t0, q0)"}
                if (args.warmup + args.steps) % ips == 0 and regions is None:
                    pd["timed_region_final_pose_is_this_registration"] = bool(np.array_equal(np.asarray(t_fin), t_g) and np.array_equal(np.asarray(q_fin), q_g))
                pd["pass"] = bool(pd["dt_m"] <= POSE_TOL_M and pd["dang_rad"] <= POSE_TOL_RAD and st_g == 0)
                out["pose_delta_vs_cpu"] = pd
                if not pd["pass"]:
                    failures.append(f"pose_delta_vs_cpu {pd['dt_m']:.3e} m / {pd['dang_rad']:.3e} rad, gn_status {st_g}")
        else:
            out["cpu_baseline"] = None
        try:        # RCCL prints its version banner through C stdio, which is flushed at exit: push it out BEFORE the JSON line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:   # noqa: BLE001
            pass
        out["parity_failures"] = failures
        print(json.dumps(out), flush=True)
        exit_code = 3 if failures else 0
        if failures:
            log("[bench] PARITY / STATUS FAILURES: " + "; ".join(failures))
    if dist is not None:
        try:
            torch.cuda.synchronize()
            if native is not None:
                native.close()
        except Exception:   # noqa: BLE001
            pass
        dist.destroy_process_group()
    ctx.close()
    if exit_code:
        sys.exit(exit_code)


if __name__ == "__main__":
    main()
