"""One sha256 per raw output buffer of the device solvers and the extractors, on fixed inputs: two builds of the library that print the same lines compute the
same bits.  Meant for changes that claim to leave every result bit for bit alone (LILI_HIP_LIBRARY selects the build, as for the other A/B tools).

    python tools/solver_bits.py [out.json]

Cases (inputs from the generators the tests use; each a fraction of a second of GPU time, every solve runs once):
  lm        lili_s2m_solve_lm, Livox and ROT (count-scaled) flavour, ~1 500 records (one-hop exchange) and ~10 000 (20 workgroups: two hops); three slots in one
            launch (lili_s2m_solve_lm_window)
  coop      persistent cooperative iterations (k_iterate_coop), ROT and front-end flavour, 300 surf + 40 edge queries at 16 lanes per query (22 workgroups: two
            hops, counts and Gram) and at 2 lanes per query (one hop)
  window    lili_window_solve with IMU factors, speed-bias priors and a marginalisation prior on keyframe 0, n_kf = 2 and 4
  gn        launch-by-launch Gauss-Newton, one-lane tail (gn_update) and six-lane tail (iterate), three iterations each from a start 0.4 deg and 35 deg off
            on the whole scan (steps of 0.003 .. 0.09 rad: the small-angle branch of the quaternion update) and on slices of 12 .. 96 queries (no valid row:
            the rejected step, status 1).  No scan makes a step turn past 0.5 rad, so the large-angle branch runs on hand-built records whose steps turn by
            0.9 rad (and 0.3 rad): on the one-lane tail through gn_update, on the six-lane tail through the sharded window iteration with an all-reduce
            callback that puts the records in place (k_window_gn).  The same call without a callback: two slots, three iterations (k_window_reduce)
  extract   ROT and Livox extractor on one small scan each, q_imu well away from identity (the acos branch of the slerp) and identity (the linear branch)
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lili_om_amd as L  # noqa: E402
from lili_om_amd import synth  # noqa: E402
from tests import test_window_solve_gpu as TW  # noqa: E402

MASK = L.MASK_SURF | L.MASK_EDGE
OUT = {}


def put(name, *bufs):
    h = hashlib.sha256()
    for b in bufs:
        h.update(b if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b).tobytes())
    OUT[name] = h.hexdigest()
    print(f"{name:58s} {OUT[name]}", flush=True)


def slot_state(m, slot):
    """pose, last_delta, gn_status, iters as the host reads them"""
    t, q, st = m.pose_get(slot)
    d, n, st2 = m.last_step(slot)
    return [t, q, d, np.array([st, st2, n], np.int64)]


def room_matcher(ctx, flavour, seed, n_surf, n_edge, slots=(0,)):
    room = synth.make_room(seed=seed, n_query=n_surf, n_edge_query=n_edge)
    P = L.make_params(flavour)
    rng = np.random.default_rng(seed + 7)
    refl = lambda n: rng.uniform(0.0, 0.05, (n, 1)).astype(np.float32)
    smap, sq = room["map_xyz"], room["q_xyz"]
    if flavour == "livox":
        smap, sq = np.c_[smap, refl(smap.shape[0])], np.c_[sq, refl(sq.shape[0])]
    m = L.ScanToMapMatcher(ctx, P)
    m.set_input_cloud(L.KIND_SURF, smap)
    m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
    for s in slots:
        m.set_queries(s, L.KIND_SURF, sq)
        m.set_queries(s, L.KIND_EDGE, room["eq_xyz"])
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    return m, tb, qb


def case_lm(ctx):
    for flavour in ("livox", "rot"):
        for n_surf, n_edge in ((1300, 200), (9500, 500)):
            m, tb, qb = room_matcher(ctx, flavour, 61, n_surf, n_edge)
            t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(64), 0.06, 0.6)
            m.pose_set(0, t0, q0)
            m.associate_dev(0, MASK)
            s = L.api.LmSummary()
            info = m.solve_lm(0, MASK, summary=s)
            tag = f"lm/{flavour}/{n_surf}+{n_edge}"
            print(f"# {tag}: {info['iterations']} iterations, {info['successful_steps']} successful, {info['termination']}, n = {info['n_surf']} + {info['n_edge']}")
            put(tag + "/state", *slot_state(m, 0))
            put(tag + "/summary", bytes(s))
    m, tb, qb = room_matcher(ctx, "livox", 73, 2500, 200, slots=(0, 1, 2))
    for k in range(3):
        m.pose_set(k, *synth.perturbed_pose(tb, qb, np.random.default_rng(100 + k), 0.05, 0.5))
        m.associate_dev(k, MASK)
    s = (L.api.LmSummary * 3)()
    m.solve_lm_window([0, 1, 2], MASK, summary=s)
    put("lm/livox/window of 3/state", *[b for k in range(3) for b in slot_state(m, k)])
    put("lm/livox/window of 3/summary", bytes(s))


def case_coop(ctx):
    try:
        for flavour in ("rot", "frontend"):
            for lanes in (16, 2):
                ctx.set_option("persistent_iterate", 1)
                ctx.set_option("assoc_lpq", lanes)
                m, tb, qb = room_matcher(ctx, flavour, 59, 300, 40)
                m.pose_set(0, *synth.perturbed_pose(tb, qb, np.random.default_rng(31), 0.15, 1.2))
                m.iterate(0, 7, MASK)
                st = slot_state(m, 0)
                print(f"# coop/{flavour}/{lanes} lanes: status {int(st[3][0])}, {int(st[3][2])} updates")
                put(f"coop/{flavour}/{lanes} lanes per query/state", *st)
    finally:
        ctx.set_option("persistent_iterate", 0)
        ctx.set_option("assoc_lpq", 0)


def case_window(ctx):
    win4 = TW.make_window_n(4)
    for n_kf in (2, 4):
        win = TW.cut(win4, 0, n_kf)
        m = TW.gpu_side(ctx, win)
        # a marginalisation prior on keyframe 0 (blocks t, q, speed-bias: 15 local columns), linearised at the initial state: a fixed well-conditioned J0, small r0
        i, j = np.meshgrid(np.arange(15), np.arange(15), indexing="ij")
        J0 = np.where(i == j, 8.0 + 0.5 * i, 0.25 / (1.0 + np.abs(i - j)))
        s0 = win["init"][0]
        prior = dict(block_kind=[0, 1, 2], block_keyframe=[0, 0, 0], x0=[s0["t"], s0["q"], s0["sb"]], J0=J0, r0=0.01 * np.cos(np.arange(15.0)))
        ws = TW.window_problem(L.WindowSolver(ctx, m), win, n_kf, prior=prior)
        s = L.api.LmSummary()
        final, info = ws.solve(TW.state_of(win, n_kf), summary=s)
        print(f"# window/n_kf = {n_kf}: {info['iterations']} iterations, {info['successful_steps']} successful, {info['termination']}")
        put(f"window/n_kf = {n_kf}/state_out", final)
        put(f"window/n_kf = {n_kf}/slots", *[b for k in range(n_kf) for b in slot_state(m, k)])
        put(f"window/n_kf = {n_kf}/summary", bytes(s))


REC_T0, REC_Q0 = np.array([1.5, -2.25, 0.125]), np.array([0.5, 0.5, -0.5, 0.5])


def step_record(ang):
    """A Gauss-Newton record (LILI_GRAM_DOUBLES) whose step from the pose (REC_T0, REC_Q0) turns by `ang` rad about a skew axis: rows 3..6 of the Gram are the plus-Jacobian
    of REC_Q0 (orthonormal columns for a unit quaternion), so P^T G P = I on the rotation block and P^T G7r = -step"""
    G = np.zeros((8, 8))
    G[0, 0], G[1, 1], G[2, 2] = 4.0, 16.0, 0.25
    x0, x1, x2, x3 = REC_Q0
    Jq = np.array([[-x1, -x2, -x3], [x0, x3, -x2], [-x3, x0, x1], [x2, -x1, x0]])
    G[3:7, 3:7] = Jq @ Jq.T
    step = ang * np.array([0.6, -0.64, 0.48])
    G[3:7, 7] = -(Jq @ step)
    G[7, 3:7] = G[3:7, 7]
    G[:3, 7] = G[7, :3] = [-0.5, 0.25, 1.0]
    G[7, 7] = 1.0
    rec = np.zeros(L.api.GRAM_DOUBLES)
    rec[:64] = G.ravel()
    return rec


def case_gn(ctx):
    import torch
    ctx.set_option("persistent_iterate", 0)
    work = synth.make_workload(n_map=40_000, n_az=32, half_extent=(45.0, 40.0))
    for flavour in ("rot", "frontend"):
        P = L.make_params(flavour)
        m = L.ScanToMapMatcher(ctx, P)
        m.set_input_cloud(L.KIND_SURF, work["map_xyz"])
        for s in (0, 2):
            m.set_queries(s, L.KIND_SURF, work["scan_xyz"])
        tb, qb = L.api.body_pose_from_lidar(work["lidar_t"], work["lidar_q"], P)
        gram = torch.zeros(L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        # the whole scan, started off by `deg`, then thin slices of it: too few neighbours inside the gate, no valid row, the step is rejected
        for deg, n_q in ((0.4, 0), (35.0, 0), (35.0, 12), (35.0, 24), (35.0, 48), (35.0, 96)):
            for s in (0, 2):
                m.set_queries(s, L.KIND_SURF, work["scan_xyz"][:n_q] if n_q else work["scan_xyz"])
            t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(5), 0.05, deg)
            m.pose_set(0, t0, q0)
            m.pose_set(2, t0, q0)
            nq = n_q or "all"
            for it in range(3):
                m.associate_dev(0, L.MASK_SURF)
                m.linearize_dev(0, gram.data_ptr(), L.MASK_SURF)
                m.gn_update(0, gram.data_ptr())
                m.iterate(2, 1, L.MASK_SURF)
                a, b = slot_state(m, 0), slot_state(m, 2)
                print(f"# gn/{flavour}/{deg} deg, {nq} queries, iteration {it}: |rotation step| one lane {np.linalg.norm(a[2][3:]):.4f} rad (status {int(a[3][0])}), "
                      f"six lanes {np.linalg.norm(b[2][3:]):.4f} rad (status {int(b[3][0])})")
                put(f"gn/{flavour}/{deg} deg/{nq} queries/iteration {it}/one lane", *a)
                put(f"gn/{flavour}/{deg} deg/{nq} queries/iteration {it}/six lanes", *b)
    # the one-lane tail on a record of the caller's (step_record): steps of 0.9 rad (the large-angle branch of the quaternion update) and 0.3 rad
    m = L.ScanToMapMatcher(ctx, L.make_params("rot"))
    for ang in (0.9, 0.3):
        gram = torch.from_numpy(step_record(ang)).to("cuda")
        torch.cuda.synchronize()
        m.pose_set(5, REC_T0, REC_Q0)
        m.gn_update(5, gram.data_ptr())
        a = slot_state(m, 5)
        print(f"# gn/hand-built record, {ang} rad: |rotation step| {np.linalg.norm(a[2][3:]):.4f} rad (status {int(a[3][0])})")
        put(f"gn/hand-built record/{ang} rad/one lane", *a)
    # The six-lane tail on the same records.  The sharded window iteration hands its reduced records to the caller's all-reduce and runs the update of every slot on what
    # comes back (k_window_gn): an "all-reduce" that replaces the records gives the six-lane solver a caller's record.  Without a callback the same call ends inside the
    # reduction launch (k_window_reduce) on the scan's own records.
    for flavour in ("rot", "frontend"):
        m = L.ScanToMapMatcher(ctx, L.make_params(flavour))
        m.set_input_cloud(L.KIND_SURF, work["map_xyz"])
        for s in (0, 1):
            m.set_queries(s, L.KIND_SURF, work["scan_xyz"])
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        gram = torch.zeros(2 * L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
        recs = torch.from_numpy(np.concatenate([step_record(0.9), step_record(0.3)]))
        CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)

        def replace_records(send, recv, count, dtype, op, comm, stream):
            if recv == gram.data_ptr() and count == gram.numel():      # (the counts of the count-scaled flavour pass through)
                torch.cuda.synchronize()
                gram.copy_(recs)
                torch.cuda.synchronize()
            return 0
        cb = CB(replace_records)
        torch.cuda.synchronize()
        for s in (0, 1):
            m.pose_set(s, REC_T0, REC_Q0)
        m.iterate_window_sharded([0, 1], 1, counts.data_ptr(), gram.data_ptr(), C.cast(cb, C.c_void_p).value, None, L.MASK_SURF)
        ctx.sync()
        for s, ang in ((0, 0.9), (1, 0.3)):
            a = slot_state(m, s)
            print(f"# gn/{flavour}/hand-built record, {ang} rad, six lanes (k_window_gn): |rotation step| {np.linalg.norm(a[2][3:]):.4f} rad (status {int(a[3][0])})")
            put(f"gn/{flavour}/hand-built record/{ang} rad/six lanes", *a)
        tb, qb = L.api.body_pose_from_lidar(work["lidar_t"], work["lidar_q"], m.params)
        for s in (0, 1):
            m.pose_set(s, *synth.perturbed_pose(tb, qb, np.random.default_rng(5 + s), 0.05, 0.4))
        m.iterate_window_sharded([0, 1], 3, counts.data_ptr(), gram.data_ptr(), None, None, L.MASK_SURF)
        ctx.sync()
        a = [b for s in (0, 1) for b in slot_state(m, s)]
        print(f"# gn/{flavour}/window of 2, 3 iterations (k_window_reduce): status {int(a[3][0])}, {int(a[7][0])}")
        put(f"gn/{flavour}/window of 2/six lanes", *a, gram.cpu().numpy())


def case_extract(ctx):
    w = synth.make_workload(n_map=300_000, n_az=391, half_extent=(150.0, 150.0), seed=synth.SEED_SCENE)
    refl = np.random.default_rng(0).integers(1, 255, w["scan_xyz"].shape[0]).astype(np.float32)
    raw = np.concatenate([w["scan_xyz"], refl[:, None]], 1).astype(np.float32)
    ang = 0.6
    away = [np.cos(ang / 2), np.sin(ang / 2) * 0.3, -np.sin(ang / 2) * 0.5, np.sin(ang / 2) * 0.81]
    for name, q_imu in (("q_imu 0.6 rad", away), ("q_imu identity", [1.0, 0.0, 0.0, 0.0])):
        g = L.RotExtractor(ctx, n_scans=64, ds_rate=4).extract(raw, q_imu, [0.7071, 0.0, 0.0, 0.7071])
        print(f"# extract/rot/{name}: {len(g['full'])} full, {len(g['edge'])} edge, {len(g['surf'])} surf")
        for k in ("full", "edge", "surf"):
            put(f"extract/rot/{name}/{k}", g[k])
        scan = synth.make_livox_scan(3)
        g = L.LivoxExtractor(ctx).extract(scan, q_imu)
        print(f"# extract/livox/{name}: {len(g['cutted'])} cut, {len(g['edge'])} edge, {len(g['surf'])} surf")
        for k in ("cutted", "edge", "surf"):
            put(f"extract/livox/{name}/{k}", g[k])


def main():
    ctx = L.Context(0)
    try:
        for case in (case_lm, case_coop, case_window, case_gn, case_extract):
            case(ctx)
    finally:
        ctx.close()
    h = hashlib.sha256("".join(f"{k}={v};" for k, v in OUT.items()).encode()).hexdigest()
    print(f"{'ALL (' + str(len(OUT)) + ' buffers)':58s} {h}")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(OUT, f, indent=1)


if __name__ == "__main__":
    main()
