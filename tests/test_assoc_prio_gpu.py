"""Option assoc_prio (the one-lane association kernels change their waves' issue priority by phase) changes scheduling and never a bit.

One small scene at which a misplaced priority call could still go wrong — the last wave partly live, lanes that leave the search early (NaN rows, rows
several cells outside the grid), lanes that walk the shell of the 5x5x5 block while their neighbours are done — goes through every one-lane launch shape
with assoc_prio 0 and 1: k_associate_surf / k_associate_edge (one launch per kind), k_associate_both (both kinds in one launch), k_associate_lin (the
front-end flavour, which linearises in the association launch; fuse_lin_block = 64), a ROT registration with restarts, and k_associate_coop<2> (assoc_lpq
= 2, the first launch after pose_set, which carries the option as well).  Records, counts and poses must
agree bit for bit.  The per-workgroup counts are not readable from outside; what is compared is their sum as the device takes it (the returned count) and
the valid flags they count (the records' query indices), which must also agree with each other."""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth

pytestmark = pytest.mark.gpu

N_SURF = 64 * 65 + 37          # the last wave of the surf launch has 37 live lanes
N_EDGE = 517
BOTH = L.MASK_SURF | L.MASK_EDGE


@pytest.fixture(scope="module")
def scene():
    w = synth.make_workload(n_map=60_000, n_az=80, half_extent=(60.0, 50.0))
    rng = np.random.default_rng(5)
    t_l = np.asarray(w["lidar_t"], np.float64)
    surf = w["scan_xyz"][rng.choice(w["scan_xyz"].shape[0], N_SURF, replace=False)].astype(np.float64)
    shell = rng.choice(N_SURF, 300, replace=False)              # more than 1 m off every surface they came from: nothing in the inner block, the shell walk
    d = rng.normal(0, 1, (300, 3))
    surf[shell] += 1.2 * d / np.linalg.norm(d, axis=1, keepdims=True)
    rest = np.setdiff1d(np.arange(N_SURF), shell)
    special = rng.choice(rest, 9, replace=False)
    for k in range(3):
        surf[special[k], k] = np.nan                            # a NaN coordinate each
    surf[special[3:]] += np.array([[400.0, 0, 0], [0, -400.0, 0], [0, 0, 90.0], [-400.0, 400.0, 0], [300.0, 0, -50.0], [0, 500.0, 0]])      # cells outside the grid
    surf[N_SURF - 1] = [np.nan, 0.0, 0.0]                       # and one in the partly live wave
    em = w["edge_map_xyz"].astype(np.float64)
    near = em[np.linalg.norm(em[:, :2], axis=1) < 50.0]
    edge = near[rng.choice(near.shape[0], N_EDGE)] + rng.normal(0, 0.03, (N_EDGE, 3)) - t_l      # LiDAR frame (the generator's LiDAR has no rotation)
    edge[7] += 300.0
    edge[300, 1] = np.nan
    return dict(map=w["map_xyz"], edge_map=w["edge_map_xyz"], surf=surf.astype(np.float32), edge=edge.astype(np.float32), lidar_t=t_l)


def _poses(P, scene, flavour):
    if flavour == "frontend":                                   # identity extrinsic: the body frame is the LiDAR frame
        tb, qb = scene["lidar_t"].copy(), np.array([1.0, 0.0, 0.0, 0.0])
    else:
        qb = np.array(list(P.q_lb))
        qb = qb / np.linalg.norm(qb)
        _, t2 = L.api.assoc_transform([0.0, 0.0, 0.0], qb, P)
        tb = scene["lidar_t"] - t2
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(11), 0.1, 0.5)
    return tb, qb, t0, q0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _records(m):
    s, e = m.surf_records(0, N_SURF), m.edge_records(0, N_EDGE)
    out = {"surf_count": s["count"], "edge_count": e["count"]}
    for k in ("query_index", "n", "d", "score"):
        out["surf_" + k] = _bits(s[k])
    for k in ("query_index", "a", "b", "s"):
        out["edge_" + k] = _bits(e[k])
    return out


def _run(scene, prio, shape):
    flavour = "frontend" if shape == "lin" else "rot"
    P = L.make_params(flavour)
    tb, qb, t0, q0 = _poses(P, scene, flavour)
    ctx = L.Context(0)
    try:
        ctx.set_option("assoc_lpq", 2 if shape == "coop" else 1)      # 1: the one-lane kernels at this size
        ctx.set_option("assoc_prio", prio)
        if shape == "lin":
            ctx.set_option("fuse_lin_block", 64)
        m = L.ScanToMapMatcher(ctx, P)
        m.set_input_cloud(L.KIND_SURF, scene["map"])
        m.set_input_cloud(L.KIND_EDGE, scene["edge_map"])
        assert m.map_density(L.KIND_SURF)[1] == 0.0             # no fine index: the gate-sized grid, the kernels under test
        m.set_queries(0, L.KIND_SURF, scene["surf"])
        m.set_queries(0, L.KIND_EDGE, scene["edge"])
        qa, ta = L.api.assoc_transform(t0, q0, P)
        out = {}
        if shape == "per_kind":
            out["n_surf"] = m.find_corresponding_surf_features(0, qa, ta)
            out["n_edge"] = m.find_corresponding_corner_features(0, qa, ta)
            out.update(_records(m))
        elif shape == "both":
            (out["n_surf"], out["n_edge"]), = m.associate_window([0], [ta], [qa], BOTH)
            out.update(_records(m))
        elif shape in ("lin", "coop"):                          # coop: ROT flavour, one iteration = k_associate_coop<2, false> + linearise + reduce
            m.pose_set(0, t0, q0)
            m.iterate(0, 2 if shape == "lin" else 1, BOTH)
            t, q, st = m.pose_get(0)
            d, n, st2 = m.last_step(0)
            out.update(_records(m))
            out.update(pose=_bits(np.concatenate([t, q, d])), steps=(n, st, st2))
        else:
            m.pose_set(0, tb + 5.0, qb)
            m.pose_set(1, t0, q0)
            m.iterate_restart(0, 6, 3, 1, BOTH)
            t, q, st = m.pose_get(0)
            d, n, st2 = m.last_step(0)
            out.update(pose=_bits(np.concatenate([t, q, d])), steps=(n, st, st2))
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", ["per_kind", "both", "lin", "rot_restart", "coop"])
def test_priority_changes_no_bit(scene, shape):
    off, on = _run(scene, 0, shape), _run(scene, 1, shape)
    assert off.keys() == on.keys()
    for k in off:
        if isinstance(off[k], np.ndarray):
            assert off[k].shape == on[k].shape and np.array_equal(off[k], on[k]), (shape, k)
        else:
            assert off[k] == on[k], (shape, k, off[k], on[k])
    if "surf_count" in off:
        # the scene is not degenerate (3 925 surf and 510 edge queries have five map points inside the gate) and the 4 NaN + 6 outside surf rows and
        # the 2 such edge rows leave no record
        assert 1000 < off["surf_count"] <= N_SURF - 10 and 0 < off["edge_count"] <= N_EDGE - 2, (off["surf_count"], off["edge_count"])
    if "n_surf" in off:
        assert off["n_surf"] == off["surf_count"] and off["n_edge"] == off["edge_count"]      # the sum of the block counts is the number of valid flags
    if "steps" in off:
        assert off["steps"][1] == 0 and off["steps"][0] == {"lin": 2, "rot_restart": 6, "coop": 1}[shape]      # GN updates since pose_set, off["steps"]
