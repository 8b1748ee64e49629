"""The Gauss-Newton tail of the outer iteration (gn_update_block in lili_s2m.hip) and the restart of a registration without a copy launch.

* The tail exists twice: k_gn_update (the split / multi-GPU path) factorises the 6x6 normal matrix on ONE lane, the reduction + GN kernel of lili_s2m_iterate*
  on SIX lanes (row i on lane i).  Both run the same operations on the same operands in the same order, so pose, step and status agree to the last bit.
* A rejected step (no valid row: the first pivot is not positive) leaves the pose bit-unchanged on both paths and through the page-locked mirror of the
  front-end frame call.
* A step without rotation (nd2 == 0) keeps the quaternion's bits.
* lili_s2m_iterate_restart reads the first pose of every registration from the restart slot instead of copying it: it equals pose_copy + iterate(1), step by step.

Workload: synth.make_workload cut down to a 40 k-point map and a 2 k-ray scan (a few hundred surf rows)."""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth

pytestmark = pytest.mark.gpu

FLAVOURS = ["rot", "frontend"]          # count-scaled (three launches per iteration) / not count-scaled (association + linearisation in one launch)


@pytest.fixture(scope="module")
def work():
    w = synth.make_workload(n_map=40_000, n_az=32, half_extent=(45.0, 40.0))
    assert 1500 <= w["scan_xyz"].shape[0] <= 2048
    return w


def _matcher(ctx, work, flavour, slots, queries=None):
    P = L.make_params(flavour)
    m = L.ScanToMapMatcher(ctx, P)
    m.set_input_cloud(L.KIND_SURF, work["map_xyz"])
    q = work["scan_xyz"] if queries is None else queries
    for s in slots:
        m.set_queries(s, L.KIND_SURF, q)
    tb, qb = L.api.body_pose_from_lidar(work["lidar_t"], work["lidar_q"], P)
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(5), 0.05, 0.4)
    return m, t0, q0


def _state(m, slot):
    """everything the host sees of a slot's state: pose, status, last step, update count"""
    t, q, st = m.pose_get(slot)
    d, n, st2 = m.last_step(slot)
    assert st == st2
    return np.concatenate([t, q, d]).view(np.uint64), n, st


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def _same_records(a, b):
    return a["count"] == b["count"] and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("query_index", "cp", "n", "d", "score"))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_lanes_equal_the_single_lane_solver_bit_for_bit(launch_by_launch, work, flavour):
    """slot 0: associate_dev + linearize_dev + gn_update (k_gn_update: one lane); slot 2: iterate(1) (k_reduce_partials: six lanes); 10 consecutive iterations.
    The flavour without count scaling linearises inside its association launch by default, which partitions the Gram sum differently (last bits of the RECORD):
    fuse_lin = 0 gives both slots the same record, so that the comparison is between the two solvers."""
    import torch
    ctx = launch_by_launch
    m, t0, q0 = _matcher(ctx, work, flavour, (0, 2))
    gram = torch.zeros(L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    m.pose_set(0, t0, q0)
    m.pose_set(2, t0, q0)
    ctx.set_option("fuse_lin", 0)
    try:
        moved = False
        for it in range(10):
            m.associate_dev(0, L.MASK_SURF)
            m.linearize_dev(0, gram.data_ptr(), L.MASK_SURF)
            m.gn_update(0, gram.data_ptr())
            m.iterate(2, 1, L.MASK_SURF)
            a, b = _state(m, 0), _state(m, 2)
            assert a[2] == 0 and a[1] == it + 1
            assert _same_state(a, b), (flavour, it)
            moved = moved or bool(np.any(a[0][7:13] != 0))
        assert moved
        ctx.sync()
        n_rows = int(gram.cpu()[65])
        assert 200 <= n_rows <= 2048, n_rows
    finally:
        ctx.set_option("fuse_lin", 1)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_rejected_step_leaves_the_pose_unchanged(launch_by_launch, work, flavour):
    """queries 50 m outside the map: no valid row, H = 0, the first pivot is not positive — status 1 on both paths, the pose keeps its bits; a restart that
    falls on such a step still initialises the slot from the restart slot"""
    import torch
    ctx = launch_by_launch
    far = work["scan_xyz"] + np.array([45.0 + 50.0 + 60.0, 0.0, 0.0], np.float32)
    m, t0, q0 = _matcher(ctx, work, flavour, (0, 2, 3), queries=far)
    gram = torch.zeros(L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for s in (0, 1, 2):
        m.pose_set(s, t0, q0)
    want = np.concatenate([t0, q0]).view(np.uint64)
    m.associate_dev(0, L.MASK_SURF)
    m.linearize_dev(0, gram.data_ptr(), L.MASK_SURF)
    m.gn_update(0, gram.data_ptr())
    m.iterate(2, 1, L.MASK_SURF)
    for s in (0, 2):
        bits, n, st = _state(m, s)
        assert st == 1 and n == 1 and np.array_equal(bits[:7], want) and not np.any(bits[7:]), (flavour, s)
    assert m.surf_records(2, far.shape[0])["count"] == 0
    m.pose_set(3, t0 + 1.0, q0)
    m.iterate_restart(3, 1, 1, 1, L.MASK_SURF)
    bits, n, st = _state(m, 3)
    assert st == 1 and n == 1 and np.array_equal(bits[:7], want)


def test_rejected_step_through_the_pose_mirror():
    """the front-end frame call reads the pose from the page-locked mirror the reduction + GN kernel writes: a frame predicted 80 m away from the ring's map
    matches nothing, and the call returns the predicted pose bit for bit (translation included) with status 1"""
    from tests.test_frontend_frame_gpu import _circuit
    ctx = L.Context(0)
    try:
        odo = L.FrontendOdometry(ctx, L.make_params("frontend"), width=5, scan_match_cnt=3, first_match_cnt=3, reference_startup=False)
        odo.reset()
        t0, q0 = _circuit(0)[:2]
        t, q, info = odo.frame(synth.make_livox_scan(100, origin=t0, yaw=_circuit(0)[2], inject_bad=False), t0, q0)
        assert not info["matched"]
        t_far = np.asarray(t0, np.float64) + np.array([80.0, 0.0, 0.0])
        q_far = np.array([np.cos(0.1), 0.0, 0.0, np.sin(0.1)])
        t, q, info = odo.frame(synth.make_livox_scan(101, origin=_circuit(1)[0], yaw=_circuit(1)[2], inject_bad=False), t_far, q_far)
        assert info["matched"] and info["gn_status"] == 1 and info["n_query"] > 100
        assert np.array_equal(t.view(np.uint64), t_far.view(np.uint64)) and np.array_equal(q.view(np.uint64), q_far.view(np.uint64))
    finally:
        ctx.close()


def test_step_without_rotation_keeps_the_quaternion(gpu_ctx, oracle):
    """A hand-built record whose rotation rows and rotation right-hand side are zero apart from a unit block: nd2 == 0, so the quaternion is not touched.  The
    API offers no way to feed a caller's record to the reduction + GN kernel (it builds its record from the partials of its own linearisation), so this case
    runs k_gn_update alone and is set against the host restatement oracle.gn_step (Cholesky) within 1 ulp.  The translation block is diag(4, 16, 1/4):
    square roots, pivots and quotients are exact in both."""
    import torch
    G = np.zeros((8, 8))
    G[0, 0], G[1, 1], G[2, 2] = 4.0, 16.0, 0.25
    for i in range(3, 7):
        G[i, i] = 1.0
    r = np.array([-0.5, 0.25, 1.0])
    G[:3, 7] = r
    G[7, :3] = r
    G[7, 7] = 1.0
    rec = np.zeros(L.api.GRAM_DOUBLES)
    rec[:64] = G.ravel()
    t0 = np.array([1.5, -2.25, 0.125])
    q0 = np.array([0.5, 0.5, -0.5, 0.5])            # unit, every product with it exact
    m = L.ScanToMapMatcher(gpu_ctx, L.make_params("rot"))
    gram = torch.from_numpy(rec).to("cuda")
    torch.cuda.synchronize()
    m.pose_set(5, t0, q0)
    m.gn_update(5, gram.data_ptr())
    t, q, st = m.pose_get(5)
    d, n, _ = m.last_step(5)
    st_o, t_o, q_o, d_o = oracle.gn_step(G, t0, q0)
    assert st == st_o == 0 and n == 1
    assert np.all(d[3:] == 0.0) and np.all(d_o[3:] == 0.0)
    assert np.array_equal(q.view(np.uint64), q0.view(np.uint64)) and np.array_equal(q_o, q0)
    assert np.all(np.abs(t - t_o) <= np.spacing(np.abs(t_o))) and np.all(np.abs(d[:3] - d_o[:3]) <= np.spacing(np.abs(d_o[:3])))
    assert np.array_equal(d[:3], -r / np.array([4.0, 16.0, 0.25]))


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("k,r", [(1, 1), (3, 1), (7, 3), (10, 10), (20, 10), (11, 10)])
def test_restart_without_a_copy_equals_pose_copy_and_iterate(launch_by_launch, work, flavour, k, r):
    """iterate_restart(0, k, r, 1) against the explicit sequence in slot 3: pose_copy(3, 1) before steps 0, r, 2 r, ... and iterate(3, 1) per step.  Pose, last
    step, update count, status and the surf records agree bit for bit after the call, after a second call on top of it, and the restart slot keeps its bits."""
    ctx = launch_by_launch
    m, t0, q0 = _matcher(ctx, work, flavour, (0, 3))
    n_q = work["scan_xyz"].shape[0]
    m.pose_set(1, t0, q0)
    other = synth.perturbed_pose(t0, q0, np.random.default_rng(6), 0.2, 1.0)      # replaced by the first restart
    m.pose_set(0, *other)
    m.pose_set(3, *other)
    slot1 = (_state(m, 1), m.debug_times(1))
    for call in range(2):
        m.iterate_restart(0, k, r, 1, L.MASK_SURF)
        for it in range(k):
            if it % r == 0:
                m.pose_copy(3, 1)
            m.iterate(3, 1, L.MASK_SURF)
        a, b = _state(m, 0), _state(m, 3)
        assert a[2] == 0 and a[1] == (call + 1) * k
        assert _same_state(a, b), (flavour, k, r, call)
        assert _same_records(m.surf_records(0, n_q), m.surf_records(3, n_q))
        now1 = (_state(m, 1), m.debug_times(1))
        assert _same_state(now1[0], slot1[0]) and now1[1] == slot1[1]
    assert np.any(_state(m, 0)[0][:7] != np.concatenate([t0, q0]).view(np.uint64))
