"""GPU parity tests of the scan-to-map matcher: HIP path (through the C ABI) vs the CPU oracle on the
same seeded inputs.  Bars: neighbour indices / valid flags exact; f32 record fields within 1 ulp-ish
(the f64 plane fit differs in the last bits between the two independent QR codes); Gram 1e-10
relative; pose after 10 Gauss-Newton iterations within 1e-4 m / 1e-4 rad (north-star tolerance).
"""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth

pytestmark = pytest.mark.gpu

VARIANTS = ["rot", "livox", "frontend"]


def _setup(gpu_ctx, oracle, variant, room, with_refl):
    P = L.make_params(variant)
    PO = oracle.params(variant)
    m = L.ScanToMapMatcher(gpu_ctx, P)
    gpu_ctx.set_debug(True)
    if with_refl:
        m.set_input_cloud(L.KIND_SURF, np.concatenate([room["map_xyz"], room["map_refl"][:, None]], 1))
        m.set_queries(0, L.KIND_SURF, np.concatenate([room["q_xyz"], room["q_refl"][:, None]], 1))
    else:
        m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
        m.set_queries(0, L.KIND_SURF, room["q_xyz"])
    m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
    m.set_queries(0, L.KIND_EDGE, room["eq_xyz"])
    return P, PO, m


def _pose(room, P, variant, rng=None, dt=0.0, dang=0.0):
    t, q = room["t_true"].copy(), room["q_true"].copy()
    if variant != "frontend":
        t, q = L.api.body_pose_from_lidar(t, q, P)      # room poses are LiDAR poses
    if rng is not None:
        t, q = synth.perturbed_pose(t, q, rng, dt, dang)
    if variant == "frontend":
        return t, q, q.copy(), t.copy()
    Q2, T2 = L.api.assoc_transform(t, q, P)
    return t, q, Q2, T2


def _scales(variant, n_s, n_e):
    if variant == "rot":
        return (1000.0, max(n_s, 1)), (200.0, max(n_e, 1))
    return 1.0, 1.0


@pytest.mark.parametrize("variant", VARIANTS)
def test_association_parity(gpu_ctx, oracle, variant):
    room = synth.make_room(seed=11, n_query=6000, n_edge_query=600)
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
    rng = np.random.default_rng(5)
    t, q, Q2, T2 = _pose(room, P, variant, rng, 0.02, 0.1)   # ROT keeps edges only within 0.1 m of the line
    n_s = m.find_corresponding_surf_features(0, Q2, T2)
    n_e = m.find_corresponding_corner_features(0, Q2, T2)
    tree = oracle.KdTree(room["map_xyz"])
    etree = oracle.KdTree(room["edge_map_xyz"])
    rs = oracle.associate_surf(tree, room["map_refl"] if variant == "livox" else None, room["q_xyz"],
                               room["q_refl"] if variant == "livox" else None, Q2, T2, PO)
    re_ = oracle.associate_edge(etree, room["eq_xyz"], Q2, T2, PO)
    assert rs["count"] > 1000 and re_["count"] > 50, "test scene must produce correspondences"
    assert n_s == rs["count"] and n_e == re_["count"]
    # neighbour lists: exact wherever the reference's gate can pass
    for kind, rec, gate, nq in ((L.KIND_SURF, rs, PO.kd_max_radius, room["q_xyz"].shape[0]),
                                (L.KIND_EDGE, re_, PO.edge_gate, room["eq_xyz"].shape[0])):
        idx, d2 = m.neighbors(0, kind, nq)
        inside = rec["nn_d2"][:, 4] < gate
        assert inside.sum() > 0
        assert np.array_equal(idx[inside], rec["nn_idx"][inside])
        assert np.array_equal(d2[inside], rec["nn_d2"][inside])          # bit-exact f32 distances
        assert np.all(~(d2[~inside][:, 4] < gate))                        # never a false accept
    # ordered record lists
    g = m.surf_records(0, room["q_xyz"].shape[0])
    sel = np.nonzero(rs["valid"])[0]
    assert np.array_equal(g["query_index"], sel)
    assert np.array_equal(g["cp"], rs["cp"][sel])
    np.testing.assert_allclose(g["n"], rs["n"][sel], rtol=3e-7, atol=1e-9)
    np.testing.assert_allclose(g["d"], rs["d"][sel], rtol=3e-7, atol=1e-9)
    np.testing.assert_allclose(g["score"], rs["score"][sel], rtol=3e-7)
    ge = m.edge_records(0, room["eq_xyz"].shape[0])
    sel = np.nonzero(re_["valid"])[0]
    assert np.array_equal(ge["query_index"], sel)
    assert np.array_equal(ge["cp"], re_["cp"][sel])
    np.testing.assert_allclose(ge["a"], re_["a"][sel], rtol=0, atol=2e-6)
    np.testing.assert_allclose(ge["b"], re_["b"][sel], rtol=0, atol=2e-6)
    assert np.array_equal(ge["s"], re_["s"][sel])


@pytest.mark.parametrize("variant", VARIANTS)
def test_linearize_gram_parity(gpu_ctx, oracle, variant):
    room = synth.make_room(seed=12, n_query=5000, n_edge_query=500)
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
    rng = np.random.default_rng(6)
    t, q, Q2, T2 = _pose(room, P, variant, rng, 0.08, 1.0)
    n_s = m.find_corresponding_surf_features(0, Q2, T2)
    n_e = m.find_corresponding_corner_features(0, Q2, T2)
    tree = oracle.KdTree(room["map_xyz"])
    etree = oracle.KdTree(room["edge_map_xyz"])
    rs = oracle.associate_surf(tree, room["map_refl"] if variant == "livox" else None, room["q_xyz"],
                               room["q_refl"] if variant == "livox" else None, Q2, T2, PO)
    re_ = oracle.associate_edge(etree, room["eq_xyz"], Q2, T2, PO)
    ss, se = _scales(variant, rs["count"], re_["count"])
    # the GPU linearises ITS OWN records; to isolate the linearisation the oracle uses its own too and
    # the association test above bounds the record differences
    for mask, want in ((L.MASK_SURF, "s"), (L.MASK_EDGE, "e"), (L.MASK_SURF | L.MASK_EDGE, "se")):
        if variant == "frontend" and "e" in want:
            continue   # the front-end has no edge factors (L/src/LidarOdometry.cpp:513-526)
        # linearise at a pose different from the association pose, like the LM iterations do
        t2, q2 = synth.perturbed_pose(t, q, np.random.default_rng(7), 0.02, 0.2)
        G, cost, counts = m.linearize(0, t2, q2, mask)
        Go = np.zeros((8, 8)); co = 0.0
        if "s" in want:
            g1, c1, n1 = oracle.linearize_surf(rs, t2, q2, PO, ss)
            Go += g1; co += c1
            assert counts[0] == n1 == n_s
        if "e" in want:
            g2, c2, n2 = oracle.linearize_edge(re_, t2, q2, PO, se)
            Go += g2; co += c2
            assert counts[1] == n2 == n_e
        scale = np.abs(Go).max()
        assert np.abs(G - Go).max() <= 2e-6 * scale      # f32 record ulps dominate; see exact-record check below
        assert abs(cost - co) <= 2e-6 * max(abs(co), 1e-12)
        assert np.allclose(G, G.T, rtol=0, atol=0)


def test_linearize_exact_records(gpu_ctx, oracle):
    """Same records on both sides (GPU records fed to the oracle): Gram must agree to 1e-12 relative."""
    room = synth.make_room(seed=13, n_query=5000, n_edge_query=500)
    variant = "rot"
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=False)
    t, q, Q2, T2 = _pose(room, P, variant, np.random.default_rng(8), 0.05, 0.7)
    n_s = m.find_corresponding_surf_features(0, Q2, T2)
    n_e = m.find_corresponding_corner_features(0, Q2, T2)
    nq, ne = room["q_xyz"].shape[0], room["eq_xyz"].shape[0]
    g = m.surf_records(0, nq)
    ge = m.edge_records(0, ne)
    rs = dict(valid=np.zeros(nq, np.uint8), cp=np.zeros((nq, 3), np.float32), n=np.zeros((nq, 3), np.float32),
              d=np.zeros(nq, np.float32), score=np.zeros(nq))
    rs["valid"][g["query_index"]] = 1
    rs["cp"][g["query_index"]] = g["cp"]; rs["n"][g["query_index"]] = g["n"]
    rs["d"][g["query_index"]] = g["d"]; rs["score"][g["query_index"]] = g["score"]
    re_ = dict(valid=np.zeros(ne, np.uint8), cp=np.zeros((ne, 3), np.float32), a=np.zeros((ne, 3), np.float32),
               b=np.zeros((ne, 3), np.float32), s=np.zeros(ne, np.float32))
    re_["valid"][ge["query_index"]] = 1
    re_["cp"][ge["query_index"]] = ge["cp"]; re_["a"][ge["query_index"]] = ge["a"]
    re_["b"][ge["query_index"]] = ge["b"]; re_["s"][ge["query_index"]] = ge["s"]
    G, cost, counts = m.linearize(0, t, q, L.MASK_SURF | L.MASK_EDGE)
    g1, c1, n1 = oracle.linearize_surf(rs, t, q, PO, (1000.0, n_s))
    g2, c2, n2 = oracle.linearize_edge(re_, t, q, PO, (200.0, n_e))
    Go = g1 + g2
    assert (counts[0], counts[1]) == (n1, n2)
    assert np.abs(G - Go).max() <= 1e-12 * np.abs(Go).max()
    assert abs(cost - (c1 + c2)) <= 1e-12 * abs(c1 + c2)


@pytest.mark.parametrize("variant", VARIANTS)
def test_gauss_newton_pose_parity(gpu_ctx, oracle, variant):
    """10 outer iterations (re-associate + linearise + GN step) entirely on the device vs the oracle loop."""
    room = synth.make_room(seed=14, n_query=8000, n_edge_query=800, noise=0.005)
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
    rng = np.random.default_rng(synth.SEED_POSE)
    t_ref, q_ref, _, _ = _pose(room, P, variant)
    t0, q0 = synth.perturbed_pose(t_ref, q_ref, rng, 0.15, 1.0)
    mask = L.MASK_SURF if variant == "frontend" else (L.MASK_SURF | L.MASK_EDGE)
    m.pose_set(0, t0, q0)
    m.iterate(0, 10, mask)
    tg, qg, status = m.pose_get(0)
    assert status == 0
    # oracle loop
    tree = oracle.KdTree(room["map_xyz"])
    etree = oracle.KdTree(room["edge_map_xyz"])
    t, q = t0.copy(), q0.copy()
    for _ in range(10):
        if variant == "frontend":
            Q2, T2 = q, t
        else:
            Q2, T2 = L.api.assoc_transform(t, q, P)
        rs = oracle.associate_surf(tree, room["map_refl"] if variant == "livox" else None, room["q_xyz"],
                                   room["q_refl"] if variant == "livox" else None, Q2, T2, PO)
        ss, se = 1.0, 1.0
        G, _, _ = None, None, None
        if mask & L.MASK_EDGE:
            re_ = oracle.associate_edge(etree, room["eq_xyz"], Q2, T2, PO)
            ss, se = _scales(variant, rs["count"], re_["count"])
            G = oracle.linearize_surf(rs, t, q, PO, ss)[0] + oracle.linearize_edge(re_, t, q, PO, se)[0]
        else:
            ss, _ = _scales(variant, rs["count"], 1)
            G = oracle.linearize_surf(rs, t, q, PO, ss)[0]
        st, t, q, _ = oracle.gn_step(G, t, q)
        assert st == 0
    assert np.abs(tg - t).max() < 1e-4
    dq = synth.quat_mul(qg * np.array([1, -1, -1, -1]), q)
    ang = 2 * np.arcsin(min(1.0, np.linalg.norm(dq[1:])))
    assert ang < 1e-4
    # and the iteration did converge towards the truth (the edge factor ignores the extrinsic — SURVEY F6 —
    # so with a non-trivial q_lb it pulls away from it; only the plane-only variant is asserted)
    if variant == "frontend":
        assert np.linalg.norm(tg - t_ref) < 0.3 * np.linalg.norm(t0 - t_ref)


def test_host_pose_and_device_pose_paths_agree(gpu_ctx, oracle):
    room = synth.make_room(seed=15, n_query=3000, n_edge_query=300)
    P, PO, m = _setup(gpu_ctx, oracle, "rot", room, with_refl=False)
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(3), 0.1, 0.5)
    Q2, T2 = L.api.assoc_transform(t0, q0, P)
    m.find_corresponding_surf_features(0, Q2, T2)
    G, cost, counts = m.linearize(0, t0, q0, L.MASK_SURF)
    st, t1, q1, _ = L.api.gn_step_host(G, t0, q0)
    assert st == 0
    m.pose_set(0, t0, q0)
    m.iterate(0, 1, L.MASK_SURF)
    t2, q2, st2 = m.pose_get(0)
    assert st2 == 0
    assert np.abs(t1 - t2).max() < 1e-12 and np.abs(q1 - q2).max() < 1e-12
    d, n_up, st3 = m.last_step(0)                      # the step the device took = the host mirror's
    _, _, _, d_host = L.api.gn_step_host(G, t0, q0)
    assert n_up == 1 and st3 == 0 and np.abs(d - d_host).max() < 1e-12 and np.abs(d[:3] - (t2 - t0)).max() < 1e-12


def test_edge_cases(gpu_ctx, oracle):
    P = L.make_params("rot")
    PO = oracle.params("rot")
    m = L.ScanToMapMatcher(gpu_ctx, P)
    gpu_ctx.set_debug(True)
    ident_q, zero_t = [1.0, 0, 0, 0], [0.0, 0, 0]
    room = synth.make_room(seed=16, n_query=500, n_edge_query=50)
    # (a) empty query set
    m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
    m.set_queries(0, L.KIND_SURF, np.zeros((0, 3), np.float32))
    assert m.find_corresponding_surf_features(0, ident_q, zero_t) == 0
    G, cost, counts = m.linearize(0, zero_t, ident_q, L.MASK_SURF)
    assert not G.any() and cost == 0 and counts[0] == 0
    # (b) empty map and a map with fewer than 5 points: no correspondences
    for nmap in (0, 3):
        m.set_input_cloud(L.KIND_SURF, room["map_xyz"][:nmap])
        m.set_queries(0, L.KIND_SURF, room["q_xyz"])
        assert m.find_corresponding_surf_features(0, ident_q, zero_t) == 0
    # (c) queries far outside the map's bounding box, NaN query
    m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
    far = room["q_xyz"].copy()
    far[:100] += 1000.0
    far[100] = np.nan
    m.set_queries(0, L.KIND_SURF, far)
    Q2, T2 = room["q_true"], room["t_true"]       # association transform = LiDAR pose
    n = m.find_corresponding_surf_features(0, Q2, T2)
    tree = oracle.KdTree(room["map_xyz"])
    rs = oracle.associate_surf(tree, None, far, None, Q2, T2, PO)
    assert n == rs["count"]
    g = m.surf_records(0, far.shape[0])
    assert np.array_equal(g["query_index"], np.nonzero(rs["valid"])[0])
    assert g["query_index"].min() > 100
    # (d) exact distance ties: duplicated map points -> lower original index wins, like the oracle
    dup = np.concatenate([room["map_xyz"][:2000], room["map_xyz"][:2000]], 0)
    m.set_input_cloud(L.KIND_SURF, dup)
    m.set_queries(0, L.KIND_SURF, room["q_xyz"])
    m.find_corresponding_surf_features(0, Q2, T2)
    idx, d2 = m.neighbors(0, L.KIND_SURF, room["q_xyz"].shape[0])
    tree2 = oracle.KdTree(dup)
    r2 = oracle.associate_surf(tree2, None, room["q_xyz"], None, Q2, T2, PO)
    inside = r2["nn_d2"][:, 4] < 1.0
    assert inside.sum() > 10
    assert np.array_equal(idx[inside], r2["nn_idx"][inside])
    # (e) a larger gate than the map index was built for is refused, not silently wrong
    P2 = L.make_params("rot", kd_max_radius=4.0)
    m2 = L.ScanToMapMatcher(gpu_ctx, P2)
    with pytest.raises(L.LiliError):
        m2.find_corresponding_surf_features(0, Q2, T2)
    # ... and accepted once the map is rebuilt for it (kd_max_radius = 1.5 of config_utbm.yaml)
    P3 = L.make_params("rot", kd_max_radius=1.5)
    PO3 = oracle.params("rot", kd_max_radius=1.5)
    m3 = L.ScanToMapMatcher(gpu_ctx, P3)
    m3.set_input_cloud(L.KIND_SURF, room["map_xyz"])
    m3.set_queries(0, L.KIND_SURF, room["q_xyz"])
    n3 = m3.find_corresponding_surf_features(0, Q2, T2)
    r3 = oracle.associate_surf(tree, None, room["q_xyz"], None, Q2, T2, PO3)
    assert n3 == r3["count"]


def test_mid_size_outdoor_scene(gpu_ctx, oracle):
    """Reduced config-2 scene (same generator, ~0.6 M map points, 25 k queries): neighbours + counts exact."""
    w = synth.make_workload(n_map=600_000, n_az=391, half_extent=(150.0, 150.0))
    P = L.make_params("rot")
    PO = oracle.params("rot")
    m = L.ScanToMapMatcher(gpu_ctx, P)
    gpu_ctx.set_debug(True)
    m.set_input_cloud(L.KIND_SURF, w["map_xyz"])
    m.set_queries(0, L.KIND_SURF, w["scan_xyz"])
    rng = np.random.default_rng(synth.SEED_POSE)
    # body pose whose LiDAR sits at the generator's true LiDAR pose, then perturbed by 0.3 m / 2 deg
    qlb = np.array(list(P.q_lb)); qb = qlb / np.linalg.norm(qlb)
    Q2, T2 = L.api.assoc_transform([0, 0, 0], qb, P)
    t_body = w["lidar_t"] - T2
    t0, q0 = synth.perturbed_pose(t_body, qb, rng, 0.3, 2.0)
    Q2, T2 = L.api.assoc_transform(t0, q0, P)
    n = m.find_corresponding_surf_features(0, Q2, T2)
    tree = oracle.KdTree(w["map_xyz"])
    rs = oracle.associate_surf(tree, None, w["scan_xyz"], None, Q2, T2, PO, nthreads=8)
    assert rs["count"] > 5000
    assert n == rs["count"]
    idx, d2 = m.neighbors(0, L.KIND_SURF, w["scan_xyz"].shape[0])
    inside = rs["nn_d2"][:, 4] < 1.0
    assert np.array_equal(idx[inside], rs["nn_idx"][inside])
    assert np.array_equal(d2[inside], rs["nn_d2"][inside])
    g = m.surf_records(0, w["scan_xyz"].shape[0])
    assert np.array_equal(g["query_index"], np.nonzero(rs["valid"])[0])
    G, cost, counts = m.linearize(0, t0, q0, L.MASK_SURF)
    Go, co, no = oracle.linearize_surf(rs, t0, q0, PO, (1000.0, rs["count"]))
    assert counts[0] == no
    assert np.abs(G - Go).max() <= 2e-6 * np.abs(Go).max()


_OPTION_DEFAULTS = {"fuse_tail": 0, "merge_kinds": 1}


@pytest.mark.parametrize("opt", ["fuse_tail", "merge_kinds"])
def test_tuning_options_do_not_change_results(gpu_ctx, oracle, opt, launch_by_launch):
    """Launch-structure switches change no result bit: the reduction + GN update inside the
    linearisation launch (fuse_tail: last block to arrive, write-through partials, sharded tickets) against the separate
    k_reduce_partials launch, and one launch for both kinds (merge_kinds) against one launch per kind.  All add the same
    numbers in the same order."""
    room = synth.make_room(seed=24, n_query=8000, n_edge_query=200)
    P = L.make_params("rot")
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(13), 0.15, 1.0)
    res = []
    try:
        for val in (0, 1):
            gpu_ctx.set_option(opt, val)
            m = L.ScanToMapMatcher(gpu_ctx, P)
            gpu_ctx.set_debug(True)
            m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
            m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
            m.set_queries(0, L.KIND_SURF, room["q_xyz"])
            m.set_queries(0, L.KIND_EDGE, room["eq_xyz"])
            m.pose_set(0, t0, q0)
            m.iterate(0, 6, L.MASK_SURF | L.MASK_EDGE)
            t, q, st = m.pose_get(0)
            idx, d2 = m.neighbors(0, L.KIND_SURF, room["q_xyz"].shape[0])
            G, cost, counts = m.linearize(0, t, q, L.MASK_SURF | L.MASK_EDGE)
            res.append((t, q, st, idx, d2, G, counts, cost))
    finally:
        gpu_ctx.set_option(opt, _OPTION_DEFAULTS[opt])
        gpu_ctx.set_debug(False)
    a, b = res
    assert a[2] == b[2] == 0
    inside = a[4][:, 4] < 1.0
    assert inside.sum() > 1000
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[3][inside], b[3][inside]) and np.array_equal(a[4][inside], b[4][inside])
    assert np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6]) and a[7] == b[7]


def test_map_set_begin_end_overlaps_and_equals_blocking_build(gpu_ctx, oracle):
    """A pipeline that rebuilds its local map every keyframe: lili_map_set_begin builds the next index on a side stream while the iterations
    already enqueued keep the current one, lili_map_set_end swaps.  Over six keyframes with different maps (sizes, a focus box on some) the
    poses equal those of the blocking lili_map_set sequence bit for bit — including keyframes whose iterations are still in flight when the
    next build starts and a build that re-uses the buffers of the index retired two keyframes earlier."""
    room = synth.make_room(seed=71, n_query=8000, n_edge_query=300)
    P = L.make_params("rot")
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(29), 0.1, 0.6)
    rng = np.random.default_rng(11)
    n_all = room["map_xyz"].shape[0]
    maps = [np.ascontiguousarray(room["map_xyz"][np.sort(rng.choice(n_all, int(n_all * f), replace=False))]) for f in (1.0, 0.8, 0.9, 0.7, 1.0, 0.85)]
    mask = L.MASK_SURF | L.MASK_EDGE

    def run(pipelined):
        m = L.ScanToMapMatcher(gpu_ctx, P)
        m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
        m.set_queries(0, L.KIND_SURF, room["q_xyz"]); m.set_queries(0, L.KIND_EDGE, room["eq_xyz"])
        poses = []
        m.set_input_cloud(L.KIND_SURF, maps[0])
        for k in range(len(maps)):
            m.map_focus(room["t_true"], 3.0) if k % 2 else m.map_focus(None)      # the hint applies to the NEXT build
            m.pose_set(0, t0, q0)
            m.iterate(0, 12, mask)                                                   # asynchronous: 36 launches in flight
            if k + 1 < len(maps):
                if pipelined:
                    m.set_input_cloud_begin(L.KIND_SURF, maps[k + 1])                # builds while the iterations above run
                    t, q, st = m.pose_get(0)                                         # (blocks on the context's stream only)
                    m.set_input_cloud_end(L.KIND_SURF)
                else:
                    t, q, st = m.pose_get(0)
                    m.set_input_cloud(L.KIND_SURF, maps[k + 1])
            else:
                t, q, st = m.pose_get(0)
            assert st == 0
            poses.append((t.copy(), q.copy()))
        m.map_focus(None)
        return poses

    a, b = run(False), run(True)
    assert len({tuple(np.round(p[0], 9)) for p in a}) > 1                                # different maps give different poses
    for (ta, qa_), (tb_, qb_) in zip(a, b):
        assert np.array_equal(ta, tb_) and np.array_equal(qa_, qb_)
    m = L.ScanToMapMatcher(gpu_ctx, P)
    with pytest.raises(L.LiliError):
        m.set_input_cloud_end(L.KIND_SURF)                                               # nothing pending


def test_linearize_window_equals_per_slot_calls(gpu_ctx, oracle):
    """lili_s2m_linearize_window (one evaluation of the joint window: a Gram per keyframe, one synchronisation) returns what
    lili_s2m_linearize returns slot by slot, bit for bit — Gram, cost, counts — for three keyframes with different scans and poses."""
    import time
    room = synth.make_room(seed=61, n_query=9000, n_edge_query=600)
    P = L.make_params("livox")
    m = L.ScanToMapMatcher(gpu_ctx, P)
    m.set_input_cloud(L.KIND_SURF, np.concatenate([room["map_xyz"], room["map_refl"][:, None]], 1))
    m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    rng = np.random.default_rng(4)
    slots, ts, qs, ta, qa, counts_1 = [0, 2, 5], [], [], [], [], []
    for k, s in enumerate(slots):
        sel = rng.permutation(room["q_xyz"].shape[0])[: 7000 + 500 * k]
        m.set_queries(s, L.KIND_SURF, np.concatenate([room["q_xyz"][sel], room["q_refl"][sel, None]], 1))
        m.set_queries(s, L.KIND_EDGE, room["eq_xyz"][: 400 + 50 * k])
        t, q = synth.perturbed_pose(tb, qb, rng, 0.03, 0.2)
        Q2, T2 = L.api.assoc_transform(t, q, P)
        counts_1.append((m.find_corresponding_surf_features(s, Q2, T2), m.find_corresponding_corner_features(s, Q2, T2)))
        assert counts_1[-1][0] > 1000 and counts_1[-1][1] > 50
        ta.append(t); qa.append(q)
        t2, q2 = synth.perturbed_pose(t, q, rng, 0.01, 0.1)          # evaluated away from the association pose, like an LM trial point
        ts.append(t2); qs.append(q2)
    mask = L.MASK_SURF | L.MASK_EDGE
    single = [m.linearize(s, ts[k], qs[k], mask) for k, s in enumerate(slots)]
    # the association of the window in one call: same counts, and the records it leaves give the same Grams
    assoc = [L.api.assoc_transform(ta[k], qa[k], P) for k in range(len(slots))]
    counts_w = m.associate_window(slots, [a[1] for a in assoc], [a[0] for a in assoc], mask)
    assert counts_w == counts_1
    again = [m.linearize(s, ts[k], qs[k], mask) for k, s in enumerate(slots)]
    for (G1, c1, n1), (G2, c2, n2) in zip(single, again):
        assert np.array_equal(G1, G2) and c1 == c2 and tuple(n1) == tuple(n2)
    batch = m.linearize_window(slots, ts, qs, mask)
    for (G1, c1, n1), (G2, c2, n2) in zip(single, batch):
        assert np.array_equal(G1, G2) and c1 == c2 and tuple(n1) == tuple(n2) and n2[0] > 1000
    t0 = time.perf_counter()
    for _ in range(50):
        for k, s in enumerate(slots):
            m.linearize(s, ts[k], qs[k], mask)
    t1 = time.perf_counter()
    for _ in range(50):
        m.linearize_window(slots, ts, qs, mask)
    t2_ = time.perf_counter()
    print(f"window evaluation: {1e6 * (t1 - t0) / 50:.0f} us with three calls, {1e6 * (t2_ - t1) / 50:.0f} us with one")
    with pytest.raises(L.LiliError):
        m.linearize_window([0, 0], ts[:2], qs[:2], mask)


@pytest.mark.parametrize("variant", ["livox", "frontend"])
def test_association_that_linearises_on_the_fly(gpu_ctx, oracle, variant):
    """Flavours without count scaling run an outer iteration in TWO launches (k_associate_lin: the lane that fitted a plane / line
    computes its residual row from the values in its registers, the wave reduces its 64 rows on the MFMA; then reduce + GN) instead of
    three.  Same rows (computed from the ROUNDED record values), same robust loss; only the partition of the Gram sum differs (one
    partial per 64 queries instead of one per 1024), so the poses agree to ~1e-13 with the three-launch path — and the records the
    launch leaves behind are the same bits."""
    room = synth.make_room(seed=52, n_query=9000, n_edge_query=700, noise=0.005)
    P, PO, m0 = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
    t_ref, q_ref, _, _ = _pose(room, P, variant)
    t0, q0 = synth.perturbed_pose(t_ref, q_ref, np.random.default_rng(23), 0.15, 1.0)
    res = []
    try:
        for mask in ((L.MASK_SURF,) if variant == "frontend" else (L.MASK_SURF | L.MASK_EDGE, L.MASK_SURF)):
            for fuse in (0, 1, 2):          # 2: the fused launch with 256-thread workgroups (large scans)
                gpu_ctx.set_option("fuse_lin", 1 if fuse else 0)
                gpu_ctx.set_option("fuse_lin_block", 256 if fuse == 2 else 0)
                _, _, m = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
                m.pose_set(0, t0, q0)
                m.iterate(0, 8, mask)
                t, q, st = m.pose_get(0)
                # the records of the last association, through the staged linearisation at a FIXED pose: identical bits <=> identical records
                G, cost, counts = m.linearize(0, t0, q0, mask)
                res.append((mask, fuse, t, q, st, G, cost, tuple(counts)))
    finally:
        gpu_ctx.set_option("fuse_lin", 1)
        gpu_ctx.set_option("fuse_lin_block", 0)
    for a, b, c in zip(res[0::3], res[1::3], res[2::3]):
        for o in (b, c):
            assert a[0] == o[0] and a[1] == 0 and o[1] in (1, 2) and a[4] == o[4] == 0
            assert np.abs(a[2] - t0).max() > 1e-3                                        # the iterations moved the pose
            assert np.abs(a[2] - o[2]).max() < 1e-11 and np.abs(a[3] - o[3]).max() < 1e-11
            assert a[7] == o[7] and a[7][0] > 1000
            assert np.abs(a[5] - o[5]).max() <= 1e-9 * np.abs(a[5]).max()              # (poses differ by ~1e-13, so the last association saw ~the same pose)


@pytest.mark.parametrize("flavour", ["rot", "livox"])
def test_super_row_layout_changes_no_result(gpu_ctx, oracle, flavour):
    """The super-row copy of the map (the inner 27-cell block of a query as one run; the shell's side cells as two) is a layout, not an
    algorithm: off, on for the whole map, and on for a focus box that only part of the queries fall into (the others take the
    nine-row walk in the same launch) give bit-identical neighbours, distances, records, Gram and poses — from a pose 0.3 m / 2 deg
    off, where a good part of the queries walks the shell.  Livox flavour: the reflectivity travels with the copy."""
    room = synth.make_room(seed=41, n_query=9000, n_edge_query=300)
    P = L.make_params(flavour)
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(19), 0.3, 2.0)
    rng = np.random.default_rng(7)
    refl = lambda n: rng.uniform(0.0, 0.05, (n, 1)).astype(np.float32)
    smap, emap, sq, eq = room["map_xyz"], room["edge_map_xyz"], room["q_xyz"], room["eq_xyz"]
    if flavour == "livox":
        smap, emap, sq, eq = [np.concatenate([a.astype(np.float32), refl(a.shape[0])], 1) for a in (smap, emap, sq, eq)]
    centre = np.asarray(room["t_true"], np.float64)
    res = []
    try:
        for mode in ("off", "all", "focus"):
            gpu_ctx.set_option("super_rows", 0 if mode == "off" else 1)
            m = L.ScanToMapMatcher(gpu_ctx, P)
            m.map_focus(centre + [1.0, -0.5, 0.0], 2.5) if mode == "focus" else m.map_focus(None)
            gpu_ctx.set_debug(True)
            m.set_input_cloud(L.KIND_SURF, smap)
            m.set_input_cloud(L.KIND_EDGE, emap)
            m.set_queries(0, L.KIND_SURF, sq)
            m.set_queries(0, L.KIND_EDGE, eq)
            m.pose_set(0, t0, q0)
            m.associate_dev(0, L.MASK_SURF | L.MASK_EDGE)
            idx0, d20 = m.neighbors(0, L.KIND_SURF, sq.shape[0])
            m.iterate(0, 6, L.MASK_SURF | L.MASK_EDGE)
            t, q, st = m.pose_get(0)
            idx, d2 = m.neighbors(0, L.KIND_SURF, sq.shape[0])
            eidx, ed2 = m.neighbors(0, L.KIND_EDGE, eq.shape[0])
            G, cost, counts = m.linearize(0, t, q, L.MASK_SURF | L.MASK_EDGE)
            res.append((t, q, st, idx0, d20, idx, d2, eidx, ed2, G, counts, cost))
    finally:
        gpu_ctx.set_option("super_rows", 1)
        gpu_ctx.set_debug(False)
        L.ScanToMapMatcher(gpu_ctx, P).map_focus(None)
    a = res[0]
    assert a[2] == 0 and a[10][0] > 1000
    gate = 1.0
    assert ((a[4][:, 4] >= 0.4) & (a[4][:, 4] < gate)).sum() > 200      # queries whose 5th neighbour lies beyond the inner block: the shell matters
    for b in res[1:]:
        assert b[2] == 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for k in (3, 5, 7):          # neighbour ids / distances of the queries the reference keeps (inside the gate)
            inside = a[k + 1][:, 4] < gate
            assert np.array_equal(a[k][inside], b[k][inside]) and np.array_equal(a[k + 1][inside], b[k + 1][inside])
        assert np.array_equal(a[9], b[9]) and np.array_equal(a[10], b[10]) and a[11] == b[11]


def test_fuse_tail_toggled_between_set_queries_and_iterate(gpu_ctx, oracle, launch_by_launch):
    """the fused tail used to depend on a block size latched at set_queries.  The linearisation block is
    fixed now, so the option may change at any time: toggling it after set_queries, in the middle of a registration, changes
    no bit of the pose, and the fused launch repeated 200 times (tickets re-arm themselves) stays identical."""
    room = synth.make_room(seed=31, n_query=9000, n_edge_query=150)
    P = L.make_params("rot")
    tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
    t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(17), 0.15, 1.0)
    m = L.ScanToMapMatcher(gpu_ctx, P)
    m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
    m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
    mask = L.MASK_SURF | L.MASK_EDGE
    poses = []
    try:
        for pattern in ((1, 1, 1), (0, 0, 0), (0, 1, 0), (1, 0, 1)):
            gpu_ctx.set_option("fuse_tail", pattern[0])
            m.set_queries(0, L.KIND_SURF, room["q_xyz"])
            m.set_queries(0, L.KIND_EDGE, room["eq_xyz"])
            m.pose_set(0, t0, q0)
            m.iterate(0, 2, mask)
            gpu_ctx.set_option("fuse_tail", pattern[1])
            m.iterate(0, 2, mask)
            gpu_ctx.set_option("fuse_tail", pattern[2])
            m.iterate(0, 2, mask)
            poses.append(m.pose_get(0))
        gpu_ctx.set_option("fuse_tail", 1)
        m.pose_set(0, t0, q0)
        m.iterate(0, 6, mask)
        m.iterate_inner(0, 200, mask, want_cost=True)        # 200 fused launches on fixed records
        a = m.pose_get(0)
        gpu_ctx.set_option("fuse_tail", 0)
        m.pose_set(0, t0, q0)
        m.iterate(0, 6, mask)
        m.iterate_inner(0, 200, mask, want_cost=True)
        b = m.pose_get(0)
    finally:
        gpu_ctx.set_option("fuse_tail", 0)
    for t, q, st in poses[1:]:
        assert st == 0 and np.array_equal(t, poses[0][0]) and np.array_equal(q, poses[0][1])
    assert a[2] == b[2] == 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_inner_iterations_equal_host_gauss_newton(gpu_ctx, oracle):
    """lili_s2m_iterate_inner = the reference's ceres::Solve loop shape (fixed correspondences, L/src/BackendFusion.cpp:984-992):
    k device iterations equal k x [lili_s2m_linearize at the current pose -> lili_gn_step_host] on the same records."""
    room = synth.make_room(seed=33, n_query=7000, n_edge_query=250)
    for variant in ("rot", "livox"):
        P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
        tb, qb = L.api.body_pose_from_lidar(room["t_true"], room["q_true"], P)
        t0, q0 = synth.perturbed_pose(tb, qb, np.random.default_rng(19), 0.05, 0.4)
        mask = L.MASK_SURF | L.MASK_EDGE
        m.pose_set(0, t0, q0)
        m.associate_dev(0, mask)
        m.iterate_inner(0, 4, mask, want_cost=True)
        td, qd, st = m.pose_get(0)
        assert st == 0
        t, q = np.array(t0, np.float64), np.array(q0, np.float64)
        for _ in range(4):
            G, cost, counts = m.linearize(0, t, q, mask)
            assert counts[0] > 1000 and counts[1] > 20
            st, t, q, _ = L.api.gn_step_host(G, t, q)
            assert st == 0
        assert np.abs(td - t).max() < 1e-12 and np.abs(qd - q).max() < 1e-12
        assert np.linalg.norm(td - np.asarray(t0)) > 1e-3          # the inner loop did move the pose


def test_livox_flavour_needs_reflectivity_on_queries(gpu_ctx):
    """queries without the auxiliary float used to be matched with reflectivity 0 (|0 - map curvature| weights)."""
    room = synth.make_room(seed=5, n_query=500, n_edge_query=50)
    P = L.make_params("livox")
    m = L.ScanToMapMatcher(gpu_ctx, P)
    m.set_input_cloud(L.KIND_SURF, np.c_[room["map_xyz"], room["map_refl"]])
    m.set_queries(0, L.KIND_SURF, room["q_xyz"])                      # no aux column
    with pytest.raises(L.LiliError):
        m.find_corresponding_surf_features(0, [1.0, 0, 0, 0], [0.0, 0, 0])
    m.set_queries(0, L.KIND_SURF, np.c_[room["q_xyz"], room["q_refl"]])
    assert m.find_corresponding_surf_features(0, room["q_true"], room["t_true"]) > 0


def test_fast_tiers_equal_exact_tiers(gpu_ctx, oracle):
    """The default association uses two fast tiers with exact fall-backs — the 32-bit key selector (Sel5K) and the centred
    normal-equation plane fit.  Forcing the slow tiers (LILI_DEBUG 32768: exact (d2, index) selector; 16384: pivoted
    Householder QR) must give the same neighbours bit for bit and the same records to the f32 rounding of the fit."""
    import os
    room = synth.make_room(seed=21, n_query=8000, n_edge_query=300)
    variant = "livox"
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=True)
    t, q, Q2, T2 = _pose(room, P, variant, np.random.default_rng(4), 0.05, 0.5)
    nq = room["q_xyz"].shape[0]
    out = {}
    old = os.environ.get("LILI_DEBUG")
    try:
        for name, bits in (("fast", 0), ("exact_sel", 32768), ("qr", 16384)):
            os.environ["LILI_DEBUG"] = str(bits)
            n = m.find_corresponding_surf_features(0, Q2, T2)
            idx, d2 = m.neighbors(0, L.KIND_SURF, nq)
            out[name] = (n, idx.copy(), d2.copy(), m.surf_records(0, nq))
    finally:
        if old is None:
            os.environ.pop("LILI_DEBUG", None)
        else:
            os.environ["LILI_DEBUG"] = old
    n0, i0, d0, r0 = out["fast"]
    assert n0 > 3000
    inside = d0[:, 4] < P.kd_max_radius
    n1, i1, d1, r1 = out["exact_sel"]
    assert n1 == n0 and np.array_equal(i0[inside], i1[inside]) and np.array_equal(d0[inside].view(np.uint32), d1[inside].view(np.uint32))
    assert np.array_equal(r0["query_index"], r1["query_index"]) and np.array_equal(r0["n"], r1["n"]) and np.array_equal(r0["score"], r1["score"])
    n2, i2, d2_, r2 = out["qr"]
    assert n2 == n0 and np.array_equal(r0["query_index"], r2["query_index"])
    np.testing.assert_allclose(r0["n"], r2["n"], rtol=2e-7, atol=1e-9)
    np.testing.assert_allclose(r0["d"], r2["d"], rtol=2e-7, atol=1e-9)
    np.testing.assert_allclose(r0["score"], r2["score"], rtol=2e-7)
    assert (r0["n"].view(np.uint32) == r2["n"].view(np.uint32)).mean() > 0.99       # almost always the same f32


def test_sharded_loop_equals_fused_iterations(gpu_ctx, oracle, launch_by_launch):
    """lili_s2m_iterate_sharded (the multi-GPU loop with the collectives enqueued from C) on ONE rank — without collectives and
    with a host callback standing in for ncclAllReduce — gives the pose of the fused single-GPU iterations bit for bit."""
    import ctypes as C
    import torch
    room = synth.make_room(seed=14, n_query=6000, n_edge_query=300)
    variant = "rot"
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=False)
    t, q, Q2, T2 = _pose(room, P, variant, np.random.default_rng(9), 0.05, 0.6)
    m.pose_set(1, t, q)
    m.pose_copy(0, 1)
    m.iterate(0, 4, L.MASK_SURF)
    t_ref, q_ref, st = m.pose_get(0)
    assert st == 0 and np.abs(t_ref - t).max() > 1e-4
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    gram = torch.zeros(L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
    calls = []
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)

    def fake_allreduce(send, recv, count, dtype, op, comm, stream):     # one rank: the sum is the buffer itself
        calls.append((count, dtype, op, send == recv))
        return 0

    cb = CB(fake_allreduce)
    for fn in (None, C.cast(cb, C.c_void_p).value):
        m.pose_copy(0, 1)
        m.iterate_sharded(0, 4, counts.data_ptr(), gram.data_ptr(), fn, None)
        gpu_ctx.sync()
        t2, q2, st = m.pose_get(0)
        assert st == 0 and np.array_equal(t2, t_ref) and np.array_equal(q2, q_ref)
    assert calls == [(2, 2, 0, True), (L.api.GRAM_DOUBLES, 8, 0, True)] * 4          # ncclInt32 counts, ncclFloat64 Gram, ncclSum, in place
    m.pose_copy(0, 1)
    m.iterate_sharded(0, 8, counts.data_ptr(), gram.data_ptr(), None, None, restart_every=4, restart_slot=1)
    gpu_ctx.sync()
    t3, q3, _ = m.pose_get(0)
    assert np.array_equal(t3, t_ref) and np.array_equal(q3, q_ref)                      # two registrations of four iterations


def test_native_rccl_communicator_single_rank(gpu_ctx, oracle, launch_by_launch):
    """lili_om_amd/rccl.py: a one-rank RCCL communicator next to PyTorch's runtime; the sharded loop with the real ncclAllReduce
    enqueued from C reproduces the fused iterations (a sum over one rank is the identity)."""
    import torch
    from lili_om_amd import rccl
    comm = rccl.Communicator(0, 1)
    try:
        x = torch.arange(8, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        comm.all_reduce(x.data_ptr(), 8, rccl.ncclFloat64, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert x.tolist() == list(range(8))
        room = synth.make_room(seed=15, n_query=4000, n_edge_query=200)
        P, PO, m = _setup(gpu_ctx, oracle, "rot", room, with_refl=False)
        t, q, Q2, T2 = _pose(room, P, "rot", np.random.default_rng(10), 0.05, 0.6)
        m.pose_set(1, t, q)
        m.pose_copy(0, 1)
        m.iterate(0, 3, L.MASK_SURF)
        t_ref, q_ref, _ = m.pose_get(0)
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        gram = torch.zeros(L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        m.pose_copy(0, 1)
        m.iterate_sharded(0, 3, counts.data_ptr(), gram.data_ptr(), comm.allreduce_fn, comm.handle)
        gpu_ctx.sync()
        t2, q2, st = m.pose_get(0)
        assert st == 0 and np.array_equal(t2, t_ref) and np.array_equal(q2, q_ref)
    finally:
        comm.close()




@pytest.mark.parametrize("variant", VARIANTS)
def test_iterate_restart_equals_pose_copy_and_iterate(gpu_ctx, oracle, launch_by_launch, variant):
    """lili_s2m_iterate_restart — the loop the headline and configs[2] variant B time — with n_iters not a multiple of restart_every: the pose of
    pose_copy + iterate per registration bit for bit, on the three-launch path (rot) and the fused one (livox, frontend); with time_association
    (events around the association launches, the three-launch path for every flavour) a positive time and the pose of fuse_lin = 0; bad restart
    arguments raise."""
    room = synth.make_room(seed=16, n_query=5000, n_edge_query=300)
    P, PO, m = _setup(gpu_ctx, oracle, variant, room, with_refl=(variant == "livox"))
    t, q, _, _ = _pose(room, P, variant, np.random.default_rng(12), 0.08, 0.8)
    mask = L.MASK_SURF | L.MASK_EDGE
    n_iters, every = 7, 3                                      # registrations of 3, 3 and 1 iterations
    m.pose_set(1, t, q)
    m.pose_set(0, *synth.perturbed_pose(t, q, np.random.default_rng(13), 0.2, 1.0))     # replaced by the first restart
    m.iterate_restart(0, n_iters, every, 1, mask)
    t_r, q_r, st_r = m.pose_get(0)
    ends = []
    for k in range(0, n_iters, every):
        m.pose_copy(0, 1)
        m.iterate(0, min(every, n_iters - k), mask)
        ends.append(m.pose_get(0))
    t_m, q_m, st_m = ends[-1]
    assert st_r == st_m == 0
    assert np.array_equal(t_r, t_m) and np.array_equal(q_r, q_m)
    assert not np.array_equal(ends[0][0], t_m)                 # the last registration is one iteration long: it ends elsewhere than a full one
    try:
        gpu_ctx.set_option("fuse_lin", 0)
        m.iterate_restart(0, n_iters, every, 1, mask)
        t_u, q_u, _ = m.pose_get(0)
        gpu_ctx.set_option("fuse_lin", 1)
        ms = m.iterate_restart(0, n_iters, every, 1, mask, time_association=True)
        t_e, q_e, st_e = m.pose_get(0)
    finally:
        gpu_ctx.set_option("fuse_lin", 1)
    assert ms > 0 and st_e == 0
    assert np.array_equal(t_e, t_u) and np.array_equal(q_e, q_u)
    if variant == "rot":                                       # no fused path for count-scaled flavours: all four runs are one computation
        assert np.array_equal(t_e, t_r) and np.array_equal(q_e, q_r)
    with pytest.raises(L.LiliError):
        m.iterate_restart(0, n_iters, every, 0, mask)          # restart_slot == slot
    with pytest.raises(L.LiliError):
        m.iterate_restart(0, n_iters, -1, 1, mask)
