"""Context teardown (lili_ctx_destroy): every lazily created state of a context — matcher slots and map index, voxel filter and keyframe ring, both extractors,
loop closure with its private filter, archive and global map with its private sort, IMU pre-integration and the local pose graph with their timing events — is
touched once at the smallest size its entry point takes, the context is closed, and a second context repeats the round: every call succeeds, both kernel timers
report a positive time, and the second round's outputs are the first round's byte for byte.  A third context created afterwards still works."""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from lili_om_amd.archive import ARCHIVE_FULL
from tests import local_graph_cases as Cs
from tests import preint_model as PM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(7)
    room = synth.make_room(seed=3, n_query=400, n_edge_query=40)
    surf = np.concatenate([room["map_xyz"], room["map_refl"][:, None]], 1).astype(np.float32)
    edge = np.concatenate([room["edge_map_xyz"], np.ones((room["edge_map_xyz"].shape[0], 1))], 1).astype(np.float32)
    dirs, _, _ = synth.spinning_rays(120, synth.hdl64_elevations_deg())
    t = synth.OutdoorScene().raycast(np.array([0.0, 0.0, 1.8]), dirs)
    ok = np.isfinite(t)
    rot_scan = np.concatenate([(dirs * t[:, None])[ok], np.full((int(ok.sum()), 1), 10.0)], 1).astype(np.float32)
    walk = Cs._walk_case("teardown_n1", 41, 1)
    return dict(room=room, surf=surf, edge=edge, rot_scan=rot_scan, livox_scan=synth.make_livox_scan(seed=1),
                vox_small=np.concatenate([rng.uniform(-8, 8, (3000, 3)), rng.uniform(0, 255, (3000, 1))], 1).astype(np.float32),
                vox_large=np.concatenate([rng.uniform(-12, 12, (9000, 3)), rng.uniform(0, 255, (9000, 1))], 1).astype(np.float32),
                kf_surf=[surf[k::24].copy() for k in range(3)], kf_edge=[edge[k::3].copy() for k in range(3)],
                kf_t=np.array([[0.0, 0.0, 0.0], [0.3, 0.1, 0.0], [0.1, -0.2, 0.05]]), kf_q=np.tile([1.0, 0.0, 0.0, 0.0], (3, 1)),
                imu=PM.segment_of(next(c for c in PM.golden_cases() if c["n"] == 40)), walk=walk)


def _match(ctx, i):
    """a map build and a few iterations on a few hundred points"""
    room, P = i["room"], L.make_params("rot")
    m = L.ScanToMapMatcher(ctx, P)
    m.set_input_cloud(L.KIND_SURF, room["map_xyz"])
    m.set_queries(0, L.KIND_SURF, room["q_xyz"])
    m.pose_set(0, *L.api.body_pose_from_lidar(room["t_true"] + 0.05, room["q_true"], P))
    m.iterate(0, 3, L.MASK_SURF)
    t, q, status = m.pose_get(0)
    return [t.tobytes(), q.tobytes(), status]


def _round(ctx, i):
    out = _match(ctx, i)
    for pts in (i["vox_small"], i["vox_large"]):                     # the single-launch filter (<= 8192 points) and the general chain
        cen, cnt = L.api.voxel_filter(ctx, pts, 0.4)
        assert 0 < cen.shape[0] < pts.shape[0]
        out += [cen.tobytes(), cnt.tobytes()]
    lm = L.LocalMap(ctx, L.KIND_SURF, width=2, leaf=0.4)
    for k in range(3):                                               # the third push pops the first keyframe into the pool
        lm.push(i["kf_surf"][k], i["kf_t"][k], i["kf_q"][k])
    n_raw, n_map = lm.commit()
    assert n_raw == i["kf_surf"][1].shape[0] + i["kf_surf"][2].shape[0] and 0 < n_map <= n_raw
    out.append(lm.get(n_map).tobytes())
    rot = L.RotExtractor(ctx, n_scans=64, ds_rate=1).extract(i["rot_scan"])
    assert rot["full"].shape[0] > 1000 and rot["surf"].shape[0] > 0
    out += [rot[k].tobytes() for k in ("full", "edge", "surf")]
    lv = L.LivoxExtractor(ctx).extract(i["livox_scan"])
    assert lv["cutted"].shape[0] > 0
    out += [lv[k].tobytes() for k in ("cutted", "edge", "surf")]
    lc = L.LoopClosure(ctx, lc_map_width=1, leaf=0.4)
    (src_raw, src_ds), (tgt_raw, tgt_ds) = lc.assemble(2, 0, i["kf_t"], i["kf_q"], i["kf_edge"], i["kf_surf"])
    assert 0 < src_ds <= src_raw < 1000 and 0 < tgt_ds <= tgt_raw < 1000
    res = lc.align()
    out += [lc.get_cloud(0).tobytes(), lc.get_cloud(1).tobytes(), res["transform"].tobytes(), res["iterations"], np.float64(res["fitness"]).tobytes()]
    arch = L.KeyframeArchive(ctx)
    assert arch.push(i["kf_edge"][0], i["kf_surf"][0], i["kf_surf"][1], 1.0, i["kf_t"][1], i["kf_q"][1]) == 0
    gm = L.GlobalMap(arch)
    n_raw, n_map = gm.build(ARCHIVE_FULL, 1, 0.3)
    assert n_raw == i["kf_surf"][1].shape[0] and 0 < n_map <= n_raw
    cen, cnt = gm.get()
    out += [arch.get(0, ARCHIVE_FULL).tobytes(), cen.tobytes(), cnt.tobytes()]
    ctx.set_option("imu_time", 1)
    pre = L.ImuPreintegrator(ctx)
    out.append(bytes(pre.preintegrate([i["imu"]])[0]))
    assert pre.kernel_ms() > 0.0
    ctx.set_option("local_graph_time", 1)
    lg, w = L.LocalGraph(ctx), Cs.walk_kwargs(i["walk"])
    _, (P_end, _, _), _ = lg.propagate(**w)
    poses, meas, summary = lg.run(np.concatenate([P_end, w["left"][3:7]]), **w)
    assert poses.shape == (1, 7)
    assert lg.kernel_ms() > 0.0
    out += [poses.tobytes(), meas.tobytes(), repr(summary)]
    return out


def test_two_full_contexts_and_a_third(inputs):
    rounds = []
    for _ in range(2):
        ctx = L.Context(0)
        try:
            rounds.append(_round(ctx, inputs))
        finally:
            ctx.close()
    assert len(rounds[0]) == len(rounds[1]) > 20
    assert [k for k, (a, b) in enumerate(zip(*rounds)) if a != b] == []
    ctx = L.Context(0)
    try:
        assert _match(ctx, inputs) == rounds[0][:3]
    finally:
        ctx.close()
