"""What the association entry points do with state they cannot match against: the host refuses before any launch, with the same message
whichever launch structure the call would have taken, and the context keeps working afterwards.

Entry points: lili_s2m_associate, lili_s2m_associate_dev, lili_s2m_associate_window (two slots), lili_s2m_iterate.  Cases: no queries, no map,
a gate larger than the index was built for, the Livox flavour on a map without the auxiliary float, a map of four points (no error: every
query is rejected).  After each case a correct call on the same context returns the oracle's records (bars of test_s2m_gpu.py:
indices and f32 copies exact, plane-fit fields 3e-7 relative).
"""
import numpy as np
import pytest

import lili_om_amd as L

pytestmark = pytest.mark.gpu

ENTRIES = ["associate", "associate_dev", "associate_window", "iterate"]
N_MAP, N_Q = 2000, 64
UNSET = 7        # a slot that never gets queries


@pytest.fixture(scope="module")
def scene(oracle):
    """A 2 000-point plane (z = 0, 1 cm noise, 5 points per square metre: no fine index), 64 queries on it, the body pose at the origin, and the
    oracle's surf records for them — computed once, read-only."""
    rng = np.random.default_rng(41)
    map_xyz = np.c_[rng.uniform(-10, 10, (N_MAP, 2)), rng.normal(0, 0.01, N_MAP)].astype(np.float32)
    q_xyz = np.c_[rng.uniform(-8, 8, (N_Q, 2)), rng.normal(0, 0.01, N_Q)].astype(np.float32)
    P = L.make_params("rot")
    t, q = np.zeros(3), np.array([1.0, 0, 0, 0])
    Q2, T2 = L.api.assoc_transform(t, q, P)
    rec = oracle.associate_surf(oracle.KdTree(map_xyz), None, q_xyz, None, Q2, T2, oracle.params("rot"))
    assert rec["count"] > N_Q // 2, "the scene must produce correspondences"
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(map_xyz=map_xyz, q_xyz=q_xyz, t=t, q=q, Q2=Q2, T2=T2, rec=rec)


def _call(m, entry, scene, slots=(0, 1)):
    """One call of `entry` on `slots` (the single-slot entries use the first); returns the surf counts the call reports, one per slot used
    (the device-pose entries report none: the count is read from a linearisation of the slot afterwards)."""
    s = scene
    if entry == "associate":
        return [m.find_corresponding_surf_features(slots[0], s["Q2"], s["T2"])]
    if entry == "associate_window":
        return [c[0] for c in m.associate_window(list(slots), [s["T2"]] * 2, [s["Q2"]] * 2, L.MASK_SURF)]
    m.pose_set(slots[0], s["t"], s["q"])
    if entry == "associate_dev":
        m.associate_dev(slots[0], L.MASK_SURF)
    else:
        m.iterate(slots[0], 1, L.MASK_SURF)
    return [int(m.linearize(slots[0], s["t"], s["q"], L.MASK_SURF)[2][0])]


def _check_correct_call(m, entry, scene):
    rec = scene["rec"]
    counts = _call(m, entry, scene)
    print(f"{entry}: counts {counts}, oracle {rec['count']}")
    assert counts == [rec["count"]] * len(counts)
    sel = np.nonzero(rec["valid"])[0]
    for slot in range(len(counts)):
        g = m.surf_records(slot, N_Q)
        assert g["count"] == rec["count"]
        assert np.array_equal(g["query_index"], sel)
        assert np.array_equal(g["cp"], rec["cp"][sel])
        np.testing.assert_allclose(g["n"], rec["n"][sel], rtol=3e-7, atol=1e-9)
        np.testing.assert_allclose(g["d"], rec["d"][sel], rtol=3e-7, atol=1e-9)
        np.testing.assert_allclose(g["score"], rec["score"][sel], rtol=3e-7)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_and_recovery(oracle, scene, entry):
    ctx = L.Context(0)      # a context of its own: "no map" and "no queries" need state no earlier test has touched
    try:
        m = L.ScanToMapMatcher(ctx, L.make_params("rot"))
        for slot in (0, 1):
            m.set_queries(slot, L.KIND_SURF, scene["q_xyz"])
        # no map
        with pytest.raises(L.LiliError, match="map_set first"):
            _call(m, entry, scene)
        m.set_input_cloud(L.KIND_SURF, scene["map_xyz"])
        _check_correct_call(m, entry, scene)
        # no queries (the window: its second slot)
        with pytest.raises(L.LiliError, match="set_queries first"):
            _call(m, entry, scene, slots=(UNSET, 0) if entry != "associate_window" else (0, UNSET))
        _check_correct_call(m, entry, scene)
        # kd_max_radius larger than the index was built for
        wide = L.ScanToMapMatcher(ctx, L.make_params("rot", kd_max_radius=4.0))
        with pytest.raises(L.LiliError, match="gate radius exceeds the radius the map index was built for"):
            _call(wide, entry, scene)
        _check_correct_call(m, entry, scene)
        # Livox flavour, map (and queries) without the auxiliary float
        livox = L.ScanToMapMatcher(ctx, L.make_params("livox"))
        with pytest.raises(L.LiliError, match="Livox variant needs reflectivity"):
            _call(livox, entry, scene)
        _check_correct_call(m, entry, scene)
        # a map of four points: no error, every query rejected
        m.set_input_cloud(L.KIND_SURF, scene["map_xyz"][:4])
        counts = _call(m, entry, scene)
        assert counts == [0] * len(counts)
        for slot in range(len(counts)):
            assert m.surf_records(slot, N_Q)["count"] == 0
        m.set_input_cloud(L.KIND_SURF, scene["map_xyz"])
        _check_correct_call(m, entry, scene)
    finally:
        ctx.close()
