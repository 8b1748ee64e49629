"""What the entry points BELOW the association do with state or arguments they cannot work on — linearisation, the window and multi-rank
calls, the iterate loops, the LM launches: the host refuses, the context's stream and the slots' books stay as they were, and a correct call
afterwards gives the oracle's result.  The companion of test_assoc_errors_gpu.py (same plane scene, plus a handful of edge queries on a
200-point line so that both kinds exist).  Every case is a host-side refusal or a correct call; single rank (allreduce_fn = None).

Also: the same record whichever entry point is asked for it, and kinds that are absent (no queries) from a slot.

Refusals that the iterate_window_sharded / iterate_window_gather loops used to reach only after their first launches (a bad entry in the
slot list was checked slot by slot inside the iteration) are marked HOISTED below: the code is LILI_E_ARG before and after, only the moment
differs.
"""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth

pytestmark = pytest.mark.gpu

N_MAP, N_Q, N_LINE, N_EQ = 2000, 64, 200, 6
BOTH = L.MASK_SURF | L.MASK_EDGE
SLOTS = [0, 1]
BAD_LISTS = [[0, 0], [0, L.api.MAX_SLOTS]]
E_ARG = r"lili error -1:"


@pytest.fixture(scope="module")
def scene(oracle):
    """The plane scene of test_assoc_errors_gpu.py with its oracle records, and an edge map (200 points on a line, 1 mm noise) with six
    edge queries next to it.  Computed once, read-only."""
    rng = np.random.default_rng(41)
    map_xyz = np.c_[rng.uniform(-10, 10, (N_MAP, 2)), rng.normal(0, 0.01, N_MAP)].astype(np.float32)
    q_xyz = np.c_[rng.uniform(-8, 8, (N_Q, 2)), rng.normal(0, 0.01, N_Q)].astype(np.float32)
    line = np.c_[np.linspace(-10, 10, N_LINE), rng.normal(0, 0.001, N_LINE), 1.0 + rng.normal(0, 0.001, N_LINE)].astype(np.float32)
    P = L.make_params("rot")
    t, q = np.zeros(3), np.array([1.0, 0, 0, 0])
    Q2, T2 = L.api.assoc_transform(t, q, P)
    # the edge queries in the frame the association transform maps onto the line (the plane scene is symmetric under it, a line is not)
    eq_map = np.c_[rng.uniform(-8, 8, N_EQ), rng.normal(0, 0.01, N_EQ), 1.0 + rng.normal(0, 0.01, N_EQ)]
    eq_xyz = synth.quat_rot(Q2 * np.array([1.0, -1, -1, -1]), eq_map - T2).astype(np.float32)
    rec = oracle.associate_surf(oracle.KdTree(map_xyz), None, q_xyz, None, Q2, T2, oracle.params("rot"))
    assert rec["count"] > N_Q // 2, "the scene must produce correspondences"
    # a second body pose for slot 1, close enough that its queries still match
    t1 = np.array([0.02, -0.01, 0.005])
    q1 = np.array([1.0, 0.0005, -0.0005, 0.001]); q1 /= np.linalg.norm(q1)
    Q2b, T2b = L.api.assoc_transform(t1, q1, P)
    for a in (map_xyz, q_xyz, line, eq_xyz):
        a.setflags(write=False)
    return dict(map_xyz=map_xyz, q_xyz=q_xyz, line=line, eq_xyz=eq_xyz, ts=[t, t1], qs=[q, q1], Ts=[T2, T2b], Qs=[Q2, Q2b], count=rec["count"])


class Rig:
    pass


@pytest.fixture(scope="module")
def rig(scene):
    """A context of its own (slots 0 and 1 start without queries or records), both maps set, and the two small device buffers the multi-rank
    entry points write."""
    import torch
    r = Rig()
    r.ctx = L.Context(0)
    try:
        r.m = L.ScanToMapMatcher(r.ctx, L.make_params("rot"))
        r.m.set_input_cloud(L.KIND_SURF, scene["map_xyz"])
        r.m.set_input_cloud(L.KIND_EDGE, scene["line"])
        r.counts = torch.zeros(2 * L.api.MAX_SLOTS, dtype=torch.int32, device="cuda")
        r.gram = torch.zeros(L.api.MAX_SLOTS * L.api.GRAM_DOUBLES, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        r.d_counts, r.d_gram = r.counts.data_ptr(), r.gram.data_ptr()
        yield r
    finally:
        r.ctx.close()


def _set_queries(m, scene, surf=(True, True), edge=(True, True)):
    """Queries on slots 0 and 1 (an empty cloud where the flag is off): the slots have no records afterwards."""
    for slot in SLOTS:
        m.set_queries(slot, L.KIND_SURF, scene["q_xyz"] if surf[slot] else np.zeros((0, 3), np.float32))
        m.set_queries(slot, L.KIND_EDGE, scene["eq_xyz"] if edge[slot] else np.zeros((0, 3), np.float32))


def _associate(m, scene):
    """Both slots associated at their poses, which are also the slots' device poses (what the *_dev and iterate entry points read)."""
    for slot in SLOTS:
        m.pose_set(slot, scene["ts"][slot], scene["qs"][slot])
    return m.associate_window(SLOTS, scene["Ts"], scene["Qs"], BOTH)


def _recovers(m, scene):
    """A correct associate_window + linearize gives the oracle's surf count: the context's stream is the main one again, the books are whole."""
    _set_queries(m, scene)
    counts = _associate(m, scene)
    G, cost, c = m.linearize(0, scene["ts"][0], scene["qs"][0], L.MASK_SURF)
    print(f"recovery: window counts {counts}, linearize counts {c}, oracle {scene['count']}")
    assert counts[0][0] == scene["count"] and int(c[0]) == scene["count"]
    assert np.isfinite(G).all() and cost > 0


def _calls(r, scene):
    """name -> f(slots, kind_mask): one call of the entry point on the slot list (the single-slot entries use its first slot)."""
    m, ts, qs = r.m, scene["ts"], scene["qs"]
    own = lambda s: [0] * len(s)
    return {
        "linearize": lambda s, k: m.linearize(s[0], ts[0], qs[0], k),
        "linearize_dev": lambda s, k: m.linearize_dev(s[0], r.d_gram, k),
        "iterate_inner": lambda s, k: m.iterate_inner(s[0], 1, k),
        "solve_lm": lambda s, k: m.solve_lm(s[0], k),
        "solve_lm_window": lambda s, k: m.solve_lm_window(s, k),
        "linearize_window": lambda s, k: m.linearize_window(s, ts[:len(s)], qs[:len(s)], k),
        "linearize_window_sharded": lambda s, k: m.linearize_window_sharded(s, ts[:len(s)], qs[:len(s)], r.d_gram, kind_mask=k),
        "counts_window_sharded": lambda s, k: m.counts_window_sharded(s, r.d_counts, kind_mask=k),
        "linearize_window_gather": lambda s, k: m.linearize_window_gather(s, own(s), 0, r.d_gram, kind_mask=k),
        "iterate_window": lambda s, k: m.iterate_window(s, 1, k),
        "iterate_window_sharded": lambda s, k: m.iterate_window_sharded(s, 1, r.d_counts, r.d_gram, kind_mask=k),
        "iterate_window_gather": lambda s, k: m.iterate_window_gather(s, 1, own(s), 0, r.d_gram, kind_mask=k),
    }


# the tail of the message; the slot-per-rank window words it for the ranks that own nothing ("associate the owned keyframes first")
ASSOCIATE_FIRST = {
    "linearize": "associate first", "linearize_dev": "associate first", "iterate_inner": "associate first", "solve_lm": "associate first",
    "solve_lm_window": "associate first", "linearize_window": "associate first", "linearize_window_sharded": "associate first",
    "counts_window_sharded": "associate first", "linearize_window_gather": "associate the owned keyframes first",
}


@pytest.mark.parametrize("entry", list(ASSOCIATE_FIRST))
def test_associate_first(rig, scene, entry):
    _set_queries(rig.m, scene)          # queries and a map, no association
    with pytest.raises(L.LiliError, match=ASSOCIATE_FIRST[entry] + "$"):
        _calls(rig, scene)[entry](SLOTS, BOTH)
    _recovers(rig.m, scene)


# HOISTED: the last two checked each slot inside the iteration, after the association of the slots before it had been launched (and, for a
# duplicate, after every association of the iteration: the window call behind them refused it).  LILI_E_ARG either way.
@pytest.mark.parametrize("entry", ["linearize_window_sharded", "solve_lm_window", "iterate_window", "linearize_window_gather",
                                   "iterate_window_sharded", "iterate_window_gather"])
@pytest.mark.parametrize("slots", BAD_LISTS, ids=["duplicate", "out_of_range"])
def test_bad_slot_lists(rig, scene, entry, slots):
    _set_queries(rig.m, scene)
    _associate(rig.m, scene)
    with pytest.raises(L.LiliError, match=E_ARG):
        _calls(rig, scene)[entry](slots, BOTH)
    rig.ctx.sync()
    _recovers(rig.m, scene)


@pytest.mark.parametrize("entry", ["linearize", "linearize_dev", "linearize_window", "solve_lm", "linearize_window_gather"])
@pytest.mark.parametrize("mask", [0, 4])
def test_bad_kind_masks(rig, scene, entry, mask):
    _set_queries(rig.m, scene)
    _associate(rig.m, scene)
    with pytest.raises(L.LiliError, match=E_ARG):
        _calls(rig, scene)[entry](SLOTS, mask)
    _recovers(rig.m, scene)


@pytest.mark.parametrize("entry", ["iterate_restart", "iterate_sharded"])
def test_bad_restart_arguments(rig, scene, entry):
    m = rig.m
    _set_queries(m, scene)
    with pytest.raises(L.LiliError, match="bad restart arguments$"):
        if entry == "iterate_restart":
            m.iterate_restart(0, 4, 2, 0, BOTH)
        else:
            m.iterate_sharded(0, 4, rig.d_counts, rig.d_gram, None, None, restart_every=2, restart_slot=0, kind_mask=BOTH)
    _recovers(m, scene)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(np.asarray(a[2]), np.asarray(b[2]))


def test_same_record_from_every_entry_point(rig, scene):
    m, ts, qs = rig.m, scene["ts"], scene["qs"]
    _set_queries(m, scene)
    counts = _associate(m, scene)
    print("association counts", counts)
    assert all(c[0] > 0 and c[1] > 0 for c in counts), "both kinds must have correspondences on both slots"
    one = [m.linearize(s, ts[s], qs[s], BOTH) for s in SLOTS]
    assert not np.array_equal(one[0][0], one[1][0]), "the two slots are linearised at different poses"
    for s in SLOTS:
        assert tuple(int(c) for c in one[s][2]) == counts[s]
    got = {
        "linearize_window": m.linearize_window(SLOTS, ts, qs, BOTH),
        "linearize_window_sharded": m.linearize_window_sharded(SLOTS, ts, qs, rig.d_gram, kind_mask=BOTH),
        "linearize_window_gather_at": m.linearize_window_gather_at(SLOTS, ts, qs, [0, 0], 0, rig.d_gram, kind_mask=BOTH),     # (-0.0 -> +0.0: equal)
    }
    for name, recs in got.items():
        for s in SLOTS:
            print(name, s, "cost", recs[s][1], "counts", recs[s][2], "max |dG|", np.abs(recs[s][0] - one[s][0]).max())
            assert _same(recs[s], one[s]), f"{name}, slot {s}"


def test_absent_kinds(rig, scene):
    m, ts, qs = rig.m, scene["ts"], scene["qs"]
    # slot 0: surf queries, an empty edge cloud; slot 1 full
    _set_queries(m, scene, edge=(False, True))
    _associate(m, scene)
    both, surf = m.linearize(0, ts[0], qs[0], BOTH), m.linearize(0, ts[0], qs[0], L.MASK_SURF)
    assert int(surf[2][0]) == scene["count"] and int(both[2][1]) == 0
    assert _same(both, surf)
    w_both, w_surf = m.linearize_window(SLOTS, ts, qs, BOTH), m.linearize_window(SLOTS, ts, qs, L.MASK_SURF)
    assert _same(w_both[0], w_surf[0]) and _same(w_both[0], surf)
    assert _same(w_both[1], m.linearize(1, ts[1], qs[1], BOTH))
    # slot 0: both kinds empty
    _set_queries(m, scene, surf=(False, True), edge=(False, True))
    _associate(m, scene)
    G, cost, c = m.linearize(0, ts[0], qs[0], BOTH)
    assert not G.any() and cost == 0 and list(c) == [0, 0]
    w = m.linearize_window(SLOTS, ts, qs, BOTH)
    assert not w[0][0].any() and w[0][1] == 0 and tuple(w[0][2]) == (0, 0)
    assert _same(w[1], m.linearize(1, ts[1], qs[1], BOTH))
    with pytest.raises(L.LiliError, match="no records$"):
        m.solve_lm(0, BOTH)
    _recovers(m, scene)
