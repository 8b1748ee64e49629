"""lili_localmap_repose without a GPU: the library exports it and the binding binds it; and, where oracle/_ref is built, the rule the warm-up test
(tests/test_localmap_repose_gpu.py) derives its expected maps from — a FRESH reference slice fed every earlier keyframe with the pose last read for it gives
the map the persistent slice gives — holds when no pose ever changes."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(G, "make_ref_golden.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


def test_library_exports_and_binding_binds_localmap_repose():
    assert "lili_localmap_repose" in L.api.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", L.api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "lili_localmap_repose" for line in out.splitlines() if line.strip())
    assert L.load_library().lili_localmap_repose.argtypes is not None
    assert callable(L.LocalMap.repose) and callable(L.BackendKeyframes.repose)


def test_keyframe_map_poses_is_keyframe_map_pose_per_keyframe():
    rng = np.random.default_rng(4)
    q = rng.normal(size=(5, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-20, 20, (5, 3))
    q_bl = np.array([0.98, 0.05, -0.12, 0.1]); t_bl = np.array([0.05, -0.02, 0.11])
    ts, qs = L.api.keyframe_map_poses(t, q, t_bl, q_bl)
    assert ts.shape == (5, 3) and qs.shape == (5, 4)
    for k in range(5):
        tk, qk = L.api.keyframe_map_pose(t[k], q[k], t_bl, q_bl)
        assert np.array_equal(ts[k], tk) and np.array_equal(qs[k], qk)


@pytest.mark.skipif(not os.path.exists(os.path.join(M.R.REF_DIR, "libref_localmap.so")), reason="oracle/_ref not built (needs /root/reference; build container only)")
def test_fresh_slice_replay_equals_the_persistent_slice():
    i = M.localmap_inputs(n_kf=8)
    W = M.LM_WIDTH
    args = (W, M.LM_SURF_MAP_LEAF, M.LM_EDGE_MAP_LEAF, M.LM_SURF_LEAF, M.LM_EDGE_LEAF, i["q_bl"], i["t_bl"])
    persistent = M.R.LocalMapSlice(*args)
    try:
        for c in range(len(i["surf"])):
            want = persistent.keyframe(i["surf"][c], i["edge"][c])
            persistent.commit(i["poses"][c])
            fresh = M.R.LocalMapSlice(*args)
            try:
                for j in range(c):
                    fresh.keyframe(i["surf"][j], i["edge"][j])
                    fresh.commit(i["poses"][j])      # the pose read at call max(j + 1, min(c, width)): here every call reads the same
                got = fresh.keyframe(i["surf"][c], i["edge"][c])
            finally:
                fresh.close()
            for name in ("surf_map", "edge_map", "surf_ds", "edge_ds"):
                assert np.array_equal(want[name].view(np.uint32), got[name].view(np.uint32)), (c, name)
    finally:
        persistent.close()
