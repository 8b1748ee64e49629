"""The LOAM-style (ROT) extractor on the device against the oracle on the cases of tests/rot_cases.py — the branches of k_rot_classify, k_rot_scatter, k_rot_segments,
k_rot_ring and of the second passes (k_rot_voxel_order, k_rot_rank, k_rot_select_big, k_rot_compact) that no synthetic scan reaches.  tests/test_rot_cases_cpu.py
holds, on the oracle alone, that every case is where it claims to be; tests/test_reference_cpu.py that the oracle gives on them what the reference's own
Preprocessing.cpp publishes.  The comparison is the one of tests/test_extract_rot_gpu.py: feature indices, labels, ring table and voxel counts equal, clouds and
curvatures bit for bit."""
import functools

import numpy as np
import pytest

import lili_om_amd as L
from tests import rot_cases as RC
from tests.test_extract_rot_gpu import _compare

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle_of(name, atan_mode=2):
    from oracle import oracle as O
    return RC.run_oracle(O, RC.by_name(name), atan_mode=atan_mode)


def _extractor(ctx, c):
    return L.RotExtractor(ctx, n_scans=c["n_scans"], ds_rate=c["ds_rate"], ds_v=c["ds_v"], near_range=c["near_range"])


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _run(ctx, c, o):
    ex = _extractor(ctx, c)
    g = ex.extract(c["raw"], c["q_imu"], c["q_lb"], debug=True)
    print(c["name"], c["raw"].shape[0], "rows:", g["full"].shape[0], len(g["edge_idx"]), len(g["flat_idx"]), g["surf"].shape[0],
          "oracle", o["full"].shape[0], len(o["edge_idx"]), len(o["flat_idx"]), o["surf"].shape[0])
    _compare(g, o)
    return ex, g


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_every_case_twice(gpu_ctx, oracle, family):
    """Every case under the default options, twice on the same extractor: the second result equals the first (the tags of the look-back words and of the
    seg_final words tell this call's values from the last call's)."""
    cases = RC.cases_of(family)
    assert cases
    for c in cases:
        ex, g = _run(gpu_ctx, c, _oracle_of(c["name"]))
        _same(ex.extract(c["raw"], c["q_imu"], c["q_lb"], debug=True), g)


@pytest.mark.parametrize("fold,wait", [(0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("family", ["borders", "picks", "sizes", "voxels"])
def test_fallback_launches(gpu_ctx, oracle, family, fold, wait):
    """`rot_fold` = 0: the concatenation launch instead of the look-back over the lower rings; `rot_segment_wait` = 0: the border check and the redo in k_rot_ring
    instead of the wait in k_rot_segments — the launches a spin that gave up falls back on, selected outright."""
    gpu_ctx.set_option("rot_fold", fold); gpu_ctx.set_option("rot_segment_wait", wait)
    try:
        for c in RC.cases_of(family):
            _run(gpu_ctx, c, _oracle_of(c["name"]))
    finally:
        gpu_ctx.set_option("rot_fold", 1); gpu_ctx.set_option("rot_segment_wait", 1)


@pytest.mark.parametrize("family", ["sweep", "tables"])
def test_f64_arctangents(gpu_ctx, oracle, family):
    """`rot_atan` = 1 (the f64 functions rounded to f32) against the oracle's mode 1: start / end azimuth, every wrap branch and every ring id boundary."""
    gpu_ctx.set_option("rot_atan", 1)
    try:
        for c in RC.cases_of(family):
            _run(gpu_ctx, c, _oracle_of(c["name"], 1))
    finally:
        gpu_ctx.set_option("rot_atan", 2)


@pytest.mark.parametrize("name", ["sizes_two_trips", "sizes_lds_boundary", "voxels_one_past"])
def test_second_pass_leaves_nothing_behind(gpu_ctx, oracle, name):
    """A scan of more rows than one trip of the histogram sum takes, a scan whose rings lie on both sides of the LDS working set and a scan beyond the packed voxel
    keys, each back to back with an ordinary small scan (and the small scan's own parameters) in one context."""
    big, small = RC.by_name(name), RC.by_name("slerp_identity_qlb")
    for c in (small, big, small, big, small):
        _run(gpu_ctx, c, _oracle_of(c["name"]))


@pytest.mark.parametrize("name", ["sizes_lds_boundary", "voxels_one_past"])
def test_redone_scan_into_page_locked_buffers(gpu_ctx, oracle, name):
    """With page-locked outputs the feature lists are sent early; a scan that needs a second pass sends them again: full, edge and surf equal the pageable result
    (and the oracle's)."""
    c = RC.by_name(name)
    o = _oracle_of(name)
    ex = _extractor(gpu_ctx, c)
    ref = ex.extract(c["raw"], c["q_imu"], c["q_lb"])
    assert np.array_equal(ref["full"].view(np.uint32), o["full"].view(np.uint32))
    assert np.array_equal(ref["edge"].view(np.uint32), o["full"][o["edge_idx"]].view(np.uint32))
    assert np.array_equal(ref["surf"].view(np.uint32), o["surf"].view(np.uint32))
    assert ref["edge"].shape[0] > 10 and ref["surf"].shape[0] > 100
    for _ in range(2):
        got = ex.extract(c["raw"], c["q_imu"], c["q_lb"], reuse=True)
        for k in ("full", "edge", "surf"):
            assert got[k].shape == ref[k].shape and np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
