"""CPU tests of place recognition's host side and of its referee (tests/place_model.py): the comparison-only ring / sector rule against the
paper's atan2 / ceil form, lili_place_layout against the model's tables bit for bit, lili_place_guess against numpy, the ctypes mirrors against the header."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import place as PL
from tests import place_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(n_ring, n_sector, max_radius=80.0, lidar_height=2.0):
    p = PL.default_place_params()
    p.n_ring, p.n_sector, p.max_radius, p.lidar_height = n_ring, n_sector, max_radius, lidar_height
    return p


def test_defaults():
    p = PL.default_place_params()
    assert (p.n_ring, p.n_sector, p.max_radius, p.lidar_height, p.kind) == (20, 60, 80.0, 2.0, L.ARCHIVE_FULL)


@pytest.mark.parametrize("n_ring,n_sector", [(20, 60), (1, 4), (32, 64), (7, 12)])
def test_model_is_the_papers_form_away_from_bin_edges(n_ring, n_sector):
    """random points at least 1e-3 of a bin away from every ring and sector boundary: the comparison rule in f32 and atan2 / ceil in f64 fill the same cells"""
    rng = np.random.default_rng(n_ring * 100 + n_sector)
    n = 4000
    ring = rng.integers(0, n_ring + 1, n)                      # (ring n_ring: beyond max_radius, skipped by both)
    sec = rng.integers(0, n_sector, n)
    r = 80.0 * (ring + rng.uniform(1e-3, 1 - 1e-3, n)) / n_ring
    th = 2 * math.pi * (sec + rng.uniform(1e-3, 1 - 1e-3, n)) / n_sector
    pts = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-3, 8, n)], 1).astype(np.float32)
    a = PM.describe(pts, n_ring, n_sector, 80.0, 2.0)
    b = PM.describe_atan(pts, n_ring, n_sector, 80.0, 2.0)
    assert a.tobytes() == b.tobytes()
    assert np.count_nonzero(a) >= min(n_ring * n_sector, n) // 2


@pytest.mark.parametrize("n_ring,n_sector", [(20, 60), (1, 4), (32, 64), (7, 12)])
def test_layout_equals_the_models_tables(n_ring, n_sector):
    for max_radius in (80.0, 33.3):
        r, c, s = L.place_layout(_params(n_ring, n_sector, max_radius))
        mr, mc, ms = PM.tables(n_ring, n_sector, max_radius)
        assert r.tobytes() == mr.tobytes() and c.tobytes() == mc.tobytes() and s.tobytes() == ms.tobytes()


def test_layout_refuses_bad_parameters():
    lib = L.load_library()
    out = [np.zeros(32, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32)]
    for n_ring, n_sector, rad in [(0, 60, 80.0), (33, 60, 80.0), (20, 0, 80.0), (20, 62, 80.0), (20, 68, 80.0), (20, 60, 0.0), (20, 60, float("nan")), (20, 60, float("inf"))]:
        assert lib.lili_place_layout(C.byref(_params(n_ring, n_sector, rad)), *[L.api._ptr(o) for o in out]) != 0
    p = _params(20, 60)
    p.kind = 3
    assert lib.lili_place_layout(C.byref(p), *[L.api._ptr(o) for o in out]) != 0
    assert not any(o.any() for o in out)


def test_whole_sector_rotation_shifts_the_models_descriptor_exactly():
    rng = np.random.default_rng(5)
    cells = [(int(s), int(r)) for s, r in zip(rng.integers(0, 60, 200), rng.integers(0, 20, 200))]
    pts = PM.bin_centre_points(cells, 20, 60, 80.0, rng)
    d0 = PM.describe(pts, 20, 60, 80.0, 2.0)
    for s in (1, 7, 15, 30, 59):
        a = 2 * math.pi * s / 60
        rot = pts.astype(np.float64) @ np.array([[math.cos(a), math.sin(a), 0], [-math.sin(a), math.cos(a), 0], [0, 0, 1]])
        d = PM.describe(rot.astype(np.float32), 20, 60, 80.0, 2.0)
        assert d.tobytes() == np.roll(d0, s, axis=0).tobytes()
        dist, shift = PM.pair(d0, d)
        assert shift == s and dist <= 1e-12


def test_vectorised_distance_is_the_statement_by_statement_one():
    rng = np.random.default_rng(6)
    for _ in range(20):
        A = (rng.uniform(-1, 8, (60, 20)) * (rng.uniform(size=(60, 20)) < 0.3)).astype(np.float32)
        B = (rng.uniform(-1, 8, (60, 20)) * (rng.uniform(size=(60, 20)) < 0.3)).astype(np.float32)
        A[rng.integers(0, 60, 9)] = 0
        B[rng.integers(0, 60, 9)] = 0
        a, b = PM.shift_distances(A, B), PM.shift_distances_loops(A, B)
        assert np.array_equal(np.isinf(a), np.isinf(b))
        assert np.abs(a[np.isfinite(a)] - b[np.isfinite(b)]).max() <= 1e-14
    assert np.isinf(PM.shift_distances(np.zeros((60, 20), np.float32), B)).all()


def test_guess_against_numpy():
    """three rigid transforms in f64: 1e-12 per entry for |t| <= 1e3 m"""
    rng = np.random.default_rng(7)
    for _ in range(200):
        ts, td = rng.normal(size=3), rng.normal(size=3)
        ps = np.concatenate([ts / np.linalg.norm(ts) * rng.uniform(0, 1e3), rng.normal(size=4)])
        pd = np.concatenate([td / np.linalg.norm(td) * rng.uniform(0, 1e3), rng.normal(size=4)])
        ps[3:] /= np.linalg.norm(ps[3:]) * rng.uniform(0.5, 2.0)      # (quaternions are normalised inside)
        pd[3:] /= np.linalg.norm(pd[3:])
        n_sector = int(rng.choice([4, 12, 60, 64]))
        shift = int(rng.integers(0, n_sector))
        T = L.place_guess(ps, pd, shift, n_sector)
        assert np.abs(T - PM.guess(ps, pd, shift, n_sector)).max() <= 1e-12
    # the convention: the same pose, shift s -> a pure yaw of +s sectors about the LiDAR's own z axis
    T = L.place_guess([0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], 15, 60)
    assert np.allclose(T[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    lib = L.load_library()
    bad, ok, out = np.array([0, 0, 0, 0, 0, 0, 0.0]), np.array([0, 0, 0, 1, 0, 0, 0.0]), np.full(16, 7.0)
    assert lib.lili_place_guess(L.api._ptr(bad), L.api._ptr(ok), 1, 60, L.api._ptr(out)) != 0
    assert lib.lili_place_guess(L.api._ptr(ok), L.api._ptr(ok), 1, 0, L.api._ptr(out)) != 0
    assert (out == 7.0).all()


def test_struct_mirrors_match_the_header(tmp_path):
    pairs = [("lili_place_params", L.api.PlaceParams), ("lili_place_query", L.api.PlaceQuery), ("lili_place_match", L.api.PlaceMatch)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    src = tmp_path / "lay_place.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_place"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect, [(i, a, b) for i, (a, b) in enumerate(zip(got, expect)) if a != b]
