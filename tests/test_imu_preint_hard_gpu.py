"""IMU pre-integration on the device (lili_imu_preintegrate) on the hard sample streams of tests/preint_hard_cases.py, against the reference's own
header: tests/golden/ref_preint_hard.npz holds what oracle/_ref/libref_imu.so::ref_preintegrate (Preintegration.h compiled unmodified) gives for them.
Nothing here reads the reference or that library.

Comparison (tests/preint_hard_cases.py::compare, shared with tests/test_imu_preint_gpu.py).  delta_p, delta_q, delta_v, sum_dt: the reference's bits.
Jacobian and covariance entry by entry: the kernel keeps the reference's operation order and leaves out only terms with a structurally-zero factor, and
x + 0 y = x for finite y, so the derived expectation is that every entry is EQUAL as a number (==) and that an entry the reference leaves exactly 0 is exactly 0.
tests/test_preint_hard_cases_cpu.py shows that this comparison notices a missing or doubled gyr_w or acc_w term, Rr from the normalised quaternion, 1/6 for
0.1667, a zeroed V(0,9) or V(6,9) and a flipped sign of F(3,12) — two of which the earlier "1e-11 of the largest entry" let pass.

Prediction (predict = 1, lane 64): the bits of tests/preint_model.py::predict from a start rotation that is not quite orthonormal, for every hard case and for
the n = 64 and n = 128 prefixes of two of them (the chunk is 64 samples); the factor's record does not depend on the flag.
Batches: 64 segments of every family in one call — two n = 4096 and one n = 4095 segment each followed by a one-sample segment (first_row 4097, 8196 and
12294), alternating predict flags — and the same in reversed order: every record the bytes of its single call, untouched prediction slots where none was asked.
Determinism: two calls of n = 4096, the same bytes.

Measured on an MI355X, per family: unequal entries (Jacobian + covariance) / worst difference in units of 2^-53 x the largest entry of the 3 x 3 block:
  rates 0 / 0    rates_long_dt 0 / 0    long_dt 0 / 0    dt_mixed 0 / 0    tiny_dt 0 / 0    bias_large 0 / 0    acc_big 0 / 0    still 0 / 0
  gravity_only 0 / 0    one_axis 0 / 0    turns 0 / 0    max 0 / 0
and the state's bits equal in all 22 cases: no difference to explain, the assertion is equality.  The 33 earlier cases (tests/test_imu_preint_gpu.py): 0 / 0.
Prediction: dP, dR, dV = 0 in all 24 (|R1| grows to 41 in rates_long_dt: the product of rotations 16 % off orthonormal).
"""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from tests import preint_hard_cases as HC
from tests import preint_model as M
from tests.test_imu_preint_gpu import G_VEC, _rec, _start_state

pytestmark = pytest.mark.gpu

PREFIXES = (("rates_65", 64), ("dt_mixed", 128))      # prediction at whole chunks: n = 64 and n = 128


@pytest.fixture(scope="module")
def cases():
    return HC.cases()      # (asserts every case's input hash against the fixture)


@pytest.fixture(scope="module")
def pre(gpu_ctx):
    return L.ImuPreintegrator(gpu_ctx)


@pytest.fixture(scope="module")
def singles(pre, cases):
    """every case in a call of its own, without prediction: name -> (state, jacobian, covariance, raw bytes); computed once, never modified"""
    return {c["name"]: _rec(pre.preintegrate([M.segment_of(c)])[0]) for c in cases}


def _prefix(c, n):
    return dict(c, name=f"{c['name']}[:{n}]", n=n, dt=c["dt"][:n].copy(), acc=c["acc"][:n].copy(), gyr=c["gyr"][:n].copy())


@pytest.fixture(scope="module")
def predicted(cases):
    """name -> (case, (P0, R0, V0), (P1, R1, V1) of the plain restatement): the hard cases and the two whole-chunk prefixes; computed once"""
    by_name = {c["name"]: c for c in cases}
    todo = list(cases) + [_prefix(by_name[name], n) for name, n in PREFIXES]
    out = {}
    for k, c in enumerate(todo):
        start = _start_state(100 + k)
        out[c["name"]] = (c, start, M.predict(*start, c["ba"], c["bg"], G_VEC, c["acc0"], c["gyr0"], c["dt"], c["acc"], c["gyr"]))
    return out


def _same_prediction(got, want):
    return all(np.asarray(g, np.float64).tobytes() == w.tobytes() for g, w in zip(got, want))


def test_every_hard_case_against_the_reference_fixture(cases, singles):
    bad, worst = [], {}
    for c in cases:
        state, jac, cov, raw = singles[c["name"]]
        r = HC.compare(state, jac, cov, c)
        print(HC.line(c["name"], r))
        w = worst.setdefault(c["family"], [0, 0.0])
        worst[c["family"]] = [w[0] + r["jacobian"]["unequal"] + r["covariance"]["unequal"], max(w[1], r["jacobian"]["worst"], r["covariance"]["worst"])]
        if not HC.equal(r):
            bad.append((c["name"], r))
        rec = L.api.WindowImu.from_buffer_copy(raw)                # what else the record carries
        assert tuple(rec.g) == G_VEC and np.array_equal(rec.lin_ba, c["ba"]) and np.array_equal(rec.lin_bg, c["bg"])
    for f, (n, u) in worst.items():
        print(f"attained, {f:>14}: {n} unequal entries, worst {u:.3g} units of 2^-53 x block maximum")
    assert not bad, bad


def test_prediction_against_the_plain_restatement(pre, singles, predicted):
    assert {c["n"] for c, _, _ in predicted.values()} >= {1, 64, 65, 128, 129, 4095, 4096}
    for name, (c, (P0, R0, V0), want) in predicted.items():
        assert np.abs(R0 @ R0.T - np.eye(3)).max() > 1e-4                                       # the start rotation is used as it is
        out, preds = pre.preintegrate([M.segment_of(c, P0=P0, R0=R0, V0=V0, g=G_VEC)], predict=True)
        print(f"prediction {name:>16} n {c['n']:4d}: dP {np.abs(preds[0][0] - want[0]).max():.3e} dR {np.abs(preds[0][1] - want[1]).max():.3e} dV {np.abs(preds[0][2] - want[2]).max():.3e}"
              f"  (|R1| up to {np.abs(want[1]).max():.3g})")
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
        assert _same_prediction(preds[0], want), name
        if name in singles:
            assert _rec(out[0])[3] == singles[name][3], name                                 # the factor's record does not depend on the flag


def _batch(pre, order, singles, predicted):
    """one call over the named cases with alternating predict flags, into prediction slots filled with 0x5A"""
    n_seg = len(order)
    segs, rows, first_rows = [], 0, []
    for k, name in enumerate(order):
        c, (P0, R0, V0), want = predicted[name]
        segs.append(M.segment_of(c, P0=P0, R0=R0, V0=V0, g=G_VEC, predict=k % 2 == 1))
        first_rows.append(rows)
        rows += c["n"] + 1
    packed, keep, flags = pre._pack(segs)
    assert flags == [k % 2 == 1 for k in range(n_seg)]
    out = (L.api.WindowImu * n_seg)()
    pred = (L.api.ImuPrediction * n_seg)()
    C.memset(pred, 0x5A, C.sizeof(pred))
    assert pre.lib.lili_imu_preintegrate(pre.ctx.h, packed, n_seg, out, pred) == 0
    for k, name in enumerate(order):
        assert bytes(out[k]) == singles[name][3], (k, name)
        if flags[k]:
            assert _same_prediction((pred[k].P1[:], pred[k].R1[:], pred[k].V1[:]), predicted[name][2]), (k, name)
        else:
            assert bytes(pred[k]) == b"\x5A" * C.sizeof(L.api.ImuPrediction), (k, name)
    return first_rows


def _order(cases):
    rest = [c["name"] for c in cases if c["family"] != "max"]
    order = ["max_4096", "still_1", "max_4096", "still_1", "max_4095", "still_1"]
    return order + [rest[k % len(rest)] for k in range(L.api.IMU_MAX_SEGMENTS - len(order))]


def test_batch_of_every_family(pre, cases, singles, predicted):
    order = _order(cases)
    by_name = {c["name"]: c for c in cases}
    assert len(order) == 64 and {by_name[n]["family"] for n in order} == set(HC.FAMILIES)
    first_rows = _batch(pre, order, singles, predicted)
    assert [first_rows[k] for k in (1, 3, 5)] == [4097, 8196, 12294]                          # the one-sample segments behind the long ones: rows beyond 8000
    assert [by_name[order[k]]["n"] for k in (1, 3, 5)] == [1, 1, 1]


def test_batch_in_reversed_order(pre, cases, singles, predicted):
    _batch(pre, _order(cases)[::-1], singles, predicted)


def test_two_calls_give_the_same_bytes(pre, cases, singles):
    c = next(c for c in cases if c["n"] == 4096)
    assert _rec(pre.preintegrate([M.segment_of(c)])[0])[3] == singles[c["name"]][3]
