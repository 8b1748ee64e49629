"""tests/cycle_model.py on its own — the referee of lili_window_cycle's write-back (sign unification, gates, q -> R -> q) is checked here against the reference's
text case by case, and its round trip against the restatement lili_om_amd/loop.py already carries — and the layout of the two structures the call adds."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import loop
from tests import cycle_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def row(t=(0.0, 0.0, 0.0), q=(1.0, 0.0, 0.0, 0.0), v=(0.0, 0.0, 0.0), ba=(0.0, 0.0, 0.0), bg=(0.0, 0.0, 0.0)):
    return list(t) + list(q) + list(v) + list(ba) + list(bg)


def bits(values):
    return np.asarray(values, np.float64).tobytes()


SOLVED = row(t=(1.0, 2.0, 3.0), q=(1.0, 0.0, 0.0, 0.0), v=(0.5, -0.5, 0.25), ba=(0.1, 0.2, 0.3), bg=(0.01, 0.02, 0.03))


def shifted(**kw):
    """SOLVED with offsets added per field: the state_in whose move against SOLVED is exactly those offsets"""
    r = list(SOLVED)
    for name, d in kw.items():
        lo = dict(t=0, v=7, ba=10, bg=13)[name]
        for i, x in enumerate(d):
            r[lo + i] = SOLVED[lo + i] + x
    return r


# ---------------------------------------------------------------- the gates, one at a time: below, above, AT the threshold, NaN
@pytest.mark.parametrize("field,bit,sl", [("t", CM.BIT_P, slice(0, 3)), ("v", CM.BIT_V, slice(7, 10))])
def test_norm_gates_on_both_sides_at_and_nan(field, bit, sl):
    # SOLVED's t and v are dyadic, so (6, 8, 0) on top of them is exact and the move's norm is exactly 10
    below, at, above, nan = (shifted(**{field: d}) for d in ((6.0, 7.99, 0.0), (6.0, 8.0, 0.0), (6.0, 8.01, 0.0), (NAN, 0.0, 0.0)))
    assert CM.norm3(at[sl][0] - SOLVED[sl][0], at[sl][1] - SOLVED[sl][1], at[sl][2] - SOLVED[sl][2]) == 10.0
    ab, nx, refused = CM.gate_row(below, SOLVED)
    assert refused == 0 and bits(ab) == bits(SOLVED)
    for name, r_in in (("at", at), ("above", above), ("nan", nan)):
        ab, nx, refused = CM.gate_row(r_in, SOLVED)
        assert refused == bit, (field, name, refused)
        assert bits(ab[sl]) == bits(r_in[sl]) and bits(nx[sl]) == bits(r_in[sl])          # the refused field keeps state_in's values ...
        others = [i for i in range(16) if not sl.start <= i < sl.stop]
        assert bits([ab[i] for i in others]) == bits([SOLVED[i] for i in others])         # ... and nothing else does
    # a gate of the caller's: the same moves against 9.99 and 10.02
    assert CM.gate_row(below, SOLVED, {"gate_p": 9.99, "gate_v": 9.99})[2] == bit
    assert CM.gate_row(above, SOLVED, {"gate_p": 10.02, "gate_v": 10.02})[2] == 0


def test_q_gate_on_both_sides_at_and_nan():
    # solved q = identity: inverse(normalized(q)) is the identity exactly, so dq = q_in and qnorm = |vec(q_in)|; (0.3, 0.4, 0) has norm 0.5 in doubles
    gates = {"gate_q": 0.5}
    solved = list(SOLVED)
    assert CM.norm3(0.3, 0.4, 0.0) == 0.5
    for name, vec, want in (("below", (0.3, 0.399, 0.0), 0), ("at", (0.3, 0.4, 0.0), CM.BIT_Q), ("above", (0.3, 0.401, 0.0), CM.BIT_Q), ("nan", (NAN, 0.0, 0.0), CM.BIT_Q)):
        r_in = list(SOLVED)
        r_in[3:7] = [0.8, *vec]
        ab, nx, refused = CM.gate_row(r_in, solved, gates)
        assert refused == want, (name, refused)
        if want:
            # a refused q gate returns the input q's bytes, in abs_state and in next_state (no round trip)
            assert bits(ab[3:7]) == bits(r_in[3:7]) and bits(nx[3:7]) == bits(r_in[3:7])
        else:
            assert bits(ab[3:7]) == bits(solved[3:7]) and bits(nx[3:7]) == bits(CM.round_trip(CM.normalized(solved[3:7])))
    # with the reference's literal 10 no unit quaternion is ever refused: |vec| <= 1
    r_in = list(SOLVED)
    r_in[3:7] = [0.0, 1.0, 0.0, 0.0]
    assert CM.gate_row(r_in, solved)[2] == 0
    # a NaN or zero SOLVED q is refused too (the documented departure from Eigen's inverse())
    for q in ((NAN, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)):
        s = list(SOLVED)
        s[3:7] = q
        ab, nx, refused = CM.gate_row(SOLVED, s)
        assert refused == CM.BIT_Q and bits(ab[3:7]) == bits(SOLVED[3:7]) and bits(nx[3:7]) == bits(SOLVED[3:7])


@pytest.mark.parametrize("field,bit_of", [("ba", CM.bit_ba), ("bg", CM.bit_bg)])
def test_bias_gates_component_by_component(field, bit_of):
    lo = dict(ba=10, bg=13)[field]
    base = list(SOLVED)
    for i in range(3):
        for name, d, want in (("below", 21.99, 0), ("at", 22.0, bit_of(i)), ("above", 22.01, bit_of(i)), ("below, negative", -21.99, 0), ("above, negative", -22.01, bit_of(i)),
                              ("nan", NAN, bit_of(i))):
            r_in = list(base)
            r_in[lo + i] = d
            solved = list(base)
            solved[lo + i] = 0.0                   # the move is exactly d
            ab, nx, refused = CM.gate_row(r_in, solved)
            assert refused == want, (field, i, name, refused)
            # independence: component i alone keeps (or takes) its value, the five others take the solved ones
            assert bits([ab[lo + i]]) == bits([r_in[lo + i] if want else solved[lo + i]])
            rest = [k for k in range(16) if k != lo + i]
            assert bits([ab[k] for k in rest]) == bits([solved[k] for k in rest]) and bits(nx[:3] + nx[7:]) == bits(ab[:3] + ab[7:])
    # every subset of the six at once
    for mask in range(64):
        r_in, solved, want = list(base), list(base), 0
        for c in range(6):
            if mask >> c & 1:
                r_in[10 + c] = solved[10 + c] + 30.0
                want |= (CM.bit_ba(c) if c < 3 else CM.bit_bg(c - 3))
        ab, _, refused = CM.gate_row(r_in, solved)
        assert refused == want
        assert bits(ab[10:16]) == bits([r_in[10 + c] if mask >> c & 1 else solved[10 + c] for c in range(6)])


def test_bit_layout_is_the_headers():
    assert (CM.BIT_P, CM.BIT_Q, CM.BIT_V) == (1, 2, 4)
    assert [CM.bit_ba(i) for i in range(3)] == [8, 16, 32] and [CM.bit_bg(i) for i in range(3)] == [64, 128, 256]


# ---------------------------------------------------------------- unification
def test_unify():
    q = [-0.5, 0.5, -0.5, 0.5]
    r = CM.unify(row(q=q))
    assert bits(r[3:7]) == bits([0.5, -0.5, 0.5, -0.5])
    for q in ([0.5, 0.5, -0.5, 0.5], [0.0, 1.0, 0.0, 0.0], [-0.0, 1.0, 0.0, 0.0], [NAN, 1.0, 0.0, 0.0]):      # w >= 0, -0.0 and NaN: `< 0` is false, nothing changes
        assert bits(CM.unify(row(q=q))[3:7]) == bits(q)
    solved, ab, nx, refused = CM.apply([SOLVED, SOLVED], [row(q=(-1.0, 0.0, 0.0, 0.0)), row(q=(1.0, 0.0, 0.0, 0.0))])
    assert bits(solved[0][3:7]) == bits([1.0, -0.0, -0.0, -0.0]) and refused == [0, 0]


# ---------------------------------------------------------------- q -> R -> q on every branch of matrix -> quaternion
def _unit(q):
    return CM.normalized([float(v) for v in q])


BRANCH_INPUTS = [("trace", [(1.0, 0.0, 0.0, 0.0), (0.9, 0.1, -0.3, 0.2), (0.6, 0.5, 0.4, -0.3), (0.51, 0.5, 0.5, 0.49)]),
                 (0, [(0.0, 1.0, 0.0, 0.0), (0.02, 0.99, 0.05, -0.03), (0.3, 0.9, 0.2, 0.1)]),
                 (1, [(0.0, 0.0, 1.0, 0.0), (0.02, 0.05, 0.99, -0.03), (0.3, 0.2, 0.9, 0.1)]),
                 (2, [(0.0, 0.0, 0.0, 1.0), (0.02, 0.05, -0.03, 0.99), (0.3, 0.1, 0.2, 0.9)])]


@pytest.mark.parametrize("branch,inputs", BRANCH_INPUTS)
def test_round_trip_on_every_branch_against_loop(branch, inputs):
    for q in inputs:
        qn = _unit(q)
        R = CM.matrix_from_quat(qn)
        assert CM.branch_of(R) == branch, (q, CM.branch_of(R))                  # the input reaches the branch it is here for
        mine = CM.round_trip(qn)
        theirs = loop.quat_from_matrix(loop._matrix_from_quat(np.array(qn)))
        assert bits(np.array(R)) == bits(loop._matrix_from_quat(np.array(qn)))
        assert bits(mine) == bits(theirs), (q, mine, theirs)
        assert max(abs(a - b) for a, b in zip(mine, qn)) < 1e-15 or max(abs(a + b) for a, b in zip(mine, qn)) < 1e-15      # and it is the rotation it started from
    # next_state takes the round trip of the NORMALISED solved q, abs_state the raw one
    s = list(SOLVED)
    s[3:7] = [2.0 * v for v in _unit(inputs[1])]
    s = CM.unify(s)
    ab, nx, refused = CM.gate_row(SOLVED, s)
    assert refused == 0 and bits(ab[3:7]) == bits(s[3:7]) and bits(nx[3:7]) == bits(CM.round_trip(CM.normalized(s[3:7])))


def test_moves_are_what_the_gates_compare():
    r_in = shifted(t=(6.0, 8.0, 0.0), v=(0.0, 3.0, 4.0), ba=(1.0, -2.0, 3.0), bg=(-0.5, 0.25, 0.125))
    m = CM.moves([r_in], [SOLVED])[0]
    assert m["p"] == 10.0 and m["v"] == 5.0 and m["q"] == 0.0
    assert np.allclose(m["ba"], [1.0, 2.0, 3.0], rtol=0, atol=1e-15) and m["bg"] == [0.5, 0.25, 0.125]
    assert math.isnan(CM.moves([row(t=(NAN, 0, 0))], [SOLVED])[0]["p"])


# ---------------------------------------------------------------- the two structures the call adds to the ABI
def test_cycle_struct_mirrors_match_the_header(tmp_path):
    pairs = [("lili_window_cycle_options", L.api.WindowCycleOptions), ("lili_window_cycle_result", L.api.WindowCycleResult), ("lili_window_prior_storage", L.api.WindowPriorStorage)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    src = tmp_path / "lay_cycle.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_cycle"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect, [(i, a, b) for i, (a, b) in enumerate(zip(got, expect)) if a != b]
    o = L.api.WindowCycleOptions()
    assert (o.gate_p, o.gate_q, o.gate_v, o.gate_ba, o.gate_bg, o.use_resident_prior) == (10.0, 10.0, 10.0, 22.0, 22.0, 0)
    assert {"lili_window_cycle", "lili_window_cycle_reset", "lili_window_prior_get", "lili_window_prior_set"} <= set(L.api.exported_symbols())
