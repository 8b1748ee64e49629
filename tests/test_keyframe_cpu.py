"""CPU tests of the keyframe hand-over (L/src/LidarOdometry.cpp:565-586, 624-650, 675-680): the numpy model (tests/keyframe_model.py) against what the reference's own
odometry nodes published with if_to_deskew = 1 (tests/golden/ref_keyframe.npz, written by tests/golden/make_ref_keyframe_golden.py), the host helpers of the C ABI
(lili_kf_rule_step, lili_pose_relative) against the nodes' flags and poses and against the model on designed cases, and — where oracle/_ref is built — the live nodes."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from tests import keyframe_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FLAVOURS = ("livox", "rot")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ref_keyframe.npz"))


def stored(gold, flavour):
    """(frame, cloud, rows in (x y z intensity), published xyz, wrong column) of every stored selection"""
    for fr in gold[f"{flavour}/kf_frames"]:
        for name in M.CLOUDS:
            k = f"{flavour}/{int(fr)}/{name}"
            yield int(fr), name, gold[f"{k}/in"], gold[f"{k}/out"], gold[f"{k}/wrong"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model_rows(gold, flavour, fr, rows, **mut):
    """the model on stored rows of frame fr; mut: undistort's mutation switches, or t = another translation, or intensity = another column"""
    if fr == 0:
        return rows[:, :3]                                  # checkInitialization: published as they are
    t = mut.pop("t", gold[f"{flavour}/rel_pose"][fr, 4:])
    inten = mut.pop("intensity", rows[:, 3])
    return M.undistort(rows[:, :3], inten, t, **mut)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_model_equals_the_reference_node(gold, flavour):
    assert list(gold[f"{flavour}/kf_frames"]) == [0, 1, 4] and list(gold[f"{flavour}/kf"]) == [1, 1, 0, 0, 1, 0]
    n_rows = 0
    for fr, name, rows, out, _ in stored(gold, flavour):
        assert rows.shape[0] == out.shape[0] == gold[f"{flavour}/{fr}/{name}/idx"].shape[0]
        got = model_rows(gold, flavour, fr, rows)
        assert (bits(got) == bits(out)).all(), (flavour, fr, name, np.nonzero((bits(got) != bits(out)).any(1))[0][:5])
        n_rows += rows.shape[0]
    assert n_rows > 3000


MUTATIONS = {
    "clamp_removed": lambda g, f, fr, rows, wrong: dict(clamp=False),
    "t_rel_rounded_to_f32": lambda g, f, fr, rows, wrong: dict(t_f32=True),
    "sum_in_f32": lambda g, f, fr, rows, wrong: dict(sum_f32=True),
    "abs_pose_translation": lambda g, f, fr, rows, wrong: dict(t=g[f"{f}/abs_pose"][fr, 4:]),
    "wrong_time_column": lambda g, f, fr, rows, wrong: dict(intensity=wrong),
}
# what the natural data tells apart (measured on the whole clouds when the fixture was written): only the ROT full cloud has rows that clamp beyond rounding of 1
CAUGHT_BY = {"clamp_removed": ("rot",), "t_rel_rounded_to_f32": FLAVOURS, "sum_in_f32": FLAVOURS, "abs_pose_translation": FLAVOURS, "wrong_time_column": FLAVOURS}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_fixture_tells_every_mutation_apart(gold, mutation):
    for flavour in CAUGHT_BY[mutation]:
        wrong_rows = 0
        for fr, name, rows, out, wrong in stored(gold, flavour):
            if fr == 0:
                continue
            got = model_rows(gold, flavour, fr, rows, **MUTATIONS[mutation](gold, flavour, fr, rows, wrong))
            wrong_rows += int((bits(got) != bits(out)).any(1).sum())
        assert wrong_rows >= 1, (mutation, flavour)


def test_selection_holds_the_hard_rows(gold):
    """every stored cloud has its every-16th rows; the clamped rows (ratio > 1) and the rows at ratio 0 are there"""
    n_clamped = n_zero = 0
    for flavour in FLAVOURS:
        for fr, name, rows, out, _ in stored(gold, flavour):
            k = f"{flavour}/{fr}/{name}"
            n, idx = int(gold[f"{k}/n"]), gold[f"{k}/idx"]
            assert set(range(0, n, 16)) <= set(idx.tolist()) and (np.diff(idx) > 0).all() and (idx.size == 0 or idx[-1] < n)
            r = M.ratio_of(rows[:, 3], clamp=False)
            n_clamped += int((r > 1).sum()); n_zero += int((r == 0).sum())
    assert n_clamped >= 24 and n_zero >= 1


def c_rule_flags(poses, matched=None):
    rule = L.api.KeyframeRule()
    return [rule.step(p[4:], p[:4], True if matched is None else matched[i]) for i, p in enumerate(poses)]


def model_rule_flags(poses, matched=None):
    rule = M.Rule()
    return [rule.step(p[4:], p[:4], True if matched is None else matched[i]) for i, p in enumerate(poses)]


def fixture_pose_sets(gold):
    yield "ref_keyframe/livox", gold["livox/abs_pose"], gold["livox/rel_pose"], gold["livox/kf"]
    yield "ref_keyframe/rot", gold["rot/abs_pose"], gold["rot/rel_pose"], gold["rot/kf"]
    for f, pre in (("ref_frontend.npz", ""), ("ref_frontend_R.npz", ""), ("ref_cfg2.npz", "frontendka_")):
        d = np.load(os.path.join(GOLD, f))
        yield f, d[pre + "abs_pose"], d[pre + "rel_pose"], d[pre + "kf"]


def test_rule_reproduces_every_fixture(gold):
    n = 0
    for name, ap, _, kf in fixture_pose_sets(gold):
        flags = c_rule_flags(ap)
        assert flags[0] == M.KF_FIRST, name
        assert [int(f != M.KF_NO) for f in flags] == [int(k) for k in kf], (name, flags, kf)
        assert flags == model_rule_flags(ap), name
        n += 1
    assert n == 5


def _pose(x=0.0, angle=0.0, w=None):
    q = np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)])
    if w is not None:
        q = np.array([w, 0.0, 0.0, 0.0])
    return np.r_[q, x, 0.0, 0.0]


def test_rule_designed_cases():
    I = _pose()
    cases = {
        # standstill: only the `> 2` branch fires — every third frame behind the start-up
        "standstill": ([I] * 12, None),
        # motion of 0.3 m per frame: the `> 1` branch, one frame in between
        "motion": ([_pose(0.3 * k) for k in range(10)], None),
        # rotation alone, 0.15 rad per frame
        "rotation": ([_pose(0.0, 0.15 * k) for k in range(10)], None),
        # w one ulp above 1: ang = 2 acos(w) is NaN and compares false; the distance is 0: behaves like a standstill
        "w_above_one": ([I] + [_pose(w=np.nextafter(1.0, 2.0))] * 9, None),
        # just below both thresholds / just above the distance threshold
        "below": ([_pose(0.19 * (k % 2), 0.09 * (k % 2)) for k in range(10)], None),
        "above": ([_pose(0.2000001 * (k % 2)) for k in range(10)], None),
        # an unmatched frame keeps the flag of the frame before it, whichever it was, and still counts
        "unmatched_keeps_true": ([_pose(0.3 * k) for k in range(8)], [True, True, False, False, True, True, True, True]),
        "unmatched_keeps_false": ([I] * 10, [True, True, True, False, False, False, True, True, True, True]),
        "never_matched": ([I] * 6, [False] * 6),
    }
    for name, (poses, matched) in cases.items():
        got, want = c_rule_flags(poses, matched), model_rule_flags(poses, matched)
        assert got == want, (name, got, want)
        assert got[0] == M.KF_FIRST
    # by hand from L:575 and L:675-676: after a keyframe kf_num = n + 1, so `n - kf_num` runs 0, 1, 2, 3 over the following frames: `> 1` fires at the third, `> 2` at the fourth
    assert c_rule_flags([I] * 10) == [2, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert c_rule_flags([_pose(0.3 * k) for k in range(8)]) == [2, 1, 0, 0, 1, 0, 0, 1]
    assert c_rule_flags([_pose(0.0, 0.15 * k) for k in range(8)]) == [2, 1, 0, 0, 1, 0, 0, 1]
    assert c_rule_flags([I] + [_pose(w=np.nextafter(1.0, 2.0))] * 9) == [2, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert c_rule_flags([_pose(0.19 * (k % 2), 0.09 * (k % 2)) for k in range(10)]) == [2, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert c_rule_flags(*cases["unmatched_keeps_true"])[:4] == [2, 1, 1, 1]
    assert c_rule_flags([I] * 6, [False] * 6) == [2, 1, 1, 1, 1, 1]
    # a reset starts a new sequence
    rule = L.api.KeyframeRule()
    assert [rule.step(I[4:], I[:4]) for _ in range(3)] == [2, 1, 0]
    rule.reset()
    assert rule.flag and [rule.step(I[4:], I[:4]) for _ in range(3)] == [2, 1, 0]


def test_pose_relative_equals_the_nodes(gold):
    n = 0
    for name, ap, rp, _ in fixture_pose_sets(gold):
        for k in range(1, ap.shape[0]):
            t, q = L.api.pose_relative(ap[k - 1, 4:], ap[k - 1, :4], ap[k, 4:], ap[k, :4])
            assert np.r_[q, t].tobytes() == rp[k].tobytes(), (name, k)
            tm, qm = M.pose_relative(ap[k - 1, 4:], ap[k - 1, :4], ap[k, 4:], ap[k, :4])
            assert np.r_[qm, tm].tobytes() == rp[k].tobytes(), (name, k)
            n += 1
    assert n == 25
    # a quaternion that is not unit: inverse() divides by the squared norm
    rng = np.random.default_rng(5)
    for _ in range(50):
        a, b = rng.normal(size=7), rng.normal(size=7)
        t, q = L.api.pose_relative(a[4:], a[:4], b[4:], b[:4])
        tm, qm = M.pose_relative(a[4:], a[:4], b[4:], b[:4])
        assert t.tobytes() == tm.tobytes() and q.tobytes() == qm.tobytes()


def test_rule_state_layout_matches_the_header(tmp_path):
    T = L.api.KfRuleState
    lines = ['printf("%zu\\n", sizeof(lili_kf_rule_state));'] + [f'printf("%zu\\n", offsetof(lili_kf_rule_state, {f}));' for f, _ in T._fields_]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    assert (L.api.KF_NO, L.api.KF_YES, L.api.KF_FIRST) == (M.KF_NO, M.KF_YES, M.KF_FIRST)


def _ref():
    from oracle import ref as R
    return R


def _have_ref():
    try:
        return _ref().available()
    except Exception:      # noqa: BLE001
        return False


@pytest.mark.skipif(not _have_ref(), reason="oracle/_ref is not built (needs the reference sources)")
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_live_node_equals_fixture_and_model_on_standstill(gold, flavour):
    import sys
    sys.path.insert(0, GOLD)
    import make_ref_keyframe_golden as K
    pre = K.inputs(flavour)
    ap, rp, kf, pub = K.run_node(flavour, pre)
    assert ap.tobytes() == gold[f"{flavour}/abs_pose"].tobytes() and rp.tobytes() == gold[f"{flavour}/rel_pose"].tobytes()
    assert [int(k) for k in kf] == list(gold[f"{flavour}/kf"]) and sorted(pub) == list(gold[f"{flavour}/kf_frames"])
    for fr in sorted(pub):
        for name in M.CLOUDS:
            k = f"{flavour}/{fr}/{name}"
            xyz = np.ascontiguousarray(pub[fr][name][:, :3], np.float32)
            assert xyz.shape[0] == int(gold[f"{k}/n"])
            assert hashlib.sha256(xyz.tobytes()).digest() == gold[f"{k}/sha"].tobytes(), k
            assert xyz[gold[f"{k}/idx"]].tobytes() == gold[f"{k}/out"].tobytes(), k
    # standstill: the same scan six times.  Keyframes by the `> 2` branch; the model reproduces every published cloud from the node's own rel_pose
    still = [dict(pre[2], stamp=pre[i]["stamp"]) for i in range(6)]
    ap, rp, kf, pub = K.run_node(flavour, still)
    assert [int(k != M.KF_NO) for k in c_rule_flags(ap)] == [int(k) for k in kf]
    tcol = M.TIME_COL[flavour]
    assert len(pub) >= 3
    for fr in sorted(pub):
        for name, key in (("edge", "edge"), ("surf", "surf"), ("full", "cutted")):
            rows = np.ascontiguousarray(still[fr][key], np.float32)
            want = np.ascontiguousarray(pub[fr][name][:, :3], np.float32)
            got = rows[:, :3] if fr == 0 else M.undistort(rows[:, :3], rows[:, tcol], rp[fr, 4:])
            assert got.tobytes() == want.tobytes(), (flavour, fr, name)
