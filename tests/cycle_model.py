"""Plain-float restatement of what lili_window_cycle does AFTER the solve: the quaternion sign unification (L/src/BackendFusion.cpp:994-1006 with unifyQuaternion,
L/include/utils/math_tools.h:166-173), the write-back gates (L:1187-1284) and the q -> R -> q round trip the next window's start state goes through
(Rs = q.normalized().toRotationMatrix(), then Quaterniond(Rs); Eigen 3.3's two conversions).  Referee of the write-back only: the solve and the prior have
referees of their own (tests/test_window_solve_gpu.py, tests/marg_harness.py).

Every value is a Python float (IEEE binary64), every operation one of + - * / sqrt, each correctly rounded, written in the order the library's header states:
  normalized(q) = q / sqrt(x*x + y*y + z*z + w*w), summed left to right;  inverse(q) = conjugate(q) / (x*x + y*y + z*z + w*w);  Eigen's quaternion product;
  pnorm, vnorm, |vec| = sqrt(d0*d0 + d1*d1 + d2*d2), summed left to right.
One departure from Eigen, on purpose: inverse() returns the zero quaternion when the squared norm is not > 0, which would turn a NaN or zero solved q into
qnorm = 0 and ACCEPT it; here the division is unconditional, so such a q gives a NaN qnorm and is refused.  For a finite non-zero q the two are the same code.
A state row is t[3], q[4] (w x y z), v[3], ba[3], bg[3]."""
import math

DEFAULT_GATES = dict(gate_p=10.0, gate_q=10.0, gate_v=10.0, gate_ba=22.0, gate_bg=22.0)
BIT_P, BIT_Q, BIT_V = 1, 2, 4


def bit_ba(i):
    return 8 << i


def bit_bg(i):
    return 64 << i


def unify(row):
    """tmpQuat with w < 0 negated; -0.0 and NaN are left alone, as `< 0` leaves them"""
    row = [float(v) for v in row]
    if row[3] < 0:
        for i in range(3, 7):
            row[i] = -row[i]
    return row


def normalized(q):
    w, x, y, z = q
    n = _sqrt(((x * x + y * y) + z * z) + w * w)
    return [_div(w, n), _div(x, n), _div(y, n), _div(z, n)]


def _div(a, b):
    """IEEE division: Python raises on a zero divisor where the hardware gives an infinity or a NaN"""
    if b == 0:
        return float("nan") if (a == 0 or a != a) else math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def inverse(q):
    w, x, y, z = q
    n2 = ((x * x + y * y) + z * z) + w * w
    return [_div(w, n2), _div(-x, n2), _div(-y, n2), _div(-z, n2)]


def qmul(a, b):
    return [((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
            ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] + a[2] * b[0]) + a[3] * b[1]) - a[1] * b[3],
            ((a[0] * b[3] + a[3] * b[0]) + a[1] * b[2]) - a[2] * b[1]]


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else float("nan")


def norm3(d0, d1, d2):
    return _sqrt((d0 * d0 + d1 * d1) + d2 * d2)


def matrix_from_quat(q):
    """Eigen 3.3 QuaternionBase::toRotationMatrix (2 (a + b) and 2 a + 2 b are the same double: scaling by two is exact)"""
    w, x, y, z = q
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def branch_of(R):
    """which of the four branches of Eigen 3.3's quaternionbase_assign_impl<Matrix3> a matrix takes: "trace", or the index of the largest diagonal entry"""
    if (R[0][0] + R[1][1]) + R[2][2] > 0:
        return "trace"
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    return i


def quat_from_matrix(R):
    tr = (R[0][0] + R[1][1]) + R[2][2]
    if tr > 0:
        t = _sqrt(tr + 1.0)
        w = 0.5 * t
        t = _div(0.5, t)
        return [w, (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t]
    i = branch_of(R)
    j, k = (i + 1) % 3, (i + 2) % 3
    t = _sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
    q = [0.0, 0.0, 0.0, 0.0]
    q[1 + i] = 0.5 * t
    t = _div(0.5, t)
    q[0] = (R[k][j] - R[j][k]) * t
    q[1 + j] = (R[j][i] + R[i][j]) * t
    q[1 + k] = (R[k][i] + R[i][k]) * t
    return q


def round_trip(q):
    """Quaterniond(q.toRotationMatrix()) of an already normalised q"""
    return quat_from_matrix(matrix_from_quat(q))


def gate_row(row_in, row_solved, gates=None):
    """one keyframe: (abs_state row, next_state row, refused bits) from state_in's row and the UNIFIED solved row"""
    g = dict(DEFAULT_GATES)
    g.update(gates or {})
    a, x = [float(v) for v in row_in], [float(v) for v in row_solved]
    pnorm = norm3(a[0] - x[0], a[1] - x[1], a[2] - x[2])
    vnorm = norm3(a[7] - x[7], a[8] - x[8], a[9] - x[9])
    qn = normalized(x[3:7])
    dq = qmul(inverse(qn), a[3:7])
    qnorm = norm3(dq[1], dq[2], dq[3])
    refused = 0
    if not pnorm < g["gate_p"]:
        refused |= BIT_P
    if not qnorm < g["gate_q"]:
        refused |= BIT_Q
    if not vnorm < g["gate_v"]:
        refused |= BIT_V
    for i in range(3):
        if not abs(a[10 + i] - x[10 + i]) < g["gate_ba"]:
            refused |= bit_ba(i)
        if not abs(a[13 + i] - x[13 + i]) < g["gate_bg"]:
            refused |= bit_bg(i)
    ab = list(x)
    if refused & BIT_P:
        ab[0:3] = a[0:3]
    if refused & BIT_Q:
        ab[3:7] = a[3:7]
    if refused & BIT_V:
        ab[7:10] = a[7:10]
    for i in range(3):
        if refused & bit_ba(i):
            ab[10 + i] = a[10 + i]
        if refused & bit_bg(i):
            ab[13 + i] = a[13 + i]
    nx = list(ab)
    if not refused & BIT_Q:
        nx[3:7] = round_trip(qn)
    return ab, nx, refused


def apply(state_in, solved_raw, gates=None):
    """(solved (unified), abs_state, next_state, refused) of a whole window, rows as lists of floats"""
    solved = [unify(r) for r in solved_raw]
    out = [gate_row(a, x, gates) for a, x in zip(state_in, solved)]
    return solved, [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def moves(state_in, solved):
    """per keyframe (pnorm, qnorm, vnorm, |dba| x 3, |dbg| x 3): what the gates compare with their thresholds"""
    res = []
    for a, x in zip(state_in, solved):
        a, x = [float(v) for v in a], [float(v) for v in x]
        dq = qmul(inverse(normalized(x[3:7])), a[3:7])
        res.append(dict(p=norm3(a[0] - x[0], a[1] - x[1], a[2] - x[2]), q=norm3(dq[1], dq[2], dq[3]), v=norm3(a[7] - x[7], a[8] - x[8], a[9] - x[9]),
                        ba=[abs(a[10 + i] - x[10 + i]) for i in range(3)], bg=[abs(a[13 + i] - x[13 + i]) for i in range(3)]))
    return res
