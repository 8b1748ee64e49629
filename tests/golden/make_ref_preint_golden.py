"""Writes tests/golden/ref_preint.npz: inputs and outputs of the reference's Preintegration.h compiled unmodified
(oracle/_ref/libref_imu.so::ref_preintegrate; built by oracle/refshim/Makefile where the reference's sources are present).
Seeds 1..3 of tests/test_window_cpu.py::_samples, one 400-sample stream per seed; the cases are its prefixes of
n in tests/preint_model.py::NS samples (dt[0] = 0 from n = 40 on).

With `hard`: tests/golden/ref_preint_hard.npz instead — the same call on the designed streams of tests/preint_hard_cases.py.  Those regenerate bit for bit
from their seeds, so that file holds per case the outputs (state (11), Jacobian (225), covariance (225)), the masks of their exactly-zero entries and the
SHA-256 of the input bytes, and no inputs.

Recorded numbers only; run from the repository root:

    python tests/golden/make_ref_preint_golden.py [hard]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import preint_hard_cases as HC  # noqa: E402
from tests import preint_model as M  # noqa: E402


def main():
    lib = M.ref_library()
    if lib is None:
        raise SystemExit("oracle/_ref/libref_imu.so is not built")
    streams = M.generate_streams()
    state, jac, cov = [], [], []
    for seed in M.SEEDS:
        s = streams[seed]
        for n in M.NS:
            dt, acc, gyr, acc0, gyr0 = M.case_inputs(s["stream"], n)
            st, J, P = M.ref_preintegrate(lib, dt, acc, gyr, acc0, gyr0, s["ba"], s["bg"])
            state.append(st); jac.append(J.reshape(-1)); cov.append(P.reshape(-1))
    np.savez_compressed(M.GOLDEN, seeds=np.array(M.SEEDS, np.int32), ns=np.array(M.NS, np.int32),
                        dt=np.array([streams[s]["stream"][0] for s in M.SEEDS]), acc=np.array([streams[s]["stream"][1] for s in M.SEEDS]),
                        gyr=np.array([streams[s]["stream"][2] for s in M.SEEDS]), ba=np.array([streams[s]["ba"] for s in M.SEEDS]),
                        bg=np.array([streams[s]["bg"] for s in M.SEEDS]), state=np.array(state), jacobian=np.array(jac), covariance=np.array(cov))
    print(f"{M.GOLDEN}: {os.path.getsize(M.GOLDEN)} bytes, {len(state)} cases")


def main_hard():
    lib = M.ref_library()
    if lib is None:
        raise SystemExit("oracle/_ref/libref_imu.so is not built")
    cases = HC.generate()
    state, jac, cov = [], [], []
    for c in cases:
        st, J, P = M.ref_preintegrate(lib, c["dt"], c["acc"], c["gyr"], c["acc0"], c["gyr0"], c["ba"], c["bg"])
        state.append(st); jac.append(J.reshape(-1)); cov.append(P.reshape(-1))
    jac, cov = np.array(jac), np.array(cov)
    np.savez_compressed(HC.GOLDEN, names=np.array([c["name"] for c in cases]), ns=np.array([c["n"] for c in cases], np.int32), sha256=np.array([c["sha256"] for c in cases]),
                        state=np.array(state), jacobian=jac, covariance=cov, zero_j=jac == 0.0, zero_p=cov == 0.0)
    print(f"{HC.GOLDEN}: {os.path.getsize(HC.GOLDEN)} bytes, {len(state)} cases")


if __name__ == "__main__":
    main_hard() if sys.argv[1:] == ["hard"] else main()
