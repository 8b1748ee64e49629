#!/usr/bin/env python
"""Generates tests/golden/ref_keyframe.npz: the keyframe hand-over of the reference's odometry nodes (oracle/_ref/libref_lo.so and libref_lo_R.so, the reference's
LidarOdometry.cpp of both packages compiled as they are) run with if_to_deskew = 1 on the sequences of make_ref_golden.run_frontend() / run_frontend_rot().

Per flavour f in (livox, rot):
  f/kf, f/abs_pose, f/rel_pose                 the node's flag and poses after every frame (qw qx qy qz x y z)
  f/kf_frames                                  the frames whose three clouds were published (0, 1, 4)
  f/<frame>/<cloud>/n, /sha                    row count and sha-256 of the published xyz (float32, row-major), cloud in (edge, surf, full)
  f/<frame>/<cloud>/idx, /in, /out             a selection of rows: their index, the node's INPUT row (x, y, z, intensity) and the published xyz
The selection holds every row on which one of the model's mutations (tests/keyframe_model.py: clamp removed, t_rel rounded to f32, sum in f32, abs_pose's translation,
wrong time column) changes a bit — unless it changes more than a quarter of the cloud, which every 16th row shows anyway: storing those rows would store the whole
cloud —, every row with ratio > 1 or ratio == 0, and every 16th row.  Input row i and published row i correspond (checked here).

Only runs where oracle/_ref exists (the build container).  Run from the repository root:
    python tests/golden/make_ref_keyframe_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_ref_golden as G            # noqa: E402
from oracle import ref as R            # noqa: E402
from tests import keyframe_model as M  # noqa: E402


def inputs(flavour):
    """the three clouds the extraction node hands the odometry node, per frame"""
    if flavour == "livox":
        frames, stamps, imu_t, gyr = G.frontend_inputs()
        return R.run_scans("livox", G.LIVOX_PARAMS, frames, stamps, imu_t, gyr)
    scans, stamps, imu_t, gyr = G.frontend_rot_inputs()
    return R.run_scans("rot", G.ROT_PARAMS, scans, stamps, imu_t, gyr)


def run_node(flavour, pre, deskew=1):
    """-> abs_pose, rel_pose, kf per frame and {frame: {cloud: published rows}}"""
    params = dict(G.FRONTEND_PARAMS if flavour == "livox" else G.FRONTEND_R_PARAMS)
    params["/lidar_odometry/if_to_deskew"] = deskew
    lo = R.LidarOdometry(params, flavour=flavour)
    ap, rp, kf = [], [], []
    for o in pre:
        a, r, k = lo.frame(o["stamp"], o["edge"], o["surf"], o["cutted"])
        ap.append(a); rp.append(r); kf.append(k)
    stamp_frame = {o["stamp"]: i for i, o in enumerate(pre)}
    pub = {}
    for topic, stamp, a in lo.published():
        for name, tp in M.TOPICS.items():
            if topic == tp:
                pub.setdefault(stamp_frame[stamp], {})[name] = a
    lo.close()
    return np.array(ap), np.array(rp), np.array(kf), pub


def mutants(xyz, rows, tcol, t_rel, t_abs):
    """the published xyz under every mutation of the model"""
    inten = rows[:, tcol]
    wrong = rows[:, tcol + 1] if tcol == 8 else rows[:, 3]      # Livox: curvature; ROT: the padding float behind z
    return [M.undistort(xyz, inten, t_rel, clamp=False), M.undistort(xyz, inten, t_rel, t_f32=True), M.undistort(xyz, inten, t_rel, sum_f32=True),
            M.undistort(xyz, inten, t_abs), M.undistort(xyz, wrong, t_rel)]


def build(flavour):
    pre = inputs(flavour)
    ap, rp, kf, pub = run_node(flavour, pre)
    ap0, rp0, kf0, _ = run_node(flavour, pre, deskew=0)
    assert ap.tobytes() == ap0.tobytes() and rp.tobytes() == rp0.tobytes() and (kf == kf0).all(), "deskew changed the poses"
    tcol = M.TIME_COL[flavour]
    d = {f"{flavour}/kf": kf.astype(np.int32), f"{flavour}/abs_pose": ap, f"{flavour}/rel_pose": rp, f"{flavour}/kf_frames": np.array(sorted(pub), np.int32)}
    for fr in sorted(pub):
        for name, key in (("edge", "edge"), ("surf", "surf"), ("full", "cutted")):
            rows_in = np.ascontiguousarray(pre[fr][key], np.float32)
            out = np.ascontiguousarray(pub[fr][name][:, :3], np.float32)
            assert rows_in.shape[0] == out.shape[0], (flavour, fr, name)
            xyz, inten = rows_in[:, :3], rows_in[:, tcol]
            t_rel = rp[fr, 4:] if fr > 0 else np.zeros(3)       # frame 0: checkInitialization publishes the clouds as they are
            model = M.undistort(xyz, inten, t_rel) if fr > 0 else xyz
            assert model.tobytes() == out.tobytes(), (flavour, fr, name, "the model does not reproduce the node")
            sel = np.zeros(out.shape[0], bool)
            sel[::16] = True
            r = M.ratio_of(inten, clamp=False)
            sel |= (r > 1) | (r == 0)
            wrong_rows = []
            if fr > 0:
                for m in mutants(xyz, rows_in, tcol, t_rel, ap[fr, 4:]):
                    bad = (m.view(np.uint32) != out.view(np.uint32)).any(1)
                    wrong_rows.append(int(bad.sum()))
                    if bad.sum() * 4 <= bad.size:      # a mutation that moves most of the cloud (abs_pose's translation, the wrong column) is caught on every 16th row already
                        sel |= bad
            idx = np.nonzero(sel)[0].astype(np.int32)
            k = f"{flavour}/{fr}/{name}"
            d[f"{k}/n"] = np.int32(out.shape[0]); d[f"{k}/sha"] = np.frombuffer(bytes.fromhex(G.sha(out)), np.uint8)
            d[f"{k}/idx"] = idx; d[f"{k}/in"] = np.ascontiguousarray(np.c_[xyz[idx], inten[idx]], np.float32); d[f"{k}/out"] = out[idx]
            d[f"{k}/wrong"] = rows_in[idx, tcol + 1] if tcol == 8 else rows_in[idx, 3]      # the column the "wrong time column" mutation reads
            print(f"{k}: {out.shape[0]} rows, {idx.size} stored, rows a mutation gets wrong (clamp, t f32, sum f32, abs pose, column): {wrong_rows}")
    return d


def main():
    assert R.available(), "oracle/_ref is missing: build it first (python -c 'import __graft_entry__ as g; g.build()')"
    d = {}
    for flavour in ("livox", "rot"):
        d.update(build(flavour))
    path = os.path.join(HERE, "ref_keyframe.npz")
    np.savez_compressed(path + ".tmp.npz", **d)
    os.replace(path + ".tmp.npz", path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
