"""bench.py as the driver runs it: the JSON contract, the parity self-checks that make a run FAIL (exit status 3) when a GPU-vs-oracle
pose delta exceeds the north star's 1e-4 m / 1e-4 rad, and the multi-rank path (ranks sharing GPU 0: the pool has one GPU per box) with the replica mode
and the lili_p2p mailbox round trip."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _last_json(text):
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError("no JSON line in: " + text[-2000:])


def test_bench_default_run_passes_its_own_parity_checks():
    """python bench.py --gpus 1 --steps 20 --warmup 5 --full — the driver's command with every check: exit status 0, every parity field inside the tolerance."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["metric"].startswith("scan-to-map iterations/s") and d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["value"] > 1000
    assert d["parity_failures"] == []
    pd = d["pose_delta_vs_cpu"]
    assert pd["pass"] and pd["dt_m"] <= 1e-4 and pd["dang_rad"] <= 1e-4 and pd["gn_status"] == 0
    assert d["final_pose"]["gn_status"] == 0
    for key in ("0", "1", "4"):
        c = d["extras"]["configs"][key]
        assert "error" not in c, (key, c)
        assert c["parity"]["pass"] and c["parity"]["dt_m"] <= 1e-4 and c["parity"]["dang_rad"] <= 1e-4, (key, c["parity"])
    assert d["extras"]["configs"]["1"]["frames"] == 100                       # BASELINE configs[1]: the first 100 frames
    rl = d["roofline"]
    assert rl["bound"] == "hbm" and 0 < rl["frac"] < 1 and abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-5
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference")
    seam = d["extras"]["configs"]["4"]["cpp_seam"]
    assert seam.get("window_equals_single_calls_bit_for_bit") is True, seam


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR, twice: only the headline (no roofline, CPU baseline or extras), ms_per_step
    of the 20 timed steps, and the arrays of the last timed step as float32 / float64 .npy under 64 MB — the same bits in both runs."""
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(out)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        d = _last_json(r.stdout)
        assert d["steps"] == 20 and d["warmup"] == 5 and d["unit"] == "iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert abs(d["value"] * d["ms_per_step"] - 1000.0) <= 1e-3 * 1000.0 and d["parity_failures"] == []
        assert "extras" not in d and d["roofline"] is None and d["cpu_baseline"] is None
        files = {f.name[:-4]: np.load(f) for f in sorted(out.glob("*.npy"))}
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert np.array_equal(files["pose_t"], d["final_pose"]["t"]) and np.array_equal(files["pose_q"], d["final_pose"]["q"]) and files["gn_status"][0] == 0
        qi = files["surf_query_index"]
        assert qi.shape[0] > 100000 and np.all(np.diff(qi) > 0) and files["surf_normal"].shape == (qi.shape[0], 3)
        runs.append(files)
    assert runs[0].keys() == runs[1].keys() and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])


@pytest.mark.parametrize("world", [2, 4])
def test_bench_ranks_sharing_one_gpu(world):
    """torch.distributed.run --nproc-per-node N bench.py --gpus N (gloo control plane, all ranks on GPU 0): the strong split through lili_p2p with its
    mailbox round trip, the replica mode without any collective, both bit-identical-pose checks, exit status 0."""
    env = dict(os.environ, LILI_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "20", "--warmup", "10", "--n-map", "500000", "--n-az", "500", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == world and d["scaling"] == "strong" and d["parity_failures"] == []
    mg = d["multi_gpu_check"]
    assert mg["ranks"] == world and mg["final_pose_bit_identical_on_all_ranks"] and mg["max_gn_status"] == 0
    assert mg["p2p_mailbox_round_trip"] is True and d["config"]["collectives"].startswith("lili_p2p")
    assert mg["replicas_final_pose_bit_identical_on_all_ranks"] and mg["replicas_max_gn_status"] == 0
    ex = d["extras"]
    assert ex["replicas_iterations_per_s"] > 0 and ex["weak_scaling_iterations_per_s"] > 0
    # the slot-per-rank window (one keyframe per rank at full size, one gather per iteration): all ranks end with the same bits for every slot
    assert ex.get("window_gather_error") is None, ex.get("window_gather_error")
    assert ex["window_gather_slot_iterations_per_s"] > 0 and ex["window_gather_poses_bit_identical_on_all_ranks"] is True and ex["window_gather_max_gn_status"] == 0
    assert ex["window_gather_dt_truth_m"] < 0.05
