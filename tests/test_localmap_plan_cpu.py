"""The plan of lili_localmap_commit (lili_om_amd/csrc/lili_localmap_plan.h: merge or rebuild, the route, the range of sequence numbers that stays, the keyframes that
come in), checked on the CPU: tests/localmap_plan_check.cpp includes the header alone, runs the named cases and a seeded random sweep over rings of up to 12
keyframes, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_localmap_plan_named_cases_and_sweep(tmp_path):
    exe = tmp_path / "localmap_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "localmap_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "localmap_plan_check: ok" in out.stdout
