"""The contract of a caller's lili_cloud (lili_om_amd/csrc/lili_cloud_source.h: what a description may not be, and where a kernel reads the rows of n clouds
from — in place, through a page-locked buffer's device-side address, or from a staging buffer at offsets of 256 bytes), checked on the CPU:
tests/cloud_source_check.cpp includes the header alone, runs the named cases and a seeded random sweep over up to 8 clouds against the two-pass code the readers
used to repeat, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cloud_source_named_cases_and_sweep(tmp_path):
    exe = tmp_path / "cloud_source_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "cloud_source_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "cloud_source_check: ok" in out.stdout
