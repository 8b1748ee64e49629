"""The owner types of the library's host code (DevBuf, PinBuf, Event, Stream, ExtState), checked on the CPU: tests/own_check.cpp includes the header, stands in for
the runtime calls it uses with counting malloc / free versions, and runs under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_types_free_exactly_what_they_own(tmp_path):
    exe = tmp_path / "own_check"
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                           os.path.join(ROOT, "tests", "own_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "own_check: ok" in out.stdout
