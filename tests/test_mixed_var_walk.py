"""judge_reply_mixed (include/srpc/mixed_walk.hpp), the host restatement of
the decode's per-frame tables with string plans, row by row and with string
lengths of 2^63 and 2^64 - 1, under AddressSanitizer / UndefinedBehaviorSanitizer
in a stand-alone program: tests/cpp/mixed_var_walk_test.cpp."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def sanitizers_link(tmp_path) -> bool:
    """Does this toolchain link a trivial program with the sanitizers' runtimes?"""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", *SAN, "-o", str(tmp_path / "probe"), str(src)], capture_output=True).returncode == 0


def test_mixed_var_walk_under_asan_ubsan(tmp_path):
    if not sanitizers_link(tmp_path):
        pytest.skip("sanitizer runtime not installed")
    exe = str(tmp_path / "mixed_var_walk_san")
    cmd = ["g++", "-std=c++20", *SAN, "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Wextra",
           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(HERE, "cpp", "mixed_var_walk_test.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr  # with the runtimes present, a failed build is the project's
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")  # as tests/test_mixed_abi.py
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and " 0 failed" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
