"""srpc_frames_unpack_replies without a device: the symbol is exported and in
the ctypes table, its host-side argument checks answer before any device
work, and the client's host frame walk (include/srpc/frame_walk.hpp) holds
under AddressSanitizer / UndefinedBehaviorSanitizer in a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

from srpc_amd import _lib, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["srpc_frames_unpack_replies", "srpc_frames_replies_per_tile"]


def test_symbols_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies"][1]) == 9
    assert re.search(r"#define SRPC_REPLY_NO_CODE 0xFF\b", header) and _lib.SRPC_REPLY_NO_CODE == 0xFF
    assert _lib.lib().srpc_gpu_abi_version() == 8  # an addition within ABI 8


def test_host_side_argument_checks():
    L = _lib.lib()
    cols = (C.c_void_p * 1)(0x1000)
    codes = C.c_void_p(0x2000)
    # a NULL plan
    assert L.srpc_frames_unpack_replies(None, None, 0, None, 0, cols, codes, None, None) == _lib.SRPC_E_INVALID
    # NULL outputs and a stream of 4 GiB are refused before the plan is looked at
    # (the plan here is not one: it must not be read)
    fake = C.create_string_buffer(64)
    plan = C.cast(fake, C.c_void_p)
    assert L.srpc_frames_unpack_replies(plan, None, 0, None, 1, None, codes, None, None) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_unpack_replies(plan, None, 0, None, 1, cols, None, None, None) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_unpack_replies(plan, None, 1 << 32, None, 1, cols, codes, None, None) == _lib.SRPC_E_INVALID
    out = C.c_uint32(77)
    assert L.srpc_frames_replies_per_tile(None, C.byref(out)) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_replies_per_tile(plan, None) == _lib.SRPC_E_INVALID
    assert out.value == 77


def test_frame_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "frame_walk_san")
    cmd = ["g++", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(HERE, "cpp", "frame_walk_test.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0 and "asan" in out.stderr.lower() and "cannot find" in out.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert out.returncode == 0, out.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")  # as tests/test_sanitizers.py
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and " 0 failed" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
