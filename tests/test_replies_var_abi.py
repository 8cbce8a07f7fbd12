"""srpc_frames_unpack_replies_var and its companions without a device: the
symbols are exported, declared and in the ctypes table, the host-side argument
checks answer before the plan is read or any device work is done, and the
host form of the per-frame table (include/srpc/reply_walk.hpp) holds under
AddressSanitizer / UndefinedBehaviorSanitizer in a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

from srpc_amd import _lib, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["srpc_frames_replies_var_scratch_bytes", "srpc_frames_unpack_replies_var", "srpc_frames_replies_var_tile",
       "srpc_frames_frame_var"]


def test_symbols_exported_and_bound():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name in NEW:
        assert name in exported and re.search(rf"\b{name}\s*\(", header), name
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies_var"][1]) == 12
    assert len(_lib.SIGNATURES["srpc_frames_frame_var"][1]) == 7
    assert re.search(r"#define SRPC_GPU_ABI_VERSION 8\b", header)
    assert _lib.lib().srpc_gpu_abi_version() == 8  # additions within ABI 8


def test_host_side_argument_checks():
    L = _lib.lib()
    f = L.srpc_frames_unpack_replies_var
    cols = (C.c_void_p * 1)(0x1000)
    soffs = (C.c_void_p * 1)(0x3000)
    codes, offs, scratch = C.c_void_p(0x2000), C.c_void_p(0x4000), C.c_void_p(0x5000)
    INV = _lib.SRPC_E_INVALID
    assert f(None, None, 0, offs, 1, cols, soffs, codes, None, scratch, 1 << 20, None) == INV
    # NULL arguments and a stream of 4 GiB are refused before the plan is looked
    # at (the plan here is not one: it must not be read)
    fake = C.create_string_buffer(64)
    plan = C.cast(fake, C.c_void_p)
    assert f(plan, None, 0, None, 1, cols, soffs, codes, None, scratch, 1 << 20, None) == INV   # d_offs, n > 0
    assert f(plan, None, 0, offs, 1, None, soffs, codes, None, scratch, 1 << 20, None) == INV   # d_cols
    assert f(plan, None, 0, offs, 1, cols, None, codes, None, scratch, 1 << 20, None) == INV    # d_str_offs
    assert f(plan, None, 0, offs, 1, cols, soffs, None, None, scratch, 1 << 20, None) == INV    # d_codes
    assert f(plan, None, 0, offs, 1, cols, soffs, codes, None, None, 1 << 20, None) == INV      # scratch
    assert f(plan, None, 1 << 32, offs, 1, cols, soffs, codes, None, scratch, 1 << 20, None) == INV
    out = C.c_uint64(77)
    assert L.srpc_frames_replies_var_scratch_bytes(None, 10, C.byref(out)) == INV
    assert L.srpc_frames_replies_var_scratch_bytes(plan, 10, None) == INV
    fr, im = C.c_uint32(78), C.c_uint32(79)
    assert L.srpc_frames_replies_var_tile(None, C.byref(fr), C.byref(im)) == INV
    assert L.srpc_frames_replies_var_tile(plan, None, C.byref(im)) == INV
    assert L.srpc_frames_replies_var_tile(plan, C.byref(fr), None) == INV
    assert (out.value, fr.value, im.value) == (77, 78, 79)
    # frame_var: nothing to do, then NULL arguments
    assert L.srpc_frames_frame_var(None, None, 0, None, 0, None, None) == _lib.SRPC_OK
    assert L.srpc_frames_frame_var(None, offs, 1, codes, 64, None, None) == INV
    assert L.srpc_frames_frame_var(codes, None, 1, codes, 64, None, None) == INV
    assert L.srpc_frames_frame_var(codes, offs, 1, None, 64, None, None) == INV


def test_reply_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "reply_walk_san")
    cmd = ["g++", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(HERE, "cpp", "reply_walk_test.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0 and "asan" in out.stderr.lower() and "cannot find" in out.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert out.returncode == 0, out.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")  # as tests/test_sanitizers.py
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and " 0 failed" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
