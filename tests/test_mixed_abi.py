"""The mixed-batch entry points without a device: the symbols are exported, in
the ctypes table and in the header, still within ABI 8; their host-side
argument checks answer before any plan is read and before any device work; and
the host form of the ranks and of the per-frame judgement
(include/srpc/mixed_walk.hpp) holds under AddressSanitizer /
UndefinedBehaviorSanitizer in a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

from srpc_amd import _lib, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["srpc_frames_mixed_index_bytes", "srpc_frames_mixed_index", "srpc_frames_mixed_ranks",
       "srpc_frames_mixed_tile", "srpc_frames_pack_requests_mixed", "srpc_frames_unpack_replies_mixed"]
INVALID, ALIGN, CAPACITY = _lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_CAPACITY


def test_symbols_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    assert len(_lib.SIGNATURES["srpc_frames_pack_requests_mixed"][1]) == 13
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies_mixed"][1]) == 16
    assert re.search(r"#define SRPC_FRAMES_MIXED_MAX_FIELDS 192\b", header) and _lib.SRPC_FRAMES_MIXED_MAX_FIELDS == 192
    assert _lib.lib().srpc_gpu_abi_version() == 8  # additions within ABI 8


def fake_plans(k=16):
    """Plan pointers that are not plans (zeroed memory would read as a plan with
    no fields, 0xFF bytes as garbage): a call that reads them before refusing
    its arguments shows in its return value or crashes."""
    mem = [C.create_string_buffer(b"\xff" * 64, 64) for _ in range(k)]
    arr = (C.c_void_p * k)(*[C.cast(m, C.c_void_p).value for m in mem])
    return arr, mem


def test_index_argument_checks():
    L = _lib.lib()
    out = C.c_uint64(77)
    assert L.srpc_frames_mixed_index_bytes(100, 0, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_index_bytes(100, 17, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_index_bytes(1 << 32, 4, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_index_bytes(100, 4, None) == INVALID
    assert out.value == 77
    # K + 1 u32 per 256 calls and per 16 such rows, 8-byte aligned, never empty
    for n, k, want in ((0, 1, 8), (1, 1, 16), (256, 4, 40), (257, 4, 64), (50_001, 16, ((196 + 13) * 17 * 4 + 7) // 8 * 8)):
        assert L.srpc_frames_mixed_index_bytes(n, k, C.byref(out)) == 0 and out.value == want
    m, idx, cnt = 0x1000, 0x2000, 0x3000
    assert L.srpc_frames_mixed_index(None, 5, 4, idx, 64, cnt, None, None) == INVALID
    assert L.srpc_frames_mixed_index(m, 5, 4, None, 64, cnt, None, None) == INVALID
    assert L.srpc_frames_mixed_index(m, 5, 4, idx, 64, None, None, None) == INVALID
    assert L.srpc_frames_mixed_index(m, 5, 0, idx, 64, cnt, None, None) == INVALID
    assert L.srpc_frames_mixed_index(m, 5, 17, idx, 64, cnt, None, None) == INVALID
    assert L.srpc_frames_mixed_index(m, 1 << 32, 4, idx, 1 << 40, cnt, None, None) == INVALID
    assert L.srpc_frames_mixed_index(m, 5, 4, idx + 4, 64, cnt, None, None) == ALIGN
    assert L.srpc_frames_mixed_index(m, 257, 4, idx, 63, cnt, None, None) == CAPACITY
    assert L.srpc_frames_mixed_ranks(None, m, 5, 4, 0x4000, None) == INVALID
    assert L.srpc_frames_mixed_ranks(idx, None, 5, 4, 0x4000, None) == INVALID
    assert L.srpc_frames_mixed_ranks(idx, m, 5, 4, None, None) == INVALID
    assert L.srpc_frames_mixed_ranks(idx, m, 5, 17, 0x4000, None) == INVALID
    assert L.srpc_frames_mixed_ranks(idx + 4, m, 5, 4, 0x4000, None) == ALIGN


def test_pack_and_decode_refuse_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    col = (C.c_void_p * 1)(0x1000)
    cols = (C.c_void_p * 16)(*[C.cast(col, C.c_void_p).value] * 16)
    cap = (C.c_uint64 * 16)(*[10] * 16)
    m, idx, out, offs, codes, buf = 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    t = C.c_uint32(77)
    assert L.srpc_frames_mixed_tile(None, 4, C.byref(t)) == INVALID
    assert L.srpc_frames_mixed_tile(plans, 0, C.byref(t)) == INVALID
    assert L.srpc_frames_mixed_tile(plans, 17, C.byref(t)) == INVALID
    assert L.srpc_frames_mixed_tile(plans, 4, None) == INVALID
    assert t.value == 77

    def pack(plans=plans, k=4, cols=cols, cap=cap, m=m, idx=idx, n=5, out=out, out_cap=1 << 20, offs=offs):
        return L.srpc_frames_pack_requests_mixed(plans, k, cols, None, cap, m, idx, n, out, out_cap, offs, None, None)

    assert pack(plans=None) == INVALID
    assert pack(k=0) == INVALID
    assert pack(k=17) == INVALID
    assert pack(cols=None) == INVALID
    assert pack(cap=None) == INVALID
    assert pack(m=None) == INVALID
    assert pack(idx=None) == INVALID
    assert pack(out=None) == INVALID
    assert pack(n=1 << 32, out_cap=1 << 62) == INVALID

    def unpack(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, m=m, idx=idx, n=5, cols=cols, cap=cap,
               codes=codes):
        return L.srpc_frames_unpack_replies_mixed(plans, k, buf, buf_len, offs, nf, m, idx, n, 13, cols, None, cap,
                                                  codes, None, None)

    assert unpack(plans=None) == INVALID
    assert unpack(k=0) == INVALID
    assert unpack(k=17) == INVALID
    assert unpack(cols=None) == INVALID
    assert unpack(cap=None) == INVALID
    assert unpack(codes=None) == INVALID
    assert unpack(m=None) == INVALID
    assert unpack(idx=None) == INVALID
    assert unpack(buf=None) == INVALID
    assert unpack(offs=None) == INVALID       # required with frames: there is no uniform mode
    assert unpack(nf=6) == INVALID            # more frames than calls
    assert unpack(buf_len=1 << 32) == INVALID
    assert unpack(n=1 << 32, nf=3) == INVALID


def test_mixed_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mixed_walk_san")
    cmd = ["g++", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(HERE, "cpp", "mixed_walk_test.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0 and "asan" in out.stderr.lower() and "cannot find" in out.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert out.returncode == 0, out.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")  # as tests/test_sanitizers.py
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and " 0 failed" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
