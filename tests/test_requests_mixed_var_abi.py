"""srpc_frames_unpack_requests_mixed_var without a device: the symbol is
exported, in the ctypes table and in the header, still within ABI 8, and its
host-side argument checks answer before any plan is read and before any device
work.  The refusals that need real plans (SRPC_E_UNSUPPORTED, _ALIGN, _CAPACITY,
and their order) are in tests/test_gpu_requests_mixed_var.py: a plan cannot be
created without a device."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build

from tests.test_mixed_abi import fake_plans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "srpc_frames_unpack_requests_mixed_var"
INVALID = _lib.SRPC_E_INVALID


def test_symbol_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    assert NAME in exported and NAME in _lib.SIGNATURES and re.search(rf"\b{NAME}\s*\(", header)
    assert len(_lib.SIGNATURES[NAME][1]) == 20
    assert _lib.lib().srpc_gpu_abi_version() == 8  # an addition within ABI 8
    assert re.search(r"#define SRPC_GPU_ABI_VERSION 8\b", header)
    # the measurement hook's comment lists the call
    hook = header[header.index("Measurement hook"):header.index("int srpc_time_next_call")]
    assert "_unpack_requests_mixed_var" in hook


def test_arguments_are_refused_before_a_plan_is_read():
    L = _lib.lib()
    plans, _keep = fake_plans()  # reading one of these as a plan shows in the return value or crashes
    col = (C.c_void_p * 1)(0x1000)
    cols = (C.c_void_p * 16)(*[C.cast(col, C.c_void_p).value] * 16)
    so = (C.c_void_p * 16)(*[C.cast(col, C.c_void_p).value] * 16)
    one = (C.c_uint64 * 1)(100)
    scap = (C.c_void_p * 16)(*[C.cast(one, C.c_void_p).value] * 16)
    cap = (C.c_uint64 * 16)(*[10] * 16)
    buf, offs, cls, idx, cnt, ends, scr = 0x7000, 0x5000, 0x2000, 0x3000, 0x4000, 0x6000, 0x8000

    def call(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, cols=cols, so=so, scap=scap, cap=cap, cls=cls,
             idx=idx, idx_bytes=1 << 20, cnt=cnt, ends=ends, scr=scr, scr_bytes=1 << 20):
        return L.srpc_frames_unpack_requests_mixed_var(plans, k, buf, buf_len, offs, nf, cols, so, scap, None, cap, cls,
                                                       idx, idx_bytes, cnt, ends, None, scr, scr_bytes, None)

    for name in ("plans", "cols", "so", "scap", "cap", "idx", "cnt", "ends", "scr"):
        assert call(**{name: None}) == INVALID, name
    for name in ("buf", "offs", "cls"):  # required when there are frames
        assert call(**{name: None}) == INVALID, name
    assert call(k=0) == INVALID
    assert call(k=-1) == INVALID
    assert call(k=17) == INVALID
    assert call(buf_len=1 << 32) == INVALID
    assert call(nf=1 << 32) == INVALID
    # ahead of everything a plan or a later check could say: misaligned pointers,
    # an empty index and no scratch with a bad argument are still SRPC_E_INVALID
    odd = dict(buf=buf + 1, idx=idx + 4, offs=offs + 2, cnt=cnt + 4, ends=ends + 4, scr=scr + 4, idx_bytes=0, scr_bytes=0)
    assert call(k=17, **odd) == INVALID
    assert call(buf_len=1 << 32, **odd) == INVALID
    assert call(nf=1 << 32, **odd) == INVALID
    assert call(cap=None, **odd) == INVALID
    assert call(scap=None, **odd) == INVALID
    for name in ("idx", "cnt", "ends", "scr", "buf", "offs"):
        kw = dict(odd)
        kw[name] = None
        assert call(**kw) == INVALID, name
