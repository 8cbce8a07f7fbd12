"""The server's arrival-order decode into struct arrays without a device
(srpc_frames_unpack_requests_mixed_aos, include/srpc_gpu.h): the symbol is
exported, in the ctypes table with the column call's arguments (d_cols replaced
by d_recs, h_stride, h_leaf_offs, h_fill; scratch added) and in the header,
still within ABI 8; and every step-1 SRPC_E_INVALID refusal is answered before
a plan is read (the plans here are 0xFF bytes: a call that looked at one would
crash or answer something else)."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build
from tests.test_mixed_abi import fake_plans
from tests.test_mixed_aos_abi import arrays, with_one

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "srpc_frames_unpack_requests_mixed_aos"
INVALID = _lib.SRPC_E_INVALID


def test_symbol_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    assert NAME in exported and NAME in _lib.SIGNATURES and re.search(rf"\b{NAME}\s*\(", header)
    assert len(_lib.SIGNATURES["srpc_frames_unpack_requests_mixed"][1]) == 15
    assert len(_lib.SIGNATURES[NAME][1]) == 15 - 1 + 4 + 2 == 20
    assert _lib.lib().srpc_gpu_abi_version() == 8  # an addition within ABI 8


def test_refuses_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    recs, strides, loffs, fills, cap, _keep2 = arrays()
    buf, offs, cls, idx, cnt, scratch = 0x7000, 0x5000, 0x6000, 0x3000, 0x9000, 0x8000

    def unpack(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, recs=recs, strides=strides, loffs=loffs,
               fills=fills, cap=cap, cls=cls, idx=idx, cnt=cnt, scratch=scratch):
        return L.srpc_frames_unpack_requests_mixed_aos(plans, k, buf, buf_len, offs, nf, recs, strides, loffs, fills,
                                                       None, cap, cls, idx, 1 << 20, cnt, None, scratch, 1 << 20, None)

    # each NULL pointer in turn
    assert unpack(plans=None) == INVALID
    assert unpack(buf=None) == INVALID
    assert unpack(offs=None) == INVALID
    assert unpack(recs=None) == INVALID
    assert unpack(strides=None) == INVALID
    assert unpack(loffs=None) == INVALID
    assert unpack(fills=None) == INVALID
    assert unpack(cap=None) == INVALID
    assert unpack(cls=None) == INVALID
    assert unpack(idx=None) == INVALID
    assert unpack(cnt=None) == INVALID
    assert unpack(scratch=None) == INVALID
    # the ranges
    assert unpack(k=0) == INVALID
    assert unpack(k=17) == INVALID
    assert unpack(buf_len=1 << 32) == INVALID
    assert unpack(nf=1 << 32) == INVALID
    # per plan: the stride, and the pointers behind the arrays
    assert unpack(strides=with_one(strides, C.c_uint64, 0, 0)) == INVALID
    assert unpack(strides=with_one(strides, C.c_uint64, 3, 1 << 32)) == INVALID
    assert unpack(fills=with_one(fills, C.c_void_p, 1, None)) == INVALID
    assert unpack(loffs=with_one(loffs, C.c_void_p, 2, None)) == INVALID
    assert unpack(recs=with_one(recs, C.c_void_p, 3, None)) == INVALID  # an array with room and no memory
    assert unpack(k=16, strides=with_one(strides, C.c_uint64, 15, 0)) == INVALID
