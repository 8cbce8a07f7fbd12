"""The server's arrival-order decode into columns or struct arrays, plan by plan,
without a device (srpc_frames_unpack_requests_mixed_legs, include/srpc_gpu.h):
the symbol is exported, in the ctypes table with the _mixed_var request call's
20 arguments plus d_recs, h_stride, h_leaf_offs and h_fill, and in the header,
still within ABI 8; and every step-1 SRPC_E_INVALID refusal is answered before
a plan is read (the plans here are 0xFF bytes: a call that looked at one would
crash or answer something else).  The refusals that need real plans --
UNSUPPORTED, INVALID for the layout, ALIGN, CAPACITY, in that order -- are in
tests/test_gpu_requests_mixed_legs.py."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build
from tests.test_mixed_abi import fake_plans
from tests.test_mixed_legs_abi import declared_args

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "srpc_frames_unpack_requests_mixed_legs"
INVALID = _lib.SRPC_E_INVALID


def test_symbol_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    assert NAME in exported and NAME in _lib.SIGNATURES and re.search(rf"\b{NAME}\s*\(", header)
    assert len(_lib.SIGNATURES["srpc_frames_unpack_requests_mixed_var"][1]) == 20
    assert len(_lib.SIGNATURES[NAME][1]) == 20 + 4 == 24 == declared_args(header, NAME)
    # declared after the _mixed_var request call, in a section of its own within ABI 8
    assert header.index("int srpc_frames_unpack_requests_mixed_var(") < header.index(f"int {NAME}(")
    assert "added within ABI 8" in header[:header.index(f"int {NAME}(")].rsplit("/* ----", 1)[1]
    assert _lib.lib().srpc_gpu_abi_version() == 8 and "#define SRPC_GPU_ABI_VERSION 8" in header
    from srpc_amd import packer
    assert callable(packer.MixedLegFrames.unpack_requests)
    assert packer.MixedLegFrames.unpack_requests is not packer.MixedVarFrames.unpack_requests


def test_refuses_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    col = (C.c_void_p * 1)(0x1000)
    cols = (C.c_void_p * 16)(*[C.cast(col, C.c_void_p).value] * 16)
    so = (C.c_void_p * 16)()
    caps = (C.c_void_p * 16)()
    cap = (C.c_uint64 * 16)(*[10] * 16)
    recs = (C.c_void_p * 16)(*[0xB000] * 16)
    stride = (C.c_uint64 * 16)(16, 0, 8, 0)
    loff = (C.c_uint32 * 2)(8, 12)
    loffs = (C.c_void_p * 16)(*[C.cast(loff, C.c_void_p).value] * 16)
    fill = C.create_string_buffer(b"\x11" * 256, 256)
    fills = (C.c_void_p * 16)(*[C.cast(fill, C.c_void_p).value] * 16)
    buf, offs, cls, idx, cnt, ends, scratch = 0x7000, 0x5000, 0x6000, 0x3000, 0x9000, 0xA000, 0x8000

    def edited(arr, k, v, ctype=C.c_void_p):
        vals = [arr[i] for i in range(16)]
        vals[k] = v
        return (ctype * 16)(*vals)

    def unpack(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, cols=cols, so=so, caps=caps, recs=recs,
               stride=stride, loffs=loffs, fills=fills, first=None, cap=cap, cls=cls, idx=idx, cnt=cnt, ends=ends,
               scratch=scratch):
        return L.srpc_frames_unpack_requests_mixed_legs(plans, k, buf, buf_len, offs, nf, cols, so, caps, recs, stride,
                                                        loffs, fills, first, cap, cls, idx, 1 << 20, cnt, ends, None,
                                                        scratch, 1 << 30, None)

    # srpc_frames_unpack_requests_mixed_var's checks: each required pointer NULL in turn
    assert unpack(plans=None) == INVALID
    assert unpack(buf=None) == INVALID
    assert unpack(offs=None) == INVALID
    assert unpack(cols=None) == INVALID
    assert unpack(so=None) == INVALID
    assert unpack(caps=None) == INVALID
    assert unpack(cap=None) == INVALID
    assert unpack(cls=None) == INVALID
    assert unpack(idx=None) == INVALID
    assert unpack(cnt=None) == INVALID
    assert unpack(ends=None) == INVALID
    assert unpack(scratch=None) == INVALID
    # ... and the struct-array arrays
    assert unpack(recs=None) == INVALID
    assert unpack(stride=None) == INVALID
    assert unpack(loffs=None) == INVALID
    assert unpack(fills=None) == INVALID
    # the ranges
    assert unpack(k=0) == INVALID
    assert unpack(k=17) == INVALID
    assert unpack(buf_len=1 << 32) == INVALID
    assert unpack(nf=1 << 32) == INVALID
    # per plan: the stride, and for a record plan the pointers behind the arrays
    assert unpack(stride=edited(stride, 3, 1 << 32, C.c_uint64)) == INVALID
    assert unpack(stride=edited(stride, 0, 1 << 32, C.c_uint64)) == INVALID
    assert unpack(loffs=edited(loffs, 0, None)) == INVALID
    assert unpack(fills=edited(fills, 2, None)) == INVALID  # a record plan without a fill
    assert unpack(recs=edited(recs, 2, None)) == INVALID    # ... without an array, with room
    assert unpack(recs=edited(recs, 2, None), first=(C.c_uint64 * 16)(*[9] * 16)) == INVALID  # one element of room
    assert unpack(k=16, stride=edited(stride, 15, 8, C.c_uint64), loffs=edited(loffs, 15, None)) == INVALID


def test_all_column_strides_pass_the_argument_step():
    """A stride of 0 on every plan is the all-columns call: step 1 lets it through
    and the plans are read.  The plans are 0xFF bytes as long as a real plan
    (no prefix that short, more fields and strings than any call takes), which
    step 2 answers with SRPC_E_UNSUPPORTED; so would a column plan's NULL
    struct-array entries be, which step 1 must not look at."""
    L = _lib.lib()
    mem = [C.create_string_buffer(b"\xff" * (1 << 16), 1 << 16) for _ in range(4)]
    plans = (C.c_void_p * 4)(*[C.cast(m, C.c_void_p).value for m in mem])
    col = (C.c_void_p * 1)(0x1000)
    cols = (C.c_void_p * 4)(*[C.cast(col, C.c_void_p).value] * 4)
    null = (C.c_void_p * 4)()
    cap = (C.c_uint64 * 4)(10, 10, 10, 10)
    zero = (C.c_uint64 * 4)()
    rc = L.srpc_frames_unpack_requests_mixed_legs(plans, 4, 0x7000, 100, 0x5000, 3, cols, null, null, null, zero, null,
                                                  null, None, cap, 0x6000, 0x3000, 1 << 20, 0x9000, 0xA000, None, 0x8000,
                                                  1 << 30, None)
    assert rc == _lib.SRPC_E_UNSUPPORTED != INVALID
