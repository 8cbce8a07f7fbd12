"""The struct-array legs of the mixed batches without a device
(srpc_frames_pack_requests_mixed_aos / _unpack_replies_mixed_aos /
_mixed_aos_scratch_bytes, include/srpc_gpu.h): the symbols are exported, in the
ctypes table and in the header, still within ABI 8; and every SRPC_E_INVALID
refusal of both calls is answered before a plan is read (the plans here are
0xFF bytes: a call that looked at one would crash or answer something else)."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build
from tests.test_mixed_abi import fake_plans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["srpc_frames_mixed_aos_scratch_bytes", "srpc_frames_pack_requests_mixed_aos",
       "srpc_frames_unpack_replies_mixed_aos"]
INVALID = _lib.SRPC_E_INVALID


def test_symbols_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name in NEW + ["srpc_frames_mixed_aos_tile"]:
        assert name in exported and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header), name
    assert len(_lib.SIGNATURES["srpc_frames_mixed_aos_scratch_bytes"][1]) == 4
    # the column calls' arguments with d_cols replaced by d_recs, h_stride, h_leaf_offs (+ h_fill, scratch)
    assert len(_lib.SIGNATURES["srpc_frames_pack_requests_mixed_aos"][1]) == 13 - 1 + 3
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies_mixed_aos"][1]) == 16 - 1 + 6
    assert _lib.lib().srpc_gpu_abi_version() == 8  # additions within ABI 8


def arrays(stride=16):
    offs = (C.c_uint32 * 1)(8)
    fill = C.create_string_buffer(256)
    keep = (offs, fill)
    recs = (C.c_void_p * 16)(*[0x10000 * (k + 1) for k in range(16)])
    strides = (C.c_uint64 * 16)(*[stride] * 16)
    loffs = (C.c_void_p * 16)(*[C.cast(offs, C.c_void_p).value] * 16)
    fills = (C.c_void_p * 16)(*[C.cast(fill, C.c_void_p).value] * 16)
    cap = (C.c_uint64 * 16)(*[10] * 16)
    return recs, strides, loffs, fills, cap, keep


def with_one(arr, ctype, k, value):
    vals = list(arr)
    vals[k] = value
    return (ctype * 16)(*vals)


def test_pack_refuses_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    recs, strides, loffs, _, cap, _keep2 = arrays()
    m, idx, out, offs = 0x2000, 0x3000, 0x4000, 0x5000

    def pack(plans=plans, k=4, recs=recs, strides=strides, loffs=loffs, cap=cap, m=m, idx=idx, n=5, out=out,
             out_cap=1 << 20):
        return L.srpc_frames_pack_requests_mixed_aos(plans, k, recs, strides, loffs, None, cap, m, idx, n, out, out_cap,
                                                     offs, None, None)

    assert pack(plans=None) == INVALID
    assert pack(k=0) == INVALID
    assert pack(k=17) == INVALID
    assert pack(recs=None) == INVALID
    assert pack(strides=None) == INVALID
    assert pack(loffs=None) == INVALID
    assert pack(cap=None) == INVALID
    assert pack(m=None) == INVALID
    assert pack(idx=None) == INVALID
    assert pack(out=None) == INVALID
    assert pack(n=1 << 32, out_cap=1 << 62) == INVALID
    assert pack(strides=with_one(strides, C.c_uint64, 2, 0)) == INVALID         # a zero stride
    assert pack(strides=with_one(strides, C.c_uint64, 3, 1 << 32)) == INVALID   # strides are below 2^32
    assert pack(recs=with_one(recs, C.c_void_p, 1, None)) == INVALID            # an array with room and no memory
    assert pack(loffs=with_one(loffs, C.c_void_p, 0, None)) == INVALID
    assert pack(k=16, strides=with_one(strides, C.c_uint64, 15, 0)) == INVALID


def test_decode_refuses_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    recs, strides, loffs, fills, cap, _keep2 = arrays()
    m, idx, offs, codes, buf, scratch = 0x2000, 0x3000, 0x5000, 0x6000, 0x7000, 0x8000

    def unpack(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, m=m, idx=idx, n=5, recs=recs, strides=strides,
               loffs=loffs, fills=fills, cap=cap, codes=codes, scratch=scratch):
        return L.srpc_frames_unpack_replies_mixed_aos(plans, k, buf, buf_len, offs, nf, m, idx, n, 13, recs, strides,
                                                      loffs, fills, None, cap, codes, None, scratch, 1 << 20, None)

    assert unpack(plans=None) == INVALID
    assert unpack(k=0) == INVALID
    assert unpack(k=17) == INVALID
    assert unpack(recs=None) == INVALID
    assert unpack(strides=None) == INVALID
    assert unpack(loffs=None) == INVALID
    assert unpack(fills=None) == INVALID
    assert unpack(cap=None) == INVALID
    assert unpack(codes=None) == INVALID
    assert unpack(scratch=None) == INVALID
    assert unpack(m=None) == INVALID
    assert unpack(idx=None) == INVALID
    assert unpack(buf=None) == INVALID
    assert unpack(offs=None) == INVALID       # required with frames: there is no uniform mode
    assert unpack(nf=6) == INVALID            # more frames than calls
    assert unpack(buf_len=1 << 32) == INVALID
    assert unpack(n=1 << 32, nf=3) == INVALID
    assert unpack(strides=with_one(strides, C.c_uint64, 0, 0)) == INVALID
    assert unpack(strides=with_one(strides, C.c_uint64, 3, 1 << 32)) == INVALID
    assert unpack(recs=with_one(recs, C.c_void_p, 3, None)) == INVALID
    assert unpack(loffs=with_one(loffs, C.c_void_p, 2, None)) == INVALID
    assert unpack(fills=with_one(fills, C.c_void_p, 1, None)) == INVALID


def test_scratch_bytes_refusals_leave_out_untouched():
    L = _lib.lib()
    plans, _keep = fake_plans()
    _, strides, _, _, _, _keep2 = arrays()
    out = C.c_uint64(77)
    call = L.srpc_frames_mixed_aos_scratch_bytes
    assert call(None, 4, strides, C.byref(out)) == INVALID
    assert call(plans, 4, None, C.byref(out)) == INVALID
    assert call(plans, 4, strides, None) == INVALID
    assert call(plans, 0, strides, C.byref(out)) == INVALID
    assert call(plans, 17, strides, C.byref(out)) == INVALID
    assert call(plans, 4, with_one(strides, C.c_uint64, 3, 0), C.byref(out)) == INVALID
    t = C.c_uint32(77)
    assert L.srpc_frames_mixed_aos_tile(None, 4, strides, C.byref(t)) == INVALID
    assert L.srpc_frames_mixed_aos_tile(plans, 4, None, C.byref(t)) == INVALID
    assert L.srpc_frames_mixed_aos_tile(plans, 4, strides, None) == INVALID
    assert L.srpc_frames_mixed_aos_tile(plans, 4, with_one(strides, C.c_uint64, 0, 0), C.byref(t)) == INVALID
    assert out.value == 77 and t.value == 77
