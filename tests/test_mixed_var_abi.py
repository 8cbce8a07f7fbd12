"""The mixed-batch entry points with string plans, without a device: the
symbols are exported, in the ctypes table and in the header, still within ABI
8; their host-side argument checks answer SRPC_E_INVALID before any plan is
read and before any device work (the refusals that need real plans --
UNSUPPORTED, ALIGN, CAPACITY, in that order -- are in
tests/test_gpu_mixed_var.py); and the fixed-only calls keep their signatures."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["srpc_frames_mixed_var_scratch_bytes", "srpc_frames_mixed_var_tile", "srpc_frames_pack_requests_mixed_var",
       "srpc_frames_unpack_replies_mixed_var"]
INVALID = _lib.SRPC_E_INVALID


def test_symbols_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    assert len(_lib.SIGNATURES["srpc_frames_pack_requests_mixed_var"][1]) == 17
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies_mixed_var"][1]) == 21
    # the fixed-only calls are unchanged
    assert len(_lib.SIGNATURES["srpc_frames_pack_requests_mixed"][1]) == 13
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies_mixed"][1]) == 16
    assert _lib.lib().srpc_gpu_abi_version() == 8  # additions within ABI 8
    import srpc_amd
    assert srpc_amd.MixedVarFrames.__name__ in srpc_amd.__all__


def fake_plans(k=16):
    """Plan pointers that are not plans: a call that reads them before refusing
    its arguments shows in its return value or crashes."""
    mem = [C.create_string_buffer(b"\xff" * 64, 64) for _ in range(k)]
    arr = (C.c_void_p * k)(*[C.cast(m, C.c_void_p).value for m in mem])
    return arr, mem


def test_hooks_refuse_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    out = C.c_uint64(77)
    assert L.srpc_frames_mixed_var_scratch_bytes(None, 4, 10, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_var_scratch_bytes(plans, 0, 10, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_var_scratch_bytes(plans, 17, 10, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_var_scratch_bytes(plans, 4, 1 << 32, C.byref(out)) == INVALID
    assert L.srpc_frames_mixed_var_scratch_bytes(plans, 4, 10, None) == INVALID
    null = (C.c_void_p * 4)()
    assert L.srpc_frames_mixed_var_scratch_bytes(null, 4, 10, C.byref(out)) == INVALID  # a NULL plan
    assert out.value == 77
    t, img = C.c_uint32(77), C.c_uint32(78)
    assert L.srpc_frames_mixed_var_tile(None, 4, C.byref(t), C.byref(img)) == INVALID
    assert L.srpc_frames_mixed_var_tile(plans, 0, C.byref(t), C.byref(img)) == INVALID
    assert L.srpc_frames_mixed_var_tile(plans, 17, C.byref(t), C.byref(img)) == INVALID
    assert L.srpc_frames_mixed_var_tile(plans, 4, None, C.byref(img)) == INVALID
    assert L.srpc_frames_mixed_var_tile(plans, 4, C.byref(t), None) == INVALID
    assert (t.value, img.value) == (77, 78)


def test_pack_and_decode_refuse_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    col = (C.c_void_p * 1)(0x1000)
    cols = (C.c_void_p * 16)(*[C.cast(col, C.c_void_p).value] * 16)
    so = (C.c_void_p * 16)()
    caps = (C.c_void_p * 16)()
    cap = (C.c_uint64 * 16)(*[10] * 16)
    m, idx, out, offs, codes, buf, total, scratch, ends = (0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000,
                                                           0x9000, 0xA000)

    def pack(plans=plans, k=4, cols=cols, so=so, cap=cap, m=m, idx=idx, n=5, out=out, out_cap=1 << 20, offs=offs,
             total=total, scratch=scratch):
        return L.srpc_frames_pack_requests_mixed_var(plans, k, cols, so, None, cap, m, idx, n, out, out_cap, offs, total,
                                                     None, scratch, 1 << 30, None)

    assert pack(plans=None) == INVALID
    assert pack(k=0) == INVALID
    assert pack(k=17) == INVALID
    assert pack(cols=None) == INVALID
    assert pack(so=None) == INVALID
    assert pack(cap=None) == INVALID
    assert pack(m=None) == INVALID
    assert pack(idx=None) == INVALID
    assert pack(out=None) == INVALID
    assert pack(offs=None) == INVALID
    assert pack(total=None) == INVALID
    assert pack(scratch=None) == INVALID
    assert pack(n=1 << 32) == INVALID
    assert pack(out_cap=1 << 32) == INVALID

    def unpack(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, m=m, idx=idx, n=5, cols=cols, so=so, caps=caps,
               cap=cap, codes=codes, ends=ends, scratch=scratch):
        return L.srpc_frames_unpack_replies_mixed_var(plans, k, buf, buf_len, offs, nf, m, idx, n, 13, cols, so, caps,
                                                      None, cap, codes, ends, None, scratch, 1 << 30, None)

    assert unpack(plans=None) == INVALID
    assert unpack(k=0) == INVALID
    assert unpack(k=17) == INVALID
    assert unpack(cols=None) == INVALID
    assert unpack(so=None) == INVALID
    assert unpack(caps=None) == INVALID
    assert unpack(cap=None) == INVALID
    assert unpack(codes=None) == INVALID
    assert unpack(ends=None) == INVALID
    assert unpack(scratch=None) == INVALID
    assert unpack(m=None) == INVALID
    assert unpack(idx=None) == INVALID
    assert unpack(buf=None) == INVALID
    assert unpack(offs=None) == INVALID       # required with frames: there is no uniform mode
    assert unpack(nf=6) == INVALID            # more frames than calls
    assert unpack(buf_len=1 << 32) == INVALID
    assert unpack(n=1 << 32, nf=3) == INVALID
