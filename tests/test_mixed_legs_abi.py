"""The mixed-batch entry points that take, per plan, columns or a struct array
(srpc_frames_*_mixed_legs), without a device: the four symbols are exported, in
the ctypes table and in the header, still within ABI 8; the existing mixed
calls keep their argument counts; and every refusal of the header's step 1
answers SRPC_E_INVALID before any plan is read and before any device work (the
refusals that need real plans -- UNSUPPORTED, INVALID for the layout, ALIGN,
CAPACITY, in that order -- are in tests/test_gpu_mixed_legs.py)."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = {"srpc_frames_mixed_legs_scratch_bytes": 5, "srpc_frames_mixed_legs_tile": 5,
       "srpc_frames_pack_requests_mixed_legs": 20, "srpc_frames_unpack_replies_mixed_legs": 25}
OLD = {"srpc_frames_pack_requests_mixed": 13, "srpc_frames_unpack_replies_mixed": 16,
       "srpc_frames_pack_requests_mixed_aos": 15, "srpc_frames_unpack_replies_mixed_aos": 21,
       "srpc_frames_pack_requests_mixed_var": 17, "srpc_frames_unpack_replies_mixed_var": 21,
       "srpc_frames_unpack_requests_mixed": 15, "srpc_frames_unpack_requests_mixed_aos": 20,
       "srpc_frames_unpack_requests_mixed_var": 20}
INVALID = _lib.SRPC_E_INVALID


def declared_args(header, name):
    """The number of parameters the header declares for `name`."""
    m = re.search(rf"\bint {name}\s*\(([^;]*)\)\s*;", header)
    assert m, name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return params.count(",") + 1


def test_symbols_exported_bound_and_declared():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name, nargs in {**NEW, **OLD}.items():
        assert name in exported and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs == declared_args(header, name), name
    assert "added within ABI 8" in header[:header.index("srpc_frames_mixed_legs_scratch_bytes(")].rsplit("/* ----", 1)[1]
    assert _lib.lib().srpc_gpu_abi_version() == 8 and "#define SRPC_GPU_ABI_VERSION 8" in header
    import srpc_amd
    assert srpc_amd.MixedLegFrames.__name__ in srpc_amd.__all__
    from srpc_amd import packer
    assert "MixedLegFrames" in packer.__all__ and issubclass(packer.MixedLegFrames, packer.MixedVarFrames)


def fake_plans(k=16):
    """Plan pointers that are not plans: a call that reads them before refusing
    its arguments shows in its return value or crashes."""
    mem = [C.create_string_buffer(b"\xff" * 64, 64) for _ in range(k)]
    arr = (C.c_void_p * k)(*[C.cast(m, C.c_void_p).value for m in mem])
    return arr, mem


def u64s(*v):
    return (C.c_uint64 * len(v))(*v)


def test_hooks_refuse_arguments_before_reading_a_plan():
    L = _lib.lib()
    plans, _keep = fake_plans()
    stride = u64s(16, 0, 8, 0)
    out = C.c_uint64(77)
    sb = L.srpc_frames_mixed_legs_scratch_bytes
    assert sb(None, 4, stride, 10, C.byref(out)) == INVALID
    assert sb(plans, 0, stride, 10, C.byref(out)) == INVALID
    assert sb(plans, 17, stride, 10, C.byref(out)) == INVALID
    assert sb(plans, 4, stride, 1 << 32, C.byref(out)) == INVALID
    assert sb(plans, 4, stride, 10, None) == INVALID
    assert sb(plans, 4, u64s(16, 0, 1 << 32, 0), 10, C.byref(out)) == INVALID  # a stride of 2^32
    null = (C.c_void_p * 4)()
    assert sb(null, 4, stride, 10, C.byref(out)) == INVALID  # a NULL plan
    assert sb(null, 4, None, 10, C.byref(out)) == INVALID    # ... also without strides
    assert out.value == 77
    t, img = C.c_uint32(77), C.c_uint32(78)
    tile = L.srpc_frames_mixed_legs_tile
    assert tile(None, 4, stride, C.byref(t), C.byref(img)) == INVALID
    assert tile(plans, 0, stride, C.byref(t), C.byref(img)) == INVALID
    assert tile(plans, 17, stride, C.byref(t), C.byref(img)) == INVALID
    assert tile(plans, 4, stride, None, C.byref(img)) == INVALID
    assert tile(plans, 4, stride, C.byref(t), None) == INVALID
    assert tile(plans, 4, u64s(1 << 32, 0, 0, 0), C.byref(t), C.byref(img)) == INVALID
    assert tile(null, 4, stride, C.byref(t), C.byref(img)) == INVALID
    assert (t.value, img.value) == (77, 78)


def test_pack_and_decode_refuse_arguments_before_reading_a_plan():
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
    m, idx, out, offs, codes, buf, total, scratch, ends = (0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000,
                                                           0x9000, 0xA000)

    def edited(arr, k, v, ctype=C.c_void_p):
        vals = [arr[i] for i in range(16)]
        vals[k] = v
        return (ctype * 16)(*vals)

    def pack(plans=plans, k=4, cols=cols, so=so, recs=recs, stride=stride, loffs=loffs, first=None, cap=cap, m=m,
             idx=idx, n=5, out=out, out_cap=1 << 20, offs=offs, total=total, scratch=scratch):
        return L.srpc_frames_pack_requests_mixed_legs(plans, k, cols, so, recs, stride, loffs, first, cap, m, idx, n, out,
                                                      out_cap, offs, total, None, scratch, 1 << 30, None)

    # srpc_frames_pack_requests_mixed_var's checks
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
    # the struct-array arguments
    assert pack(recs=None) == INVALID
    assert pack(stride=None) == INVALID
    assert pack(loffs=None) == INVALID
    assert pack(stride=edited(stride, 1, 1 << 32, C.c_uint64)) == INVALID  # a stride of 2^32
    assert pack(loffs=edited(loffs, 2, None)) == INVALID                   # a record plan without leaf offsets
    assert pack(recs=edited(recs, 0, None)) == INVALID                     # ... without an array, with room
    assert pack(recs=edited(recs, 0, None), first=(C.c_uint64 * 16)(*[9] * 16)) == INVALID  # one element of room

    def unpack(plans=plans, k=4, buf=buf, buf_len=100, offs=offs, nf=3, m=m, idx=idx, n=5, cols=cols, so=so, caps=caps,
               recs=recs, stride=stride, loffs=loffs, fills=fills, first=None, cap=cap, codes=codes, ends=ends,
               scratch=scratch):
        return L.srpc_frames_unpack_replies_mixed_legs(plans, k, buf, buf_len, offs, nf, m, idx, n, 13, cols, so, caps,
                                                       recs, stride, loffs, fills, first, cap, codes, ends, None, scratch,
                                                       1 << 30, None)

    # srpc_frames_unpack_replies_mixed_var's checks
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
    # the struct-array arguments
    assert unpack(recs=None) == INVALID
    assert unpack(stride=None) == INVALID
    assert unpack(loffs=None) == INVALID
    assert unpack(fills=None) == INVALID
    assert unpack(stride=edited(stride, 3, 1 << 32, C.c_uint64)) == INVALID
    assert unpack(loffs=edited(loffs, 0, None)) == INVALID
    assert unpack(fills=edited(fills, 2, None)) == INVALID  # a record plan without a fill
    assert unpack(recs=edited(recs, 2, None)) == INVALID
