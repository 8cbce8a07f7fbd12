"""srpc_frames_unpack_replies_aos without a device: both symbols are exported,
bound and in the header, the ABI version is unchanged, and the first group of
refusals (NULL pointers, a zero stride, a stream of 4 GiB) answers before the
plan is read."""
import ctypes as C
import os
import re
import subprocess

from srpc_amd import _lib, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ["srpc_frames_unpack_replies_aos", "srpc_frames_replies_aos_per_tile"]


def test_symbols_exported_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (srpc_\w+)", out.stdout))
    header = open(os.path.join(ROOT, "include", "srpc_gpu.h")).read()
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    assert len(_lib.SIGNATURES["srpc_frames_unpack_replies_aos"][1]) == 12
    assert len(_lib.SIGNATURES["srpc_frames_replies_aos_per_tile"][1]) == 3
    assert _lib.lib().srpc_gpu_abi_version() == 8  # an addition within ABI 8


def test_first_refusals_answer_before_the_plan_is_read():
    L = _lib.lib()
    call = L.srpc_frames_unpack_replies_aos
    recs, codes = C.c_void_p(0x1000), C.c_void_p(0x2000)
    offs = (C.c_uint32 * 1)(8)
    fill = C.create_string_buffer(16)
    INV = _lib.SRPC_E_INVALID
    assert call(None, None, 0, None, 0, recs, 16, offs, fill, codes, None, None) == INV
    # the plan here is not one: it must not be read
    fake = C.create_string_buffer(64)
    plan = C.cast(fake, C.c_void_p)
    assert call(plan, None, 0, None, 1, None, 16, offs, fill, codes, None, None) == INV   # d_records, nframes > 0
    assert call(plan, None, 0, None, 1, recs, 16, None, fill, codes, None, None) == INV   # field_offsets
    assert call(plan, None, 0, None, 1, recs, 16, offs, None, codes, None, None) == INV   # h_fill
    assert call(plan, None, 0, None, 1, recs, 16, offs, fill, None, None, None) == INV    # d_codes
    assert call(plan, None, 0, None, 1, recs, 0, offs, fill, codes, None, None) == INV    # record_stride == 0
    assert call(plan, None, 1 << 32, None, 1, recs, 16, offs, fill, codes, None, None) == INV
    # a NULL offsets or fill is refused with no frames too
    assert call(plan, None, 0, None, 0, None, 16, None, fill, codes, None, None) == INV
    assert call(plan, None, 0, None, 0, None, 16, offs, None, codes, None, None) == INV


def test_per_tile_leaves_its_output_alone_on_refusal():
    L = _lib.lib()
    fake = C.create_string_buffer(64)
    plan = C.cast(fake, C.c_void_p)
    out = C.c_uint32(77)
    assert L.srpc_frames_replies_aos_per_tile(None, 32, C.byref(out)) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_replies_aos_per_tile(plan, 32, None) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_replies_aos_per_tile(plan, 0, C.byref(out)) == _lib.SRPC_E_INVALID
    assert out.value == 77
