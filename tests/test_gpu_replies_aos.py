"""Reply streams of mixed frames decoded in call order straight into an array
of structs (srpc_frames_unpack_replies_aos, include/srpc_gpu.h): the AoS form
of srpc_frames_unpack_replies.

Nothing expected comes from the kernel under test.  The streams, the inputs
and the per-frame table (`model`) are tests/test_gpu_replies.py's.  The expected
struct bytes are numpy: the fill record tiled n times, then every leaf's bytes
set to the call's input where the frame is full and to zero elsewhere.  The
codes, the flags and the first bad index are also compared with what the
column call returns on the same bytes.

Outputs start as 0xA5 with 16 guard bytes behind the array and behind the
codes; the fill is random bytes, so a dropped or misplaced fill byte shows."""
import ctypes as C
import struct

import numpy as np
import pytest

import srpc_amd
from srpc_amd import GpuPacker, Schema, _lib, framed_response_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import ALL_KINDS, dev, empty, host, read_status, status_buf  # noqa: E402
from tests.test_gpu_replies import (FRAME_BYTES, NO_CODE, SCHEMAS, model, packer, reference,  # noqa: E402
                                    run as run_columns, stream)

PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1

# (stride, leaf offsets): the natural C++ layout behind an 8-byte vtable slot, a
# stride that is no multiple of 16 (leaves out of wire order), stride 256 with
# the leaves at the far end
LAYOUTS = {
    "number": {"natural": (16, (8,)), "odd": (24, (20,)), "far": (256, (252,))},
    "all_kinds": {"natural": (32, (8, 9, 10, 12, 16, 24)), "odd": (40, (3, 1, 0, 6, 12, 24)),
                  "far": (256, (239, 240, 241, 242, 244, 248))},
}
CASES = [(name, lay) for name in sorted(LAYOUTS) for lay in ("natural", "odd", "far")]


def fill_of(name, lay):
    stride, _ = LAYOUTS[name][lay]
    return np.random.default_rng(stride + len(name)).integers(0, 256, stride, dtype=np.uint8)


def per_tile(name, lay):
    stride, _ = LAYOUTS[name][lay]
    return packer(name).replies_aos_per_tile(stride)


def expected_structs(name, lay, n, full):
    stride, offsets = LAYOUTS[name][lay]
    ins, _ = reference(name)
    out = np.tile(fill_of(name, lay), (n, 1))
    for x, off in zip(ins, offsets):
        s = x.dtype.itemsize
        vals = np.ascontiguousarray(np.where(full, x[:n], 0).astype(x.dtype))
        out[:, off:off + s] = vals.view(np.uint8).reshape(n, s)
    return out


def run_aos(p, name, lay, buf, buf_len, offs, n):
    """One call on fresh 0xA5-filled outputs -> (rc, codes, structs (n, stride), flags, first)."""
    stride, offsets = LAYOUTS[name][lay]
    d_buf = dev(np.frombuffer(buf, np.uint8)) if buf else empty(16)
    d_offs = None if offs is None else (dev(offs) if n else empty(16))
    d_recs = empty(n * stride + 16)
    d_codes = empty(n + 16)
    st = status_buf()
    rc = p.unpack_replies_aos(d_buf, buf_len, d_offs, n, d_recs, stride, offsets, fill_of(name, lay).tobytes(),
                              d_codes, st)
    flags, first = read_status(st)
    assert (host(d_recs, n * stride + 16)[n * stride:] == 0xA5).all(), "wrote past the array's n structs"
    assert (host(d_codes, n + 16)[n:] == 0xA5).all()
    return rc, host(d_codes, n), host(d_recs, n * stride).reshape(n, stride), flags, first


def check(name, lay, p, buf, buf_len, offs, n, want_rc=0):
    """The AoS call against the table and numpy, and against the column call on the same bytes."""
    F = FRAME_BYTES[name]
    moffs = offs if offs is not None else (np.arange(n, dtype=np.uint64) * F)
    want, full, flags, first = model(buf, buf_len, moffs, n, F, p.prefix)
    rc, codes, recs, gflags, gfirst = run_aos(p, name, lay, buf, buf_len, offs, n)
    print(f"{name}/{lay} n={n} rc={rc} flags={gflags} first={gfirst} want rc={want_rc} flags={flags} first={first}")
    assert rc == want_rc
    assert np.array_equal(codes, want)
    assert (gflags, gfirst) == (flags, first)
    exp = expected_structs(name, lay, n, full)
    bad = np.flatnonzero((recs != exp).any(axis=1))
    assert bad.size == 0, f"struct {bad[0]}: {recs[bad[0]].tolist()} != {exp[bad[0]].tolist()}"
    crc, ccodes, _, cflags, cfirst = run_columns(p, buf, buf_len, offs, n)
    assert (rc, gflags, gfirst) == (crc, cflags, cfirst) and np.array_equal(codes, ccodes)
    return want, full, flags, first


@pytest.mark.parametrize("name,lay", CASES)
def test_frames_per_tile_rule(name, lay):
    stride, _ = LAYOUTS[name][lay]
    s16 = (stride + 15) // 16 * 16
    assert per_tile(name, lay) == 16 * max(1, (16384 - 4 * s16) // (16 * FRAME_BYTES[name]))  # the documented rule


@pytest.mark.parametrize("name,lay", CASES)
@pytest.mark.parametrize("k", range(6))
def test_uniform_and_indexed_all_full(name, lay, k):
    R = per_tile(name, lay)
    n = [0, 1, R - 1, R, R + 1, 4097][k]
    p = packer(name, code=2)  # the plan's own code byte is ignored
    codes = np.random.default_rng(n).integers(0, 3, n)
    buf, offs = stream(name, n, codes)
    for o in (None, offs):
        want, full, flags, _ = check(name, lay, p, buf, len(buf), o, n)
        assert full.all() and flags == 0 and np.array_equal(want, codes)


@pytest.mark.parametrize("name,lay", CASES)
@pytest.mark.parametrize("short", ["byte", "frame"])
def test_uniform_short_stream(name, lay, short):
    F = FRAME_BYTES[name]
    n = per_tile(name, lay) + 1
    p = packer(name)
    codes = np.random.default_rng(7).integers(0, 3, n)
    buf, _ = stream(name, n, codes)
    buf_len = len(buf) - ((F // 2) if short == "byte" else F)  # mid-frame, or at a frame's edge
    want, full, flags, first = check(name, lay, p, buf, buf_len, None, n, want_rc=_lib.SRPC_ERR_BOUNDS)
    nfit = buf_len // F
    assert flags == BOUNDS and first == nfit and full[:nfit].all() and not full[nfit:].any()
    assert (want[nfit:] == NO_CODE).all()  # later structs: the fill with zero leaves (expected_structs)


@pytest.mark.parametrize("name,lay", CASES)
@pytest.mark.parametrize("share", [0.1, 0.9])
def test_indexed_with_bare_frames(name, lay, share):
    n = 4097
    p = packer(name)
    rng = np.random.default_rng(n + int(10 * share))
    codes = rng.integers(0, 3, n)
    bare = rng.random(n) < share
    special = {int(i): struct.pack(">IB", 1, int(rng.integers(1, 256))) for i in np.flatnonzero(bare)}
    buf, offs = stream(name, n, codes, special)
    want, full, flags, _ = check(name, lay, p, buf, len(buf), offs, n)
    assert np.array_equal(full, ~bare) and flags == 0  # a bare frame is an answer, not an error
    assert all(want[i] == f[4] for i, f in special.items())


BAD = ["short_header", "be32_mismatch", "wrong_name", "empty_payload", "out_of_order", "past_buffer"]


@pytest.mark.parametrize("name,lay", CASES)
@pytest.mark.parametrize("case", BAD)
def test_indexed_one_bad_frame(name, lay, case):
    """One bad frame at index 0, R - 1, R and last among full frames of mixed
    codes: every full frame around it must still decode."""
    p = packer(name)
    R = per_tile(name, lay)
    n = 2 * R + 5
    codes = np.random.default_rng(BAD.index(case)).integers(0, 3, n)
    _, rows = reference(name)
    for at in (0, R - 1, R, n - 1):
        good = rows[0][at].tobytes()
        special = {}
        want_flag = BOUNDS
        if case == "short_header":
            special[at] = b"\x00\x00\x00"
        elif case == "be32_mismatch":
            special[at] = struct.pack(">I", len(good) - 3) + good[4:]
        elif case == "wrong_name":
            b = bytearray(good)
            b[len(p.prefix) - 1] ^= 0x20
            special[at], want_flag = bytes(b), PREFIX
        elif case == "empty_payload":
            special[at] = struct.pack(">I", 0)
        buf, offs = stream(name, n, codes, special)
        bad = {at}
        if case == "out_of_order":
            a = min(at, n - 2)
            offs[a], offs[a + 1] = offs[a + 1], offs[a]
            bad = {a - 1, a, a + 1} - {-1}
        elif case == "past_buffer":
            offs[at] = len(buf) + 100
            bad = {at - 1, at} - {-1}
        want, full, flags, first = check(name, lay, p, buf, len(buf), offs, n)
        assert flags == want_flag and first == min(bad)
        assert not full[sorted(bad)].any() and full.sum() == n - len(bad)


@pytest.mark.parametrize("name,lay", CASES)
def test_oversize_junk_pushes_frames_out_of_the_image(name, lay):
    """A junk frame larger than the image in the middle of a tile: the frames
    of that tile behind it are read from global memory."""
    F = FRAME_BYTES[name]
    p = packer(name)
    R = per_tile(name, lay)
    n = 3 * R + 5
    at = R + R // 2
    rng = np.random.default_rng(R)
    codes = rng.integers(0, 3, n)
    junk = R * F + 4096  # more than the R * F + 16 bytes a tile stages
    special = {at: struct.pack(">I", junk - 4) + b"\x07" + rng.bytes(junk - 5)}
    buf, offs = stream(name, n, codes, special)
    want, full, flags, first = check(name, lay, p, buf, len(buf), offs, n)
    assert want[at] == 7 and (flags, first) == (PREFIX, at) and full.sum() == n - 1


@pytest.mark.parametrize("name,lay", CASES)
def test_long_indexed_run(name, lay):
    n = 50_001
    p = packer(name)
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 3, n)
    special = {int(i): struct.pack(">IB", 1, 9) for i in np.flatnonzero(rng.random(n) < 0.3)}
    buf, offs = stream(name, n, codes, special)
    _, full, flags, _ = check(name, lay, p, buf, len(buf), offs, n)
    assert flags == 0 and full.sum() == n - len(special)


def test_argument_refusals():
    L = _lib.lib()
    call = L.srpc_frames_unpack_replies_aos
    recs, codes, buf = empty(1024), empty(64), empty(64)
    fill = C.create_string_buffer(264)
    one = (C.c_uint32 * 1)(8)
    six = (C.c_uint32 * 6)(8, 9, 10, 12, 16, 24)
    UNS, INV, ALIGN = _lib.SRPC_E_UNSUPPORTED, _lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN

    def go(plan, offsets, stride, d_buf=buf.data_ptr(), d_recs=recs.data_ptr(), F=23):
        return call(plan._h, d_buf, F, None, 1, d_recs, stride, offsets, fill, codes.data_ptr(), None, None)

    # 2. a string plan, no prefix, a prefix too short to hold the code byte, a stride over 256
    sp = GpuPacker(Schema("S", (("s", srpc_amd.STRING),)), framed_response_prefix(srpc_amd.NUMBER))
    assert go(sp, one, 16) == UNS
    assert go(GpuPacker(ALL_KINDS), six, 32, F=17) == UNS
    assert go(GpuPacker(srpc_amd.NUMBER, b"\0\0\0\5"), one, 16, F=8) == UNS
    p, pa = packer("number"), packer("all_kinds")
    assert go(p, (C.c_uint32 * 1)(260), 264) == UNS       # the refused layout: stride 264
    assert go(p, (C.c_uint32 * 1)(300), 264) == UNS       # ... before its leaves are looked at
    hook = C.c_uint32(77)
    assert L.srpc_frames_replies_aos_per_tile(p._h, 264, C.byref(hook)) == UNS and hook.value == 77
    assert L.srpc_frames_replies_aos_per_tile(sp._h, 16, C.byref(hook)) == UNS and hook.value == 77
    # 3. a leaf past the stride, overlapping leaves (before any alignment)
    assert go(p, (C.c_uint32 * 1)(14), 16) == INV
    assert go(pa, (C.c_uint32 * 6)(8, 9, 10, 12, 16, 16), 32, F=39) == INV       # int64 over the int32
    assert go(pa, (C.c_uint32 * 6)(8, 8, 10, 12, 16, 24), 32, F=39) == INV
    assert go(pa, (C.c_uint32 * 6)(8, 9, 10, 9, 16, 24), 32, F=39) == INV        # misaligned too: INVALID first
    assert go(pa, (C.c_uint32 * 6)(8, 9, 10, 12, 16, 28), 32, F=39) == INV       # past the stride, misaligned too
    # 4. alignment: the stream, the array, an offset, the stride
    assert go(p, one, 16, d_buf=buf.data_ptr() + 8) == ALIGN
    assert go(p, one, 16, d_recs=recs.data_ptr() + 8) == ALIGN
    assert go(p, (C.c_uint32 * 1)(6), 16) == ALIGN
    assert go(p, one, 18) == ALIGN
    assert go(pa, (C.c_uint32 * 6)(8, 9, 10, 13, 16, 24), 32, F=39) == ALIGN
    assert go(pa, six, 36, F=39) == ALIGN                 # the int64 against the stride
    torch.cuda.synchronize()
    assert (host(codes, 64) == 0xA5).all() and (host(recs, 1024) == 0xA5).all()  # nothing was launched


def test_captured_and_replayed():
    """One call captured in a graph and replayed: the capture runs nothing, the
    replay writes the structs and the codes, and again after they are cleared."""
    name, lay = "all_kinds", "natural"
    stride, offsets = LAYOUTS[name][lay]
    n = 4097
    p = packer(name)
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 3, n)
    special = {int(i): struct.pack(">IB", 1, 3) for i in np.flatnonzero(rng.random(n) < 0.2)}
    buf, offs = stream(name, n, codes, special)
    want, full, flags, first = model(buf, len(buf), offs, n, FRAME_BYTES[name], p.prefix)
    exp = expected_structs(name, lay, n, full)
    d_buf, d_offs = dev(np.frombuffer(buf, np.uint8)), dev(offs)
    d_recs = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    d_codes = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    st = status_buf()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        p.unpack_replies_aos(d_buf, len(buf), d_offs, n, d_recs, stride, offsets, fill_of(name, lay).tobytes(),
                             d_codes, st, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert not d_recs.any() and not d_codes.any()  # capturing ran nothing
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(d_recs, n * stride).reshape(n, stride), exp)
        assert np.array_equal(host(d_codes, n), want) and read_status(st) == (flags, first)
        assert not d_recs[n * stride:].any() and not d_codes[n:].any()
        d_recs.zero_()
        d_codes.zero_()
