"""Reply streams of mixed frames decoded in call order on the device
(srpc_frames_unpack_replies, include/srpc_gpu.h): the client-side mirror of
the batched server.  A generated stub reads one reply at a time with
unpack_response<R> (packer.hpp:123-137: `u8 code | str(R::name) | body`);
here a whole batch's replies give one code per call and the fields in call
order, whatever mix of full frames, bare error frames and junk arrives.

Nothing expected comes from the kernel under test:
- well-formed frames are the CPU oracle's pack with a framed response prefix
  of code 0, 1 or 2, picked per call by a seeded code vector;
- bare and bad frames are literal bytes, offsets are accumulated in numpy;
- the expected codes, flags and first bad index are the header's table written
  out below (`model`), the expected fields the inputs where a frame is full
  and zero elsewhere;
- the oracle's own unpack of every well-formed frame reproduces the inputs,
  so the reference alone passes every equality made on full frames."""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, Schema, _lib, framed_response_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import ALL_KINDS, dev, empty, host, read_status, status_buf  # noqa: E402

NO_CODE = 0xFF
PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
SCHEMAS = {"number": srpc_amd.NUMBER, "all_kinds": ALL_KINDS}
FRAME_BYTES = {"number": 23, "all_kinds": 39}   # an odd stride: frames straddle every 16-byte chunk
NMAX = 50_001


def oracle_prefix(schema, code):
    pre = oracle.response_prefix(code, schema.name)
    return struct.pack(">I", len(pre) + schema.body_bytes) + pre


def dtypes(schema):
    return [oracle.KIND_DTYPE[k] for k in schema.kinds]


@functools.lru_cache(maxsize=None)
def reference(name):
    """NMAX calls' inputs and their well-formed reply frames for codes 0, 1, 2
    as (NMAX, F) byte arrays, from the CPU oracle; computed once, read-only."""
    schema = SCHEMAS[name]
    rng = np.random.default_rng(len(name))
    cols = []
    for k, dt in zip(schema.kinds, dtypes(schema)):
        if k == srpc_amd.BOOL:
            c = rng.integers(0, 2, NMAX).astype(dt)
        else:
            info = np.iinfo(dt)
            c = rng.integers(info.min, info.max, NMAX, dtype=np.int64, endpoint=True).astype(dt)
        c.setflags(write=False)
        cols.append(c)
    F = FRAME_BYTES[name]
    rows = []
    for code in (0, 1, 2):
        w = oracle.pack(schema.kinds, [np.array(c) for c in cols], NMAX, oracle_prefix(schema, code))
        a = np.frombuffer(w, np.uint8).reshape(NMAX, F)
        rows.append(a)
    return cols, rows


def model(buf, buf_len, offs, n, F, prefix):
    """The per-frame table of include/srpc_gpu.h: (codes, full, flags, first bad)."""
    codes = np.full(n, NO_CODE, np.uint8)
    full = np.zeros(n, bool)
    flags, first = 0, NONE
    for i in range(n):
        o = int(offs[i])
        e = int(offs[i + 1]) if i + 1 < n else buf_len
        flag = 0
        if o > e or e > buf_len or e - o < 4:
            flag = BOUNDS
        else:
            f, ln = buf[o:e], e - o
            if int.from_bytes(f[:4], "big") != ln - 4 or ln == 4:
                flag = BOUNDS
            else:
                codes[i] = f[4]
                if ln == F and f[:4] == prefix[:4] and f[5:len(prefix)] == prefix[5:]:
                    full[i] = True
                elif not (ln == 5 and f[4] != 0):
                    flag = PREFIX
        if flag:
            flags |= flag
            first = min(first, i)
    return codes, full, flags, first


def stream(name, n, codes, special=None):
    """Frames of calls 0..n-1: the well-formed frame with codes[i], or
    special[i] (literal bytes).  Returns (bytes, offsets)."""
    _, rows = reference(name)
    special = special or {}
    parts = [special[i] if i in special else rows[codes[i]][i].tobytes() for i in range(n)]
    offs = np.zeros(n, np.uint32)
    if n:
        offs[1:] = np.cumsum([len(p) for p in parts[:-1]])
    return b"".join(parts), offs


def packer(name, code=0):
    schema = SCHEMAS[name]
    p = GpuPacker(schema, framed_response_prefix(schema, code))
    assert p.prefix == oracle_prefix(schema, code) and p.record_bytes == FRAME_BYTES[name]
    return p


def run(p, buf, buf_len, offs, n):
    """One call on fresh 0xA5-filled outputs -> (rc, codes, cols, flags, first)."""
    schema = p.schema
    d_buf = dev(np.frombuffer(buf, np.uint8)) if buf else empty(16)
    d_offs = None if offs is None else (dev(offs) if n else empty(16))
    dts = dtypes(schema)
    d_cols = [empty(n * np.dtype(dt).itemsize + 16) for dt in dts]
    d_codes = empty(n + 16)
    st = status_buf()
    rc = p.unpack_replies(d_buf, buf_len, d_offs, n, d_cols, d_codes, st)
    flags, first = read_status(st)
    cols = [host(c, n * np.dtype(dt).itemsize, dt) for c, dt in zip(d_cols, dts)]
    guard = [host(c, n * np.dtype(dt).itemsize + 16)[-16:] for c, dt in zip(d_cols, dts)]
    assert all((g == 0xA5).all() for g in guard), "wrote past a column's n elements"
    assert (host(d_codes, n + 16)[n:] == 0xA5).all()
    return rc, host(d_codes, n), cols, flags, first


def check(name, got, n, want_codes, full, want_flags, want_first, want_rc=0):
    rc, codes, cols, flags, first = got
    assert rc == want_rc
    assert np.array_equal(codes, want_codes)
    ins, _ = reference(name)
    for c, x in zip(cols, ins):
        assert np.array_equal(c, np.where(full, x[:n], 0).astype(x.dtype))
    assert (flags, first) == (want_flags, want_first)


def sizes(name):
    R = 16 * max(1, 16384 // (16 * FRAME_BYTES[name]))  # the documented rule
    return [0, 1, R - 1, R, R + 1, 4097]


def test_frames_per_tile_rule():
    for name in SCHEMAS:
        assert packer(name).replies_per_tile == sizes(name)[3]


def test_oracle_unpacks_every_well_formed_frame():
    for name, schema in SCHEMAS.items():
        ins, rows = reference(name)
        for code in (0, 1, 2):
            st, cols, _, consumed, _ = oracle.unpack(schema.kinds, rows[code].tobytes(), NMAX,
                                                     oracle_prefix(schema, code))
            assert st == 0 and consumed == NMAX * FRAME_BYTES[name]
            for a, b in zip(ins, cols):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("k", range(6))
def test_uniform_and_indexed_all_full(name, k):
    n = sizes(name)[k]
    F = FRAME_BYTES[name]
    p = packer(name, code=2)  # the plan's own code byte is ignored
    codes = np.random.default_rng(n).integers(0, 3, n)
    buf, offs = stream(name, n, codes)
    want, full, flags, first = model(buf, len(buf), offs, n, F, p.prefix)
    assert full.all() and flags == 0 and np.array_equal(want, codes)
    uni = run(p, buf, len(buf), None, n)
    check(name, uni, n, want, full, 0, NONE)
    ind = run(p, buf, len(buf), offs, n)
    check(name, ind, n, want, full, 0, NONE)
    # all-success bytes: the columns are srpc_gpu_unpack's of the same bytes
    buf0, _ = stream(name, n, np.zeros(n, np.int64))
    got = run(p, buf0, len(buf0), None, n)
    check(name, got, n, np.zeros(n, np.uint8), full, 0, NONE)
    p0 = packer(name, code=0)
    dts = dtypes(p0.schema)
    d_cols = [empty(n * np.dtype(dt).itemsize + 16) for dt in dts]
    st = status_buf()
    assert p0.unpack(dev(np.frombuffer(buf0, np.uint8)) if n else empty(16), len(buf0), n, d_cols, st) == 0
    assert read_status(st) == (0, NONE)
    for c, dt, g in zip(d_cols, dts, got[2]):
        assert np.array_equal(host(c, n * np.dtype(dt).itemsize, dt), g)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("short", ["byte", "frame"])
def test_uniform_short_stream(name, short):
    F = FRAME_BYTES[name]
    n = sizes(name)[4]
    p = packer(name)
    codes = np.random.default_rng(7).integers(0, 3, n)
    buf, offs = stream(name, n, codes)
    buf_len = len(buf) - (1 if short == "byte" else F)
    want, full, flags, first = model(buf, buf_len, offs, n, F, p.prefix)
    nfit = buf_len // F
    assert flags == BOUNDS and first == nfit and full[:nfit].all() and not full[nfit:].any()
    assert (want[nfit:] == NO_CODE).all()
    check(name, run(p, buf, buf_len, None, n), n, want, full, BOUNDS, nfit, want_rc=_lib.SRPC_ERR_BOUNDS)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("n,share", [(1, 0.3), (1, 1.0), (63, 0.3), (63, 1.0), (4097, 0.3), (4097, 1.0),
                                     (NMAX, 0.3), (NMAX, 1.0)])
def test_indexed_with_bare_frames(name, n, share):
    F = FRAME_BYTES[name]
    p = packer(name)
    rng = np.random.default_rng(n + int(10 * share))
    codes = rng.integers(0, 3, n)
    bare = rng.random(n) < share
    special = {int(i): struct.pack(">IB", 1, int(rng.integers(1, 256))) for i in np.flatnonzero(bare)}
    buf, offs = stream(name, n, codes, special)
    want, full, flags, first = model(buf, len(buf), offs, n, F, p.prefix)
    assert np.array_equal(full, ~bare) and flags == 0  # a bare frame is an answer, not an error
    assert all(want[i] == f[4] for i, f in special.items())
    check(name, run(p, buf, len(buf), offs, n), n, want, full, 0, NONE)


BAD = ["wrong_name", "bare_code0", "one_longer", "junk_4k", "cut_last", "swapped", "empty_payload"]


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("case", BAD)
def test_indexed_one_bad_frame(name, case):
    """One bad frame in the middle of the second tile (the last frame for
    cut_last) among full frames of mixed codes and a few bare ones; every full
    frame around it must still decode."""
    F = FRAME_BYTES[name]
    p = packer(name)
    R = sizes(name)[3]
    n = 3 * R + 5
    at = R + R // 2
    rng = np.random.default_rng(BAD.index(case))
    codes = rng.integers(0, 3, n)
    _, rows = reference(name)
    good = rows[0][at].tobytes()
    special = {int(i): struct.pack(">IB", 1, 1) for i in rng.choice(n, 9, replace=False) if abs(int(i) - at) > 1}
    want_at = None  # (code, flag) of the bad frame
    if case == "wrong_name":
        b = bytearray(good)
        b[len(p.prefix) - 1] ^= 0x20
        special[at], want_at = bytes(b), (0, PREFIX)
    elif case == "bare_code0":
        special[at], want_at = struct.pack(">IB", 1, 0), (0, PREFIX)
    elif case == "one_longer":
        special[at], want_at = struct.pack(">I", F - 3) + good[4:] + b"\x00", (0, PREFIX)
    elif case == "junk_4k":
        special[at], want_at = struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091), (7, PREFIX)
    elif case == "empty_payload":
        special[at], want_at = struct.pack(">I", 0), (NO_CODE, BOUNDS)
    buf, offs = stream(name, n, codes, special)
    buf_len = len(buf)
    bad = {at}
    if case == "cut_last":
        special.pop(n - 1, None)
        buf, offs = stream(name, n, codes, special)
        buf_len = len(buf) - 3
        bad, want_at = {n - 1}, None
    elif case == "swapped":
        offs[at], offs[at + 1] = offs[at + 1], offs[at]
        bad = {at - 1, at, at + 1}
    want, full, flags, first = model(buf, buf_len, offs, n, F, p.prefix)
    # the table by hand for the frames this case is about
    for i in range(n):
        if i in bad:
            assert not full[i]
        elif i in special:
            assert not full[i] and want[i] == 1
        else:
            assert full[i] and want[i] == codes[i]
    if want_at:
        assert want[at] == want_at[0] and flags == want_at[1]
    else:
        assert all(want[i] == NO_CODE for i in bad) and flags == BOUNDS
    assert first == min(bad)
    check(name, run(p, buf, buf_len, offs, n), n, want, full, flags, first)


def test_reference_made_square_responses(golden_dir):
    """The 1024 responses the reference server packed (19 bytes each), framed."""
    with open(os.path.join(golden_dir, "square_resp_head1024.bin"), "rb") as f:
        resp = np.frombuffer(f.read(), np.uint8).reshape(1024, 19)
    frames = np.concatenate([np.tile(np.frombuffer(struct.pack(">I", 19), np.uint8), (1024, 1)), resp], axis=1)
    buf = frames.tobytes()
    nums = oracle.square_inputs(1024)
    p = packer("number")
    for offs in (None, (np.arange(1024) * 23).astype(np.uint32)):
        rc, codes, cols, flags, first = run(p, buf, len(buf), offs, 1024)
        assert rc == 0 and (flags, first) == (0, NONE) and not codes.any()
        assert np.array_equal(cols[0], nums * nums)


def test_argument_refusals():
    L = _lib.lib()
    one = (C.c_void_p * 1)(empty(64).data_ptr())
    six = (C.c_void_p * 6)(*[one[0]] * 6)
    codes, buf = empty(64), empty(64)
    sp = GpuPacker(Schema("S", (("s", srpc_amd.STRING),)), framed_response_prefix(srpc_amd.NUMBER))
    assert L.srpc_frames_unpack_replies(sp._h, buf.data_ptr(), 23, None, 1, one, codes.data_ptr(), None,
                                        None) == _lib.SRPC_E_UNSUPPORTED
    bare = GpuPacker(ALL_KINDS)  # no prefix
    assert L.srpc_frames_unpack_replies(bare._h, buf.data_ptr(), 17, None, 1, six, codes.data_ptr(), None,
                                        None) == _lib.SRPC_E_UNSUPPORTED
    tiny = GpuPacker(srpc_amd.NUMBER, b"\0\0\0\5")  # a prefix too short to hold the code byte
    assert L.srpc_frames_unpack_replies(tiny._h, buf.data_ptr(), 8, None, 1, one, codes.data_ptr(), None,
                                        None) == _lib.SRPC_E_UNSUPPORTED
    p = packer("number")
    assert L.srpc_frames_unpack_replies(p._h, buf.data_ptr(), 23, None, 1, one, None, None,
                                        None) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_unpack_replies(p._h, buf.data_ptr(), 23, None, 1, None, codes.data_ptr(), None,
                                        None) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_unpack_replies(None, buf.data_ptr(), 23, None, 1, one, codes.data_ptr(), None,
                                        None) == _lib.SRPC_E_INVALID
    assert L.srpc_frames_unpack_replies(p._h, buf.data_ptr(), 1 << 32, None, 1, one, codes.data_ptr(), None,
                                        None) == _lib.SRPC_E_INVALID
    torch.cuda.synchronize()
    assert (host(codes, 64) == 0xA5).all()  # nothing was launched
