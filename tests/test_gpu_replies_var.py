"""Reply streams of a string response decoded in call order on the device
(srpc_frames_unpack_replies_var, include/srpc_gpu.h), and the request-side
framing of string records (srpc_frames_frame_var).  A generated stub reads one
reply at a time with unpack_response<R> over a string body (packer.hpp:123-137,
216-222); here a whole batch's replies give one code per call, the fixed
columns and the string columns in call order, for any mix of full, bare and
junk frames.

Nothing expected comes from the kernels under test:
- well-formed payloads are the CPU oracle's pack with the response prefix of
  code 0, 1 or 2 (picked per call by a seeded vector), cut into frames with
  BE32s in numpy at record boundaries computed from the string lengths;
- bare and bad frames are literal bytes;
- the expected codes, flags and first bad index are the header's table written
  out below (`model`); the expected fields and strings are the inputs where a
  frame is full, and zero / empty elsewhere;
- the oracle's own unpack of the well-formed payloads reproduces the inputs,
  so the reference alone passes every equality made on full frames."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, Schema, _lib, frame_var

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import MULTIPLE, _rec_offsets, dev, empty, host, read_status, status_buf  # noqa: E402

NO_CODE = 0xFF
PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
STRING = oracle.STRING
SCHEMAS = {
    "text": Schema.of("Text", ("text", "string")),
    "multiple": MULTIPLE,
    # two strings with fixed fields between and after: the gap after the last string is walked
    "mix": Schema.of("Mix", ("a", "string"), ("b", "int32"), ("c", "string"), ("d", "int16")),
}
# frames per workgroup tile and the tile's LDS image bytes, from the library's hook
R, IMAGE = GpuPacker.for_response(SCHEMAS["text"]).replies_var_tile
LONG = IMAGE + 1000


def packer(name, code=0):
    s = SCHEMAS[name]
    p = GpuPacker.for_response(s, code)
    assert p.prefix == oracle.response_prefix(code, s.name) and p.path == srpc_amd.SRPC_PATH_VAR
    return p


def str_fields(name):
    return [f for f, k in enumerate(SCHEMAS[name].kinds) if k == STRING]


def make_lens(name, n, how, seed=0):
    """String lengths per string field (a tuple of tuples, hashable) for a named recipe."""
    rng = np.random.default_rng(seed + n)
    out = []
    for t, _ in enumerate(str_fields(name)):
        if how == "empty":
            ln = np.zeros(n, np.int64)
        elif how == "edges":  # the chunk edges of the copy
            ln = np.array([15, 16, 17, 31, 32, 33], np.int64)[(np.arange(n) + t) % 6]
        else:  # 0..40
            ln = rng.integers(0, 41, n)
        out.append(tuple(int(x) for x in ln))
    return tuple(out)


@functools.lru_cache(maxsize=64)
def batch(name, n, lens):
    """n calls' inputs (cols, offs; read-only) and, per code 0 / 1 / 2, the list
    of their well-formed payloads from the CPU oracle."""
    schema = SCHEMAS[name]
    kinds = schema.kinds
    rng = np.random.default_rng(n * 31 + len(name))
    cols, offs = [], []
    t = 0
    for k in kinds:
        if k == STRING:
            o = np.zeros(n + 1, np.uint64)
            o[1:] = np.cumsum(np.asarray(lens[t], np.uint64))
            total = int(o[n])
            c = ((np.arange(max(total, 1), dtype=np.uint64) * 7 + 3 + 11 * t) % 256).astype(np.uint8)  # every byte value
            t += 1
        else:
            dt = np.dtype(oracle.KIND_DTYPE[k])
            c = rng.integers(0, 256, max(n, 1) * dt.itemsize, dtype=np.uint8).view(dt)[:n].copy()
            o = None
        c.setflags(write=False)
        cols.append(c)
        offs.append(o)
    P = len(oracle.response_prefix(0, schema.name))
    rec = _rec_offsets(kinds, [o if o is not None else None for o in offs], n, P)
    payloads = []
    for code in (0, 1, 2):
        pre = oracle.response_prefix(code, schema.name)
        w = oracle.pack(kinds, [np.array(c) for c in cols], n, pre, [None if o is None else np.array(o) for o in offs])
        assert len(w) == int(rec[n])
        if code == 0:  # once, on the CPU: the reference's unpack reproduces the inputs
            st, back, boffs, consumed, _ = oracle.unpack(kinds, w, n, pre)
            assert st == 0 and consumed == len(w)
            for k, a, b, o, bo in zip(kinds, cols, back, offs, boffs):
                if k == STRING:
                    assert np.array_equal(o, bo) and a[:int(o[n])].tobytes() == b.tobytes()
                else:
                    assert a.tobytes() == b.tobytes()
        payloads.append([w[int(rec[i]):int(rec[i + 1])] for i in range(n)])
    return cols, offs, payloads


def framed(payload: bytes) -> bytes:
    return struct.pack(">I", len(payload)) + payload


def stream(name, n, lens, codes, special=None):
    """Frames of calls 0..n-1: the well-formed frame with codes[i], or
    special[i] (literal bytes).  Returns (bytes, u32 offsets)."""
    _, _, payloads = batch(name, n, lens)
    special = special or {}
    parts = [special[i] if i in special else framed(payloads[codes[i]][i]) for i in range(n)]
    offs = np.zeros(n, np.uint32)
    if n:
        offs[1:] = np.cumsum([len(p) for p in parts[:-1]])
    return b"".join(parts), offs


def model(buf, buf_len, offs, n, prefix, kinds):
    """The per-frame table of include/srpc_gpu.h: (codes, full, flags, first bad)."""
    codes = np.full(n, NO_CODE, np.uint8)
    full = np.zeros(n, bool)
    flags, first = 0, NONE
    P = len(prefix)
    for i in range(n):
        o = int(offs[i])
        e = int(offs[i + 1]) if i + 1 < n else buf_len
        flag = 0
        if o > e or e > buf_len or e - o < 5:
            flag = BOUNDS
        else:
            f, ln = buf[o:e], e - o
            if int.from_bytes(f[:4], "big") != ln - 4:
                flag = BOUNDS
            else:
                codes[i] = f[4]
                if ln == 5 and f[4] != 0:
                    pass  # bare
                elif ln - 4 < P or f[5:4 + P] != prefix[1:]:
                    flag = PREFIX
                else:
                    c, ok = 4 + P, True
                    for k in kinds:
                        if k == STRING:
                            if ln - c < 8:
                                ok = False
                                break
                            sl = int.from_bytes(f[c:c + 8], "little")
                            c += 8
                            if sl > ln - c:
                                ok = False
                                break
                            c += sl
                        else:
                            if oracle.KIND_SIZE[k] > ln - c:
                                ok = False
                                break
                            c += oracle.KIND_SIZE[k]
                    if ok and c == ln:
                        full[i] = True
                    else:
                        flag = BOUNDS
        if flag:
            flags |= flag
            first = min(first, i)
    return codes, full, flags, first


def run(p, buf, buf_len, offs, n, tail=b"", stream_=None, call=True, scratch=None):
    """One call on fresh 0xA5-filled outputs -> (codes, cols, str offs, flags, first);
    the frames' allocation holds `tail` after buf_len (scratch: the caller's own,
    which may be larger than the call needs, instead of a fresh one)."""
    kinds = p.schema.kinds
    d_buf = dev(np.frombuffer(buf + tail, np.uint8)) if buf or tail else empty(16)
    d_offs = dev(offs) if n else empty(16)
    d_cols, d_so = [], []
    for k in kinds:
        if k == STRING:
            d_cols.append(empty(buf_len + 16))
            d_so.append(empty(8 * (n + 1) + 16))
        else:
            d_cols.append(empty(n * oracle.KIND_SIZE[k] + 16))
            d_so.append(None)
    d_codes = empty(n + 16)
    sb = p.replies_var_scratch_bytes(n)
    scratch = empty(sb) if scratch is None else scratch
    behind = scratch[sb:].clone()
    st = status_buf()
    args = (d_buf, buf_len, d_offs, n, d_cols, d_so, d_codes, scratch, sb, st)
    if call:
        p.unpack_replies_var(*args)
        assert torch.equal(scratch[sb:], behind), "wrote past the scratch"
    else:
        return args

    return collect(p, args)


def collect(p, args):
    _, buf_len, _, n, d_cols, d_so, d_codes, _, _, st = args
    kinds = p.schema.kinds
    flags, first = read_status(st)
    cols, soffs = [], []
    for k, c, so in zip(kinds, d_cols, d_so):
        if k == STRING:
            o = host(so, 8 * (n + 1), np.uint64)
            assert (host(so, 8 * (n + 1) + 16)[8 * (n + 1):] == 0xA5).all()
            assert o[0] == 0 and (np.diff(o.astype(np.int64)) >= 0).all() and int(o[n]) <= buf_len
            allb = host(c, buf_len + 16)
            assert (allb[int(o[n]):] == 0xA5).all(), "wrote past the string column's offs[n]"
            cols.append(allb[:int(o[n])].copy())
            soffs.append(o)
        else:
            sz = oracle.KIND_SIZE[k]
            allb = host(c, n * sz + 16)
            assert (allb[n * sz:] == 0xA5).all(), "wrote past a column's n elements"
            cols.append(allb[:n * sz].view(oracle.KIND_DTYPE[k]).copy())
            soffs.append(None)
    assert (host(d_codes, n + 16)[n:] == 0xA5).all()
    return host(d_codes, n).copy(), cols, soffs, flags, first


def check(name, n, lens, got, want_codes, full, want_flags, want_first):
    codes, cols, soffs, flags, first = got
    ins, ioffs, _ = batch(name, n, lens)
    assert np.array_equal(codes, want_codes)
    for k, c, so, x, xo in zip(SCHEMAS[name].kinds, cols, soffs, ins, ioffs):
        if k == STRING:
            ln = np.where(full, np.diff(xo.astype(np.int64)), 0)
            want_o = np.zeros(n + 1, np.uint64)
            want_o[1:] = np.cumsum(ln)
            assert np.array_equal(so, want_o)
            want_c = b"".join(x[int(xo[i]):int(xo[i + 1])].tobytes() for i in np.flatnonzero(full))
            assert c.tobytes() == want_c
        else:
            assert np.array_equal(c, np.where(full, x[:n], 0).astype(x.dtype))
    assert (flags, first) == (want_flags, want_first)


def decode_and_check(name, n, lens, codes, special=None, buf_len_cut=0, offs_edit=None, scratch=None):
    p = packer(name, code=2)  # the plan's own code byte is ignored
    buf, offs = stream(name, n, lens, codes, special)
    if offs_edit:
        offs_edit(offs)
    buf_len = len(buf) - buf_len_cut
    want = model(buf, buf_len, offs, n, p.prefix, p.schema.kinds)
    got = run(p, buf, buf_len, offs, n, scratch=scratch)
    check(name, n, lens, got, *want)
    return want


def test_tile_hook():
    for name in SCHEMAS:
        assert packer(name).replies_var_tile == (R, IMAGE)
    assert R >= 64 and R % 64 == 0 and IMAGE >= 4096 and IMAGE % 16 == 0


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, R - 1, R, R + 1, 3 * R + 5])
def test_frame_counts_mixed_codes_and_bare(name, n):
    lens = make_lens(name, n, "0-40")
    codes = np.random.default_rng(n).integers(0, 3, n)
    codes_want, full, flags, first = decode_and_check(name, n, lens, codes)
    assert full.all() and flags == 0 and first == NONE and np.array_equal(codes_want, codes)
    # every 7th frame bare: an answer, not an error
    special = {i: struct.pack(">IB", 1, 1 + i % 255) for i in range(3, n, 7)}
    codes_want, full, flags, first = decode_and_check(name, n, lens, codes, special)
    assert flags == 0 and all(not full[i] and codes_want[i] == 1 + i % 255 for i in special)
    assert all(full[i] for i in range(n) if i not in special)


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("how", ["empty", "edges"])
def test_string_length_edges(name, how):
    n = R + 1
    lens = make_lens(name, n, how)
    codes = np.random.default_rng(5).integers(0, 3, n)
    _, full, flags, _ = decode_and_check(name, n, lens, codes)
    assert full.all() and flags == 0


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("where", ["first", "middle", "last", "two"])
def test_long_strings_push_frames_out_of_the_image(name, where):
    """A string longer than the tile's image among short ones, in the second of
    three tiles: the frames after it lie outside the image."""
    n = 2 * R + 3
    at = {"first": [R], "middle": [R + R // 2], "last": [2 * R - 1], "two": [R + 3, R + R // 2]}[where]
    lens = [list(l) for l in make_lens(name, n, "0-40")]
    for i in at:
        lens[-1][i] = LONG  # the schema's last string field
    lens = tuple(tuple(l) for l in lens)
    codes = np.random.default_rng(len(where)).integers(0, 3, n)
    special = {i: struct.pack(">IB", 1, 9) for i in (R + 1, 2 * R - 2)}  # bare frames around them
    _, full, flags, _ = decode_and_check(name, n, lens, codes, special)
    assert flags == 0 and full.sum() == n - 2 and all(full[i] for i in at)


BAD = ["wrong_name", "junk_4k", "bare_code0", "len_past_end", "walk_short", "len_2_63", "len_max", "four_bytes",
       "be32_off", "swapped", "cut_last"]


def first_len_at(name):
    """Frame offset of the first string's length word."""
    s = SCHEMAS[name]
    at = 4 + len(oracle.response_prefix(0, s.name))
    for k in s.kinds:
        if k == STRING:
            return at
        at += oracle.KIND_SIZE[k]


@pytest.mark.parametrize("name", sorted(SCHEMAS))
@pytest.mark.parametrize("case", BAD)
def test_one_bad_frame(name, case):
    """One bad frame in the middle of the second tile (the last frame for
    cut_last) among full frames of mixed codes and a few bare ones; every frame
    around it must still decode."""
    n = 3 * R + 5
    at = R + R // 2
    lens = make_lens(name, n, "0-40", seed=1)
    rng = np.random.default_rng(BAD.index(case))
    codes = rng.integers(0, 3, n)
    codes[at] = 2
    _, _, payloads = batch(name, n, lens)
    good = framed(payloads[2][at])
    P = len(oracle.response_prefix(0, SCHEMAS[name].name))
    la = first_len_at(name)
    special = {int(i): struct.pack(">IB", 1, 1) for i in rng.choice(n, 9, replace=False)
               if abs(int(i) - at) > 1 and int(i) != n - 1}
    want_at, bad, cut, edit = None, {at}, 0, None

    def with_len(v):
        b = bytearray(good)
        b[la:la + 8] = struct.pack("<Q", v)
        return bytes(b)

    if case == "wrong_name":
        b = bytearray(good)
        b[4 + P - 1] ^= 0x20
        special[at], want_at = bytes(b), (2, PREFIX)
    elif case == "junk_4k":
        special[at], want_at = struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091), (7, PREFIX)
    elif case == "bare_code0":
        special[at], want_at = struct.pack(">IB", 1, 0), (0, PREFIX)
    elif case == "len_past_end":  # the first string would end one byte past the frame's end
        special[at], want_at = with_len(len(good) - (la + 8) + 1), (2, BOUNDS)
    elif case == "walk_short":  # a well-formed walk that ends one byte before the frame's end
        special[at], want_at = struct.pack(">I", len(good) - 3) + good[4:] + b"\x00", (2, BOUNDS)
    elif case == "len_2_63":
        special[at], want_at = with_len(1 << 63), (2, BOUNDS)
    elif case == "len_max":
        special[at], want_at = with_len((1 << 64) - 1), (2, BOUNDS)
    elif case == "four_bytes":
        special[at], want_at = struct.pack(">I", 0), (NO_CODE, BOUNDS)
    elif case == "be32_off":
        special[at], want_at = struct.pack(">I", len(good) - 3) + good[4:], (NO_CODE, BOUNDS)
    elif case == "swapped":
        def edit(offs):
            offs[at], offs[at + 1] = offs[at + 1], offs[at]
        bad = {at - 1, at, at + 1}
    elif case == "cut_last":
        cut, bad = 3, {n - 1}
    want, full, flags, first = decode_and_check(name, n, lens, codes, special, cut, edit)
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


@pytest.mark.parametrize("name", ["multiple", "mix"])
def test_nothing_past_buf_len_is_read(name):
    """The same stream followed by two different garbage tails inside the same
    allocation: byte-identical results.  The last frame is a full frame cut
    short with its BE32 corrected, so its last field or chars would come from
    the tail -- which first holds exactly the bytes cut off -- if the bound
    slipped."""
    n = R + 7
    lens = make_lens(name, n, "0-40", seed=2)
    lens = tuple(l[:n - 1] + (40,) for l in lens)  # the last call's strings are not empty
    codes = np.random.default_rng(3).integers(0, 3, n)
    p = packer(name)
    _, _, payloads = batch(name, n, lens)
    last = payloads[codes[n - 1]][n - 1]
    for cut in (0, 1, 9):
        special = {n - 1: framed(last[:len(last) - cut])} if cut else None
        buf, offs = stream(name, n, lens, codes, special)
        tails = [last[len(last) - cut:] + bytes([0x00]) * 4096, bytes([0xFF]) * (4096 + cut)]
        a = run(p, buf, len(buf), offs, n, tail=tails[0])
        b = run(p, buf, len(buf), offs, n, tail=tails[1])
        assert np.array_equal(a[0], b[0]) and a[3:] == b[3:]
        for x, y in zip(a[1], b[1]):
            assert x.tobytes() == y.tobytes()
        want = model(buf, len(buf), offs, n, p.prefix, p.schema.kinds)
        check(name, n, lens, a, *want)
        assert want[1][:n - 1].all() and bool(want[1][n - 1]) == (cut == 0)
        assert want[0][n - 1] == codes[n - 1] and want[2] == (BOUNDS if cut else 0)


def test_overlapping_frames_stay_inside_the_string_column():
    """Offsets out of order that make one full frame count many times: its
    chars total more than buf_len, the room a string column has.  The codes and
    offsets follow the table; nothing at or past buf_len is written."""
    name, n = "text", 2 * R + 1
    p = packer(name)
    _, _, payloads = batch(name, 1, ((300,),))
    buf = framed(payloads[0][0])
    text = payloads[0][0][-300:]
    offs = np.where(np.arange(n) % 2 == 0, 0, len(buf)).astype(np.uint32)  # even frames: the whole stream
    codes_want, full, flags, first = model(buf, len(buf), offs, n, p.prefix, p.schema.kinds)
    assert full[0::2].all() and not full[1::2].any() and (flags, first) == (BOUNDS, 1)
    args = run(p, buf, len(buf), offs, n, call=False)
    p.unpack_replies_var(*args)
    assert np.array_equal(host(args[6], n), codes_want) and read_status(args[9]) == (BOUNDS, 1)
    want_o = np.zeros(n + 1, np.uint64)
    want_o[1:] = np.cumsum(np.where(full, 300, 0))
    assert np.array_equal(host(args[5][0], 8 * (n + 1), np.uint64), want_o) and int(want_o[n]) > len(buf)
    col = host(args[4][0], len(buf) + 16)
    assert col[:len(buf)].tobytes() == (text * (R + 1))[:len(buf)] and (col[len(buf):] == 0xA5).all()


def test_argument_refusals():
    L = _lib.lib()
    f = L.srpc_frames_unpack_replies_var
    p = packer("multiple")
    n = 4
    bufs = [empty(256) for _ in range(4)]
    so, codes, buf, offs = empty(64), empty(64), empty(256), dev(np.arange(4, dtype=np.uint32) * 40)
    sb = p.replies_var_scratch_bytes(n)
    scratch = empty(sb + 16)
    cols = (C.c_void_p * 4)(*[b.data_ptr() for b in bufs])
    soffs = (C.c_void_p * 4)(None, None, None, so.data_ptr())

    def call(plan=p, cols=cols, soffs=soffs, scratch_ptr=None, scratch_bytes=sb):
        return f(plan._h, buf.data_ptr(), 160, offs.data_ptr(), n, cols, soffs, codes.data_ptr(), None,
                 scratch.data_ptr() if scratch_ptr is None else scratch_ptr, scratch_bytes, None)

    fixed = GpuPacker.for_response(srpc_amd.NUMBER)
    assert call(plan=fixed) == _lib.SRPC_E_UNSUPPORTED
    assert call(plan=GpuPacker(MULTIPLE)) == _lib.SRPC_E_UNSUPPORTED  # a prefix under 1 byte
    out = C.c_uint64()
    assert L.srpc_frames_replies_var_scratch_bytes(fixed._h, n, C.byref(out)) == _lib.SRPC_E_UNSUPPORTED
    assert call(scratch_bytes=sb - 1) == _lib.SRPC_E_CAPACITY
    assert call(scratch_ptr=scratch.data_ptr() + 4) == _lib.SRPC_E_ALIGN
    for f_bad in range(4):  # a misaligned column, fixed or string
        bad = (C.c_void_p * 4)(*[b.data_ptr() + (8 if i == f_bad else 0) for i, b in enumerate(bufs)])
        assert call(cols=bad) == _lib.SRPC_E_ALIGN
    assert call(soffs=(C.c_void_p * 4)(None, None, None, so.data_ptr() + 4)) == _lib.SRPC_E_ALIGN
    assert call(soffs=(C.c_void_p * 4)(None, None, None, None)) == _lib.SRPC_E_INVALID
    assert f(p._h, buf.data_ptr() + 8, 152, offs.data_ptr(), n, cols, soffs, codes.data_ptr(), None,
             scratch.data_ptr(), sb, None) == _lib.SRPC_E_ALIGN
    torch.cuda.synchronize()
    assert (host(codes, 64) == 0xA5).all() and (host(so, 64) == 0xA5).all()  # nothing was launched


def test_captured_and_replayed():
    name, n = "mix", R + 9
    lens = make_lens(name, n, "0-40", seed=4)
    codes = np.random.default_rng(8).integers(0, 3, n)
    special = {i: struct.pack(">IB", 1, 1) for i in range(2, n, 7)}
    p = packer(name)
    buf, offs = stream(name, n, lens, codes, special)
    want = model(buf, len(buf), offs, n, p.prefix, p.schema.kinds)
    args = run(p, buf, len(buf), offs, n, call=False)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        p.unpack_replies_var(*args, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert (host(args[6], n) == 0xA5).all()  # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    check(name, n, lens, collect(p, args), *want)


@pytest.mark.parametrize("n,how", [(0, "0-40"), (1, "0-40"), (65, "0-40"), (65, "empty"), (65, "long")])
def test_frame_var_equals_numpy_framing(n, how):
    """pack_var's records framed on the device == the oracle's records framed in numpy."""
    name = "multiple"
    schema = SCHEMAS[name]
    if how == "long":
        ll = [list(l) for l in make_lens(name, n, "0-40")]
        ll[0][n // 2] = LONG
        lens = tuple(tuple(l) for l in ll)
    else:
        lens = make_lens(name, n, how)
    cols, offs, _ = batch(name, n, lens)
    method = "Echo_servicer::echo"
    pre = oracle.request_prefix(method, schema.name)
    p = GpuPacker.for_request(schema, method)
    assert p.prefix == pre
    w = oracle.pack(schema.kinds, [np.array(c) for c in cols], n, pre, [None if o is None else np.array(o) for o in offs])
    rec = _rec_offsets(schema.kinds, offs, n, len(pre))
    assert len(w) == int(rec[n])
    want = b"".join(framed(w[int(rec[i]):int(rec[i + 1])]) for i in range(n))
    total = len(w)
    d_cols = [dev(c) for c in cols]
    d_offs = [None if o is None else dev(o) for o in offs]
    wire, d_rec = empty(total + 16), empty(8 * (n + 1))
    sb = p.var_scratch_bytes(n, total)
    scratch = empty(sb + 16)
    st = status_buf()
    p.pack_var(d_cols, d_offs, n, wire, total, d_rec, scratch, sb, st)
    out = empty(len(want) + 16)
    frame_var(wire, d_rec, n, out, len(want), st)
    assert read_status(st) == (0, NONE)
    got = host(out, len(want) + 16)
    assert got[:len(want)].tobytes() == want and (got[len(want):] == 0xA5).all()
    if n:  # an output one byte too small: the last frame is not written, BOUNDS says which
        out2 = empty(len(want) + 16)
        frame_var(wire, d_rec, n, out2, len(want) - 1, st)
        last = len(want) - (4 + int(rec[n] - rec[n - 1]))
        got2 = host(out2, len(want) + 16)
        assert read_status(st) == (BOUNDS, n - 1)
        assert got2[:last].tobytes() == want[:last] and (got2[last:] == 0xA5).all()
