"""The frame decoders on frames just under 2^32 (include/srpc_gpu.h: the frame
calls admit buf_len up to 2^32 - 1 with uint32_t offsets; an `o + len` computed
in 32 bits goes wrong only for frames in the top few KiB of that range, where no
other test puts one).

The buffer is torch.empty(2^32 - 1): it only provides the address range and is
never filled as a whole.  A handful of frames sit at offset 0 and up; the last
of them (a frame no decoder accepts) has the whole gap as its extent; the rest
are copied into the buffer's last bytes, so that their offsets lie in the top
64 KiB below 2^32 and the last frame ends exactly at buf_len = 2^32 - 1, the
largest value admitted.  One more offset equal to buf_len follows (an empty
frame).  Among the top frames are hostile ones: BE32 lengths whose `o + 4 + len`
passes 2^32 (to 0, to the frame's own start, as far as it goes) and, for the
string decoder, string lengths whose end passes 2^32 or whose low 32 bits are
the true length.

Frames, expectations and checks are those of the modules named in each test:
their streams (literal bytes and oracle packs), their host models -- which work
in Python integers on a host image of the same sparse buffer -- and their
comparisons.  Only the upload differs: the two ends of the buffer.

What was read before the first run (no decoder may read at or past buf_len, and none may
form `o + 4 + len` in 32 bits):
- k_unpack_replies, reply_var_stage (frames.hip): lo[] holds uint32_t offsets, widened to
  uint64_t o0, oe, o, e before every test; a tile stages [o0 & ~15, end) with end = oe if
  o0 <= oe <= buf_len, else buf_len, at most the image's capacity; a frame is read only after
  `o <= e && e <= buf_len && e - o >= 5`, its BE32 is compared with e - o - 4 (never added to
  o), and a frame outside the image is read at buf + o for at most e - o bytes.
- k_replies_var_parse / _copy: the same offsets and tests; a string length is compared with
  the bytes the frame has left (sl > ln - c), in 64 bits; chars are copied from inside [o, e).
- k_classify: end = offs[i + 1] or buf_len, `inside = o <= end && end <= buf_len`; the prefix
  and BE32 are read only for a frame that is inside and long enough; the gathers copy
  record_bytes (fixed) or [o + 4, end) (string) of frames classify accepted.
- mv_parse_tile / mv_parse_lane (mixed_var_tile.h, the reply decode of mixed_legs.hip): o and e
  widened, `o <= e && e <= buf_len`, e - o >= 5, BE32 against len - 4; the staged span is
  clamped to buf_len as above.
- k_req_legs (mixed_req_legs.hip), req_offsets / req_stage / req_parse_lane (mixed_common.h),
  mrv_classify (mixed_req_var_tile.h): lo[] as above, req_stage clamps its span to buf_len, a
  fixed frame is taken only if `o <= buf_len && F <= buf_len - o`, a string frame only if
  `o <= end && end <= buf_len`, and is walked inside [o, end).
"""
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests import test_gpu_frames as TF  # noqa: E402
from tests import test_gpu_replies as TR  # noqa: E402
from tests import test_gpu_replies_aos as TA  # noqa: E402
from tests import test_gpu_replies_var as TV  # noqa: E402
from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402

DEV = torch.device("cuda:0")
BUF_LEN = 2**32 - 1
GUARD = 1 << 20
PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
N_LOW = 40      # frames from offset 0 (the last one spans the gap)
N_TOP = 1200    # frames in the buffer's last bytes: more than one tile of every decoder
N_TOP_LONG = 700  # ... of the longer frames (string replies, requests): still under 64 KiB


class TopBuffer:
    """Frames 0 .. k-1 from offset 0, frames k .. n-1 ending exactly at BUF_LEN, then
    (`empty_last`) one more offset equal to BUF_LEN.  `image` is the host's view of the
    same bytes (pages never written read as zero and cost nothing)."""

    def __init__(self, stream, offs, k, empty_last=True):
        offs = np.asarray(offs, np.int64)
        cut = int(offs[k])
        low, top = stream[:cut], stream[cut:]
        self.shift = BUF_LEN - len(stream)
        assert len(top) <= 65536 and self.shift > 2**31, "the top frames lie in the last 64 KiB"
        new = offs.copy()
        new[k:] += self.shift
        if empty_last:
            new = np.append(new, BUF_LEN)
        self.n = len(new)
        self.offs = new.astype(np.uint32)
        assert np.array_equal(self.offs.astype(np.int64), new) and int(self.offs[k]) >= 2**32 - 65536
        host_img = np.zeros(BUF_LEN, np.uint8)
        host_img[:cut] = np.frombuffer(low, np.uint8)
        host_img[BUF_LEN - len(top):] = np.frombuffer(top, np.uint8)
        self.np_image = host_img
        self.image = memoryview(host_img)
        self.top_at = BUF_LEN - len(top)
        self.d_buf = torch.empty(BUF_LEN, dtype=torch.uint8, device=DEV)
        self.d_buf[:cut].copy_(torch.from_numpy(np.frombuffer(low, np.uint8).copy()))
        self.d_buf[BUF_LEN - len(top):].copy_(torch.from_numpy(np.frombuffer(top, np.uint8).copy()))
        self.d_offs = dev(self.offs)

    def bytes_at(self, o, n):
        return self.np_image[o:o + n]


def hostile_be32(at_index, offs_guess):
    """Literal frames whose BE32 length makes `o + 4 + len` pass 2^32; the offsets are
    known only after the stream is laid out, so the lengths are the worst in general
    and, where `offs_guess` gives the frame's final offset, exact wraps."""
    o = offs_guess
    return {
        at_index: struct.pack(">I", 0xFFFFFFFF) + b"\x01" + b"\x00" * 11,          # as far as it goes
        at_index + 7: struct.pack(">I", (2**32 - o(at_index + 7) - 4) % 2**32) + b"\x02" + b"\x00" * 11,  # to 0
        at_index + 19: struct.pack(">I", (2**32 - 4) % 2**32) + b"\x03" + b"\x00" * 11,  # o + 4 + len = o
        at_index + 31: struct.pack(">I", (2**32 - o(at_index + 31) + 11) % 2**32) + b"\x04" + b"\x00" * 11,  # to 15
    }


def _fixed_stream(name, n, seed):
    """test_gpu_replies' frames of calls 0 .. n-1 (full frames of codes 0 / 1 / 2, bare
    error frames, junk, the hostile BE32s) split at N_LOW; the gap frame is frame N_LOW - 1."""
    F = TR.FRAME_BYTES[name]
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 3, n)
    special = {int(i): struct.pack(">IB", 1, int(rng.integers(1, 256)))
               for i in np.flatnonzero(rng.random(n) < 0.2)}
    special[N_LOW - 1] = struct.pack(">IB", 1, 9)          # bare where it stands, not with the gap behind it
    special[N_LOW + 100] = struct.pack(">I", 1020) + b"\x07" + rng.bytes(1019)   # junk with a code
    b = bytearray(TR.reference(name)[1][0][N_LOW + 150].tobytes())
    b[len(TR.oracle_prefix(TR.SCHEMAS[name], 0)) - 1] ^= 0x20                   # a wrong name
    special[N_LOW + 150] = bytes(b)
    special[N_LOW + 151] = struct.pack(">I", 0)                                  # an empty payload
    special.pop(n - 1, None)  # the last frame is a full one (ends exactly at buf_len)
    hostile_at = N_LOW + 300
    for i in (0, 7, 19, 31):
        special.pop(hostile_at + i, None)
    # two passes: the hostile lengths need the frames' final offsets
    guess = lambda i: 0  # noqa: E731
    for _ in range(2):
        sp = dict(special)
        sp.update(hostile_be32(hostile_at, guess))
        buf, offs = TR.stream(name, n, codes, sp)
        shift = BUF_LEN - len(buf)
        guess = lambda i, offs=offs, shift=shift: int(offs[i]) + shift  # noqa: E731
    return buf, offs, F


def _check_hostile(tb, hostile_at):
    """The hostile frames are what their comments say, at the offsets they got."""
    o7, o19, o31 = (int(tb.offs[hostile_at + i]) for i in (7, 19, 31))
    be = lambda o: int.from_bytes(tb.image[o:o + 4], "big")  # noqa: E731
    assert (o7 + 4 + be(o7)) == 2**32 and (o19 + 4 + be(o19)) % 2**32 == o19 and (o31 + 4 + be(o31)) % 2**32 == 15
    assert be(int(tb.offs[hostile_at])) == 0xFFFFFFFF


@pytest.mark.parametrize("name", sorted(TR.SCHEMAS))
def test_unpack_replies_top(name):
    """srpc_frames_unpack_replies; frames, model and check of tests/test_gpu_replies.py."""
    n = N_LOW + N_TOP
    buf, offs, F = _fixed_stream(name, n, 5)
    tb = TopBuffer(buf, offs, N_LOW)
    _check_hostile(tb, N_LOW + 300)
    p = TR.packer(name)
    want, full, flags, first = TR.model(tb.image, BUF_LEN, tb.offs, tb.n, F, p.prefix)
    # the premises, from the table alone
    assert first == N_LOW - 1 and not full[N_LOW - 1] and want[N_LOW - 1] == TR.NO_CODE   # the gap frame
    assert full[n - 1] and int(tb.offs[n - 1]) + F == BUF_LEN                              # ends at buf_len
    assert want[n] == TR.NO_CODE and int(tb.offs[n]) == BUF_LEN                            # the empty frame
    assert full[:N_LOW - 1].sum() > 20 and full[N_LOW:].sum() > 800 and flags == PREFIX | BOUNDS
    for i in (0, 7, 19, 31):
        assert want[N_LOW + 300 + i] == TR.NO_CODE and not full[N_LOW + 300 + i]
    dts = TR.dtypes(p.schema)
    d_cols = [empty(tb.n * np.dtype(dt).itemsize + 16) for dt in dts]
    d_codes = empty(tb.n + 16)
    st = status_buf()
    rc = p.unpack_replies(tb.d_buf, BUF_LEN, tb.d_offs, tb.n, d_cols, d_codes, st)
    gflags, gfirst = read_status(st)
    cols = [host(c, tb.n * np.dtype(dt).itemsize, dt) for c, dt in zip(d_cols, dts)]
    for c, dt in zip(d_cols, dts):
        assert (host(c, tb.n * np.dtype(dt).itemsize + 16)[-16:] == 0xA5).all(), "wrote past a column's n elements"
    assert (host(d_codes, tb.n + 16)[tb.n:] == 0xA5).all()
    print(f"FTOP unpack_replies {name}: n={tb.n} first top offset=2^32-{2**32 - int(tb.offs[N_LOW])} "
          f"full={int(full.sum())} flags={gflags} first={gfirst}")
    TR.check(name, (rc, host(d_codes, tb.n), cols, gflags, gfirst), tb.n, want, full, flags, first)


@pytest.mark.parametrize("name,lay", TA.CASES)
def test_unpack_replies_aos_top(name, lay):
    """srpc_frames_unpack_replies_aos; layouts, fill and expected structs of tests/test_gpu_replies_aos.py."""
    n = N_LOW + N_TOP
    buf, offs, F = _fixed_stream(name, n, 6)
    tb = TopBuffer(buf, offs, N_LOW)
    p = TR.packer(name)
    want, full, flags, first = TR.model(tb.image, BUF_LEN, tb.offs, tb.n, F, p.prefix)
    assert first == N_LOW - 1 and full[n - 1] and want[n] == TR.NO_CODE and full[N_LOW:].sum() > 800
    stride, offsets = TA.LAYOUTS[name][lay]
    d_recs = empty(tb.n * stride + 16)
    d_codes = empty(tb.n + 16)
    st = status_buf()
    rc = p.unpack_replies_aos(tb.d_buf, BUF_LEN, tb.d_offs, tb.n, d_recs, stride, offsets,
                              TA.fill_of(name, lay).tobytes(), d_codes, st)
    assert rc == 0 and read_status(st) == (flags, first)
    assert (host(d_recs, tb.n * stride + 16)[tb.n * stride:] == 0xA5).all(), "wrote past the array's n structs"
    assert (host(d_codes, tb.n + 16)[tb.n:] == 0xA5).all()
    assert np.array_equal(host(d_codes, tb.n), want)
    recs = host(d_recs, tb.n * stride).reshape(tb.n, stride)
    exp = TA.expected_structs(name, lay, tb.n, full)
    bad = np.flatnonzero((recs != exp).any(axis=1))
    assert bad.size == 0, f"struct {bad[0]}: {recs[bad[0]].tolist()} != {exp[bad[0]].tolist()}"


def _guarded_column(nbytes):
    """A string column of nbytes (never filled as a whole) between two 1 MiB guards; its
    first 2 MiB are 0xA5 too, so a write past offs[n] is seen."""
    raw = torch.empty(2 * GUARD + nbytes + 16, dtype=torch.uint8, device=DEV)
    raw[:3 * GUARD].fill_(0xA5)
    raw[GUARD + nbytes:].fill_(0xA5)
    return raw, raw[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("name", ["multiple", "mix"])
def test_unpack_replies_var_top(name):
    """srpc_frames_unpack_replies_var; frames, model and check of tests/test_gpu_replies_var.py.
    Every string column has buf_len bytes, as the header asks."""
    n = N_LOW + N_TOP_LONG
    assert N_TOP_LONG > 2 * TV.R, "more than two tiles of frames in the top range"
    lens = TV.make_lens(name, n, "0-40", seed=3)
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 3, n)
    p = TV.packer(name, code=2)
    P = len(p.prefix)
    _, _, payloads = TV.batch(name, n, lens)
    special = {int(i): struct.pack(">IB", 1, int(rng.integers(1, 256)))
               for i in np.flatnonzero(rng.random(n) < 0.15)}
    special[N_LOW - 1] = struct.pack(">IB", 1, 9)
    at = TV.first_len_at(name)   # the first string's length word, from the frame's start

    def relen(i, value):
        f = bytearray(TV.framed(payloads[0][i]))
        f[at:at + 8] = struct.pack("<Q", value % 2**64)
        return bytes(f)

    h = N_LOW + 400
    true_len = lambda i: int.from_bytes(TV.framed(payloads[0][i])[at:at + 8], "little")  # noqa: E731
    guess = lambda i: 0  # noqa: E731
    for _ in range(2):
        sp = dict(special)
        sp[h] = relen(h, 2**32 + true_len(h))                    # the low 32 bits are the true length
        sp[h + 3] = relen(h + 3, 2**32 - (guess(h + 3) + at + 8))  # the string's end is 2^32: 0 in 32 bits
        sp[h + 11] = relen(h + 11, 2**32 - (guess(h + 11) + at + 8) + true_len(h + 11))  # ... wraps onto its true end
        sp[h + 17] = relen(h + 17, 2**64 - 8)
        sp[h + 23] = struct.pack(">I", 0xFFFFFFFF) + b"\x01" + b"\x00" * 11
        sp[n - 1] = TV.framed(payloads[1][n - 1])                # a full frame ends exactly at buf_len
        buf, offs = TV.stream(name, n, lens, codes, sp)
        shift = BUF_LEN - len(buf)
        guess = lambda i, offs=offs, shift=shift: int(offs[i]) + shift  # noqa: E731
    tb = TopBuffer(buf, offs, N_LOW)
    assert guess(h + 3) == int(tb.offs[h + 3])
    kinds = p.schema.kinds
    want, full, flags, first = TV.model(tb.image, BUF_LEN, tb.offs, tb.n, p.prefix, kinds)
    assert first == N_LOW - 1 and full[n - 1] and want[n] == TV.NO_CODE and full[N_LOW:].sum() > 400
    for i in (h, h + 3, h + 11, h + 17, h + 23):
        assert not full[i], i
    d_cols, d_so, raws = [], [], []
    for k in kinds:
        if k == oracle.STRING:
            raw, view = _guarded_column(BUF_LEN)
            raws.append(raw)
            d_cols.append(view)
            d_so.append(empty(8 * (tb.n + 1) + 16))
        else:
            d_cols.append(empty(tb.n * oracle.KIND_SIZE[k] + 16))
            d_so.append(None)
    d_codes = empty(tb.n + 16)
    sb = p.replies_var_scratch_bytes(tb.n)
    scratch = empty(sb + 16)
    st = status_buf()
    p.unpack_replies_var(tb.d_buf, BUF_LEN, tb.d_offs, tb.n, d_cols, d_so, d_codes, scratch, sb, st)
    gflags, gfirst = read_status(st)
    assert (host(scratch, sb + 16)[sb:] == 0xA5).all(), "wrote past the scratch"
    cols, soffs = [], []
    for k, c, so in zip(kinds, d_cols, d_so):
        if k == oracle.STRING:
            o = host(so, 8 * (tb.n + 1), np.uint64)
            assert (host(so, 8 * (tb.n + 1) + 16)[8 * (tb.n + 1):] == 0xA5).all()
            assert o[0] == 0 and (np.diff(o.astype(np.int64)) >= 0).all() and int(o[tb.n]) < GUARD
            head = c[:2 * GUARD].cpu().numpy()
            assert (head[int(o[tb.n]):] == 0xA5).all(), "wrote past the string column's offs[n]"
            cols.append(head[:int(o[tb.n])].copy())
            soffs.append(o)
        else:
            sz = oracle.KIND_SIZE[k]
            allb = host(c, tb.n * sz + 16)
            assert (allb[tb.n * sz:] == 0xA5).all(), "wrote past a column's n elements"
            cols.append(allb[:tb.n * sz].view(oracle.KIND_DTYPE[k]).copy())
            soffs.append(None)
    for raw in raws:
        assert not bool((raw[:GUARD] != 0xA5).any()) and not bool((raw[GUARD + BUF_LEN:] != 0xA5).any()), "a guard"
    assert (host(d_codes, tb.n + 16)[tb.n:] == 0xA5).all()
    # test_gpu_replies_var.check over the n calls that have inputs, then the empty frame
    codes_got = host(d_codes, tb.n).copy()
    assert codes_got[n] == TV.NO_CODE and not full[n]
    for o in soffs:
        if o is not None:
            assert o[n + 1] == o[n]
    for k, c in zip(kinds, cols):
        if k != oracle.STRING:
            assert c[n] == 0
    got = (codes_got[:n], [c if k == oracle.STRING else c[:n] for k, c in zip(kinds, cols)],
           [None if o is None else o[:n + 1] for o in soffs], gflags, gfirst)
    print(f"FTOP unpack_replies_var {name}: n={tb.n} full={int(full.sum())} flags={gflags} first={gfirst}")
    TV.check(name, n, lens, got, want[:n], full[:n], flags, first)


def test_classify_gather_top():
    """srpc_frames_classify + _gather + _gather_var over fixed and string-bodied methods;
    frames and expectations of tests/test_gpu_frames.py (_mixed_var_frames and
    test_string_methods_classify_gather_pack_scatter)."""
    n = N_LOW + N_TOP_LONG
    rng = np.random.default_rng(21)
    buf, offs, want, _ = TF._mixed_var_frames(n, rng, 0.25, var_frac=0.35)
    k = int(np.flatnonzero(want[:N_LOW] == TF.UNKNOWN)[-1]) + 1   # the gap frame: a foreign one
    assert k > 8
    K = len(TF.METHODS)
    tb = TopBuffer(buf, offs, k)
    want = np.append(want, TF.UNKNOWN).astype(np.uint8)           # the empty frame
    KV = len(TF.VAR_METHODS)
    KT = K + KV
    fixed = [(srpc_amd.GpuPacker(s, srpc_amd.framed_request_prefix(s, m)), rb) for s, m, rb in TF.METHODS]
    var = [(srpc_amd.GpuPacker.for_request(s, m), 0) for s, m in TF.VAR_METHODS]
    fc = srpc_amd.FrameClassifier(fixed + var)
    N = tb.n
    d_cls, d_idx = empty(N + 16), empty(4 * KT * N + 16)
    d_counts, d_out_off = empty(8 * (KT + 2)), empty(8 * (N + 1))
    sb = fc.scratch_bytes(N)
    scratch = torch.empty(sb, dtype=torch.uint8, device=DEV)
    fc.classify(tb.d_buf, BUF_LEN, tb.d_offs, N, d_cls, d_idx, d_counts, d_out_off, scratch, sb)
    counts = host(d_counts, 8 * (KT + 2), np.uint64)
    assert np.array_equal(host(d_cls, N), want)
    assert (host(d_cls, N + 16)[N:] == 0xA5).all()
    assert [int(c) for c in counts[:KT]] == [int((want == j).sum()) for j in range(KT)]
    assert int(counts[KT + 1]) == int((want == TF.UNKNOWN).sum())
    idx = host(d_idx, 4 * KT * N, np.uint32).reshape(KT, N)
    ends = np.append(tb.offs[1:].astype(np.int64), BUF_LEN)
    for j in range(KT):
        nk = int(counts[j])
        got = idx[j, :nk]
        assert nk > 30 and np.array_equal(np.sort(got), np.flatnonzero(want == j).astype(np.uint32)), j
        assert (got >= k).sum() > 30, "frames of this method in the top range"
        d_ik = d_idx[4 * j * N:]
        if j < K:
            schema, method, _ = TF.METHODS[j]
            fin = len(srpc_amd.framed_request_prefix(schema, method)) + schema.body_bytes
            g = empty(nk * fin + 16)
            fc.gather(tb.d_buf, tb.d_offs, d_ik, nk, fin, g)
            exp_g = np.concatenate([tb.bytes_at(int(tb.offs[f]), fin) for f in got])
            assert host(g, nk * fin).tobytes() == exp_g.tobytes(), j
            assert (host(g, nk * fin + 16)[nk * fin:] == 0xA5).all()
        else:
            payloads = [tb.np_image[int(tb.offs[f]) + 4:int(ends[f])].tobytes() for f in got]
            total = sum(len(x) for x in payloads)
            g, rec = empty(total + 16), empty(8 * (nk + 1) + 16)
            gsb = fc.scratch_bytes(nk)
            gs = torch.empty(gsb, dtype=torch.uint8, device=DEV)
            srpc_amd.FrameClassifier.gather_var(tb.d_buf, tb.d_offs, d_ik, nk, g, rec, gs, gsb)
            exp_rec = np.zeros(nk + 1, np.uint64)
            exp_rec[1:] = np.cumsum([len(x) for x in payloads])
            assert np.array_equal(host(rec, 8 * (nk + 1), np.uint64), exp_rec), j
            assert host(g, total).tobytes() == b"".join(payloads), j
            assert (host(g, total + 16)[total:] == 0xA5).all() and (host(rec, 8 * (nk + 1) + 16)[-16:] == 0xA5).all()
    print(f"FTOP classify+gather+gather_var: n={N} counts={[int(c) for c in counts]} last offset={int(tb.offs[-1])}")


def test_unpack_replies_mixed_legs_top():
    """srpc_frames_unpack_replies_mixed_legs with a column plan, a string plan and record plans
    side by side; batch, model and checks of tests/test_gpu_mixed_legs.py (calc_text, mixed)."""
    from tests import test_gpu_mixed_legs as ML
    from tests.test_gpu_mixed_var import TIMEOUT, batch, build_index, joined, model
    n = N_LOW + N_TOP_LONG
    B = batch("calc_echo", n, "uniform", "short")
    L = ML.legs("calc_text", "natural", "mixed")
    assert L.recs and any(ML.is_var(L.P.methods[k][2]) for k in range(L.K)) and len(L.recs) < L.K - 1
    assert N_TOP_LONG > 2 * L.rep.tile[0], "more than two tiles of calls in the top range"
    rng = np.random.default_rng(31)
    parts = list(B.rep_frames(rng.integers(0, 3, n)))
    for i in np.flatnonzero(rng.random(n) < 0.15):
        parts[int(i)] = struct.pack(">IB", 1, int(rng.integers(1, 256)))       # bare error frames
    parts[N_LOW - 1] = struct.pack(">IB", 1, 9)                                  # the gap frame
    parts[N_LOW + 200] = struct.pack(">I", 0xFFFFFFFF) + b"\x01" + b"\x00" * 11  # o + 4 + len passes 2^32
    parts[N_LOW + 207] = struct.pack(">I", 2**32 - 4) + b"\x03" + b"\x00" * 11   # ... and comes back to o
    parts[n - 1] = b""                                                           # the last offset is buf_len
    full_last = parts[n - 2]
    assert len(full_last) > 5                                                    # a full frame ends at buf_len
    buf, offs = joined(parts)
    tb = TopBuffer(buf, offs[:n], N_LOW, empty_last=False)
    assert int(tb.offs[n - 1]) == BUF_LEN and int(tb.offs[N_LOW]) >= 2**32 - 65536
    O = ML.LegOuts(L, B)
    d_method, d_index, _ = build_index(B.method, L.K)
    d_codes = empty(n + 16)
    d_ends = empty(8 * O.nslots + 16)
    sb = L.rep.scratch_bytes(n)
    d_scratch = empty(sb + 16)
    st = status_buf()
    rc = L.rep.unpack(tb.d_buf, BUF_LEN, tb.d_offs, n, d_method, d_index, n, TIMEOUT, O.cols, O.offs, O.scap, O.recs,
                      L.fill, None, O.cap, d_codes, d_ends, st, d_scratch, sb)
    flags, bad = read_status(st)
    assert (host(d_codes, n + 16)[n:] == 0xA5).all() and (host(d_ends, 8 * O.nslots + 16)[8 * O.nslots:] == 0xA5).all()
    assert (host(d_scratch, sb + 16)[sb:] == 0xA5).all(), "wrote past the scratch"
    wc, full, wflags, wbad = model(tb.image, BUF_LEN, tb.offs, n, B, [0] * B.P.K, O.cap)
    assert wbad == N_LOW - 1 and full[n - 2] and not full[n - 1] and full[N_LOW:].sum() > 400
    assert not full[N_LOW + 200] and not full[N_LOW + 207]
    print(f"FTOP unpack_replies_mixed_legs: n={n} full={int(full.sum())} rc={rc} flags={flags} first={bad}")
    assert rc == 0
    assert np.array_equal(host(d_codes, n), wc)
    assert (flags, bad) == (wflags, wbad)
    ML.check_legs(L, B, O, full, ends=host(d_ends, 8 * O.nslots, np.uint64).copy())


def test_unpack_requests_mixed_legs_top():
    """srpc_frames_unpack_requests_mixed_legs with column, string and record plans side by
    side; streams, model and comparisons of tests/test_gpu_requests_mixed_legs.py (calc_echo,
    mixed).  The steps are that module's `check`, with the call made on the sparse buffer."""
    from srpc_amd import MixedFrames
    from tests import test_gpu_requests_mixed_legs as RL
    from tests.test_gpu_mixed_var import joined
    n = N_LOW + 600
    S = RL.side("calc_echo", "natural", "mixed")
    assert S.recs and len(S.recs) < S.K - 1 and 600 > 2 * S.req.tile[0]
    B = RL.base_batch("calc_echo")
    rng = np.random.default_rng(41)
    method = rng.integers(0, S.K, n)
    frames, intent, src = RL.stream_of(S, B, method, foreign=0.1, seed=3)
    frames[N_LOW - 1], intent[N_LOW - 1] = RL.foreign_frame(B, N_LOW - 1), RL.UNKNOWN     # the gap frame
    for i, be in ((N_LOW + 200, 0xFFFFFFFF), (N_LOW + 207, 2**32 - 4)):                   # o + 4 + len passes 2^32
        frames[i], intent[i] = struct.pack(">I", be) + frames[i][4:], RL.UNKNOWN
    frames[n - 1], intent[n - 1] = b"", RL.UNKNOWN                                        # the last offset is buf_len
    assert intent[n - 2] != RL.UNKNOWN                                                    # a request ends at buf_len
    buf, offs = joined(frames)
    tb = TopBuffer(buf, offs[:n], N_LOW, empty_last=False)
    assert int(tb.offs[n - 1]) == BUF_LEN and int(tb.offs[N_LOW]) >= 2**32 - 65536
    K, data = S.K, B.req
    want = RL.model(S, tb.image, BUF_LEN, tb.offs)
    assert np.array_equal(want, intent), "the stream is not what the test meant to build"
    counts = [int((want == k).sum()) for k in range(K)]
    f0 = [RL.FRONT if S.rec[k] else 0 for k in range(K)]
    base = [0] * K
    cap = [f0[k] + counts[k] for k in range(K)]
    alloc = [cap[k] + (RL.SPARE if S.rec[k] else 0) for k in range(K)]
    chars, scap = RL.sized(S, data, want, src, f0, cap, base)
    O = RL.LegOuts(S, alloc, chars)
    G = RL.GUARD
    nb = MixedFrames.index_bytes(n, K)
    sb = S.req.scratch_bytes(n)
    d_cls, d_index, d_counts = empty(n + G), empty(nb + G), empty(8 * (K + 1) + G)
    d_ends, d_scratch = empty(8 * O.nslots + G), empty(sb + G)
    st = status_buf()
    st[:] = 0x5A  # the call resets it
    rc = S.req.unpack_requests(tb.d_buf, BUF_LEN, tb.d_offs, n, O.cols, O.offs, scap, O.recs, S.fill, f0, cap, d_cls,
                               d_index, nb, d_counts, d_ends, st, d_scratch, sb)
    assert rc == 0
    flags, bad = read_status(st)
    raw_cls, raw_index = host(d_cls, n + G), host(d_index, nb + G)
    assert (raw_cls[n:] == 0xA5).all() and (raw_index[nb:] == 0xA5).all()
    raw_counts, raw_ends = host(d_counts, 8 * (K + 1) + G), host(d_ends, 8 * O.nslots + G)
    assert (raw_counts[-G:] == 0xA5).all() and (raw_ends[-G:] == 0xA5).all()
    assert (host(d_scratch, sb + G)[sb:] == 0xA5).all(), "wrote past the scratch"
    assert np.array_equal(raw_cls[:n], want)
    assert np.array_equal(RL.classify_cls(S, tb.d_buf, BUF_LEN, tb.d_offs, n), want)
    got_counts = raw_counts[:8 * (K + 1)].view(np.uint64).tolist()
    assert got_counts == counts + [int((want == RL.UNKNOWN).sum())]
    RL.compare_legs(S, data, O, want, src, f0, cap, base, scap, ends=raw_ends[:8 * O.nslots].view(np.uint64).copy(),
                    flags_bad=(flags, bad))
    print(f"FTOP unpack_requests_mixed_legs: n={n} counts={got_counts} flags={flags}")
