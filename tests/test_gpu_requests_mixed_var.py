"""A batch of request frames of several methods, string-bodied ones included,
decoded in arrival order on the device (srpc_frames_unpack_requests_mixed_var,
include/srpc_gpu.h), and the ordered reply pack
(srpc_frames_pack_requests_mixed_var over the response plans with d_method =
d_class and the index the decode wrote).

Nothing expected comes from the kernels under test:
- every frame is `BE32 | oracle.pack` of one element behind the plan's prefix,
  cut at record boundaries computed from the string lengths and interleaved in
  numpy / Python (tests/test_gpu_mixed_var.Batch); foreign frames are method 0's
  with the last char of the method name changed (the same length as method 0's);
  hostile frames are literal edits of a good frame;
- classes come from `model`, the header's rule written out on the host; they are
  checked against the class each frame was built to have and against
  srpc_frames_classify on the same input;
- ranks are numpy's (`cumcount`); fields, chars and offsets are the inputs.
Outputs are 0xA5-filled with 16 guard bytes behind each; the guards must
survive.  Every case asserts that its input holds what it names."""
import functools
import struct

import numpy as np
import pytest

import oracle
from srpc_amd import FrameClassifier, GpuPacker, MixedFrames, MixedVarFrames, Schema, _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

import srpc_amd  # noqa: E402
from tests.test_gpu_mixed_var import (MULTIPLE, PATTERNS, SETS, STRING, batch, cumcount, is_var, joined, nstr,  # noqa: E402
                                      plans, run_pack, sizes)
from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402

UNKNOWN = _lib.SRPC_FRAME_UNKNOWN
BOUNDS = _lib.SRPC_STATUS_BOUNDS
INVALID, ALIGN, UNSUPPORTED, CAPACITY = (_lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_UNSUPPORTED,
                                         _lib.SRPC_E_CAPACITY)
NONE = 2**64 - 1
GUARD = 16


class Doubled:
    """The one-method `echo` set with its string plan registered twice."""

    def __init__(self):
        P = plans("echo")
        self.K = 2
        self.methods = P.methods * 2
        self.req_plans, self.rep_plans = P.req_plans * 2, P.rep_plans * 2
        self.req, self.rep = MixedVarFrames(self.req_plans), MixedVarFrames(self.rep_plans)
        self.req_prefix, self.rep_prefix = P.req_prefix * 2, P.rep_prefix * 2
        self.req_fixed, self.rep_fixed = P.req_fixed * 2, P.rep_fixed * 2


@functools.lru_cache(maxsize=None)
def classifier(P):
    return FrameClassifier([(p, 0) for p in P.req_plans])


def model(P, raw, buf_len, offs):
    """d_class by the header's rule.  Frame i is bytes [offs[i], end_i), end_i the
    next offset or buf_len.  A fixed plan matches a frame of its length that
    starts with its framed prefix; a string plan matches a frame of at least its
    least length whose BE32 is its length - 4, whose payload starts with the
    prefix and whose walk ends exactly at its end.  The first match wins."""
    n = len(offs)
    cls = np.full(n, UNKNOWN, np.uint8)
    o = [int(x) for x in offs]
    e = o[1:] + [buf_len]
    heads = []
    for k in range(P.K):
        kinds, pre = P.methods[k][1].kinds, P.req_prefix[k]
        heads.append((STRING in kinds, kinds, pre, struct.pack(">I", P.req_fixed[k] - 4) + pre))
    for i in range(n):
        if not (o[i] <= e[i] <= buf_len):
            continue
        ln = e[i] - o[i]
        f = raw[o[i]:o[i] + min(ln, 4096)]  # the walk below reads inside the fixed part and the length words only
        for k, (var, kinds, pre, framed) in enumerate(heads):
            if not var:
                if ln == P.req_fixed[k] and f[:len(framed)] == framed:
                    cls[i] = k
                    break
                continue
            if ln < P.req_fixed[k] or int.from_bytes(f[:4], "big") != ln - 4 or f[4:4 + len(pre)] != pre:
                continue
            c, ok = 4 + len(pre), True
            for kind in kinds:
                if kind == STRING:
                    if ln - c < 8:
                        ok = False
                        break
                    w = raw[o[i] + c:o[i] + c + 8]
                    sl = int.from_bytes(w, "little")
                    c += 8
                    if sl > ln - c:
                        ok = False
                        break
                    c += sl
                else:
                    if oracle.KIND_SIZE[kind] > ln - c:
                        ok = False
                        break
                    c += oracle.KIND_SIZE[kind]
            if ok and c == ln:
                cls[i] = k
                break
    return cls


class Outs:
    """The request side's device outputs: per plan the columns (alloc[k] elements
    of a fixed leaf, chars[k][f] bytes of a string leaf) and the offsets arrays."""

    def __init__(self, P, alloc, chars):
        self.alloc, self.chars = alloc, chars
        self.cols, self.offs = [], []
        for k, (_, rq, _) in enumerate(P.methods):
            cs, os_ = [], []
            for f, kind in enumerate(rq.kinds):
                if kind == STRING:
                    cs.append(empty(chars[k][f] + GUARD))
                    os_.append(empty(8 * (alloc[k] + 1) + GUARD))
                else:
                    cs.append(empty(alloc[k] * oracle.KIND_SIZE[kind] + GUARD))
                    os_.append(None)
            self.cols.append(cs)
            self.offs.append(os_)
        self.nslots = sum(nstr(rq) for _, rq, _ in P.methods)


def run(P, O, raw, buf_len, offs, first, cap, scap, status=True, scratch=None):
    """One call -> dict of what it wrote besides the columns (guards checked;
    scratch: the caller's own, which may be larger, instead of a fresh one)."""
    n, K = len(offs), P.K
    d_buf = dev(np.frombuffer(raw, np.uint8)) if len(raw) else empty(16)
    d_offs = dev(np.asarray(offs, np.uint32)) if n else empty(16)
    nb = MixedFrames.index_bytes(n, K)
    sb = P.req.scratch_bytes(n)
    d_cls, d_index, d_counts = empty(n + GUARD), empty(nb + GUARD), empty(8 * (K + 1) + GUARD)
    d_ends, d_scratch = empty(8 * O.nslots + GUARD), empty(sb + GUARD) if scratch is None else scratch
    behind = d_scratch[sb:].clone()
    st = status_buf()
    st[:] = 0x5A  # the call resets it
    rc = P.req.unpack_requests(d_buf, buf_len, d_offs, n, O.cols, O.offs, scap, first, cap, d_cls, d_index, nb, d_counts,
                               d_ends, st if status else None, d_scratch, sb)
    assert rc == 0
    flags, bad = read_status(st) if status else (None, None)
    raw_cls = host(d_cls, n + GUARD)
    assert (raw_cls[n:] == 0xA5).all() and (host(d_index, nb + GUARD)[nb:] == 0xA5).all()
    raw_counts = host(d_counts, 8 * (K + 1) + GUARD)
    raw_ends = host(d_ends, 8 * O.nslots + GUARD)
    assert (raw_counts[-GUARD:] == 0xA5).all() and (raw_ends[-GUARD:] == 0xA5).all()
    assert torch.equal(d_scratch[sb:], behind), "wrote past the scratch"
    return dict(cls=raw_cls[:n].copy(), counts=raw_counts[:8 * (K + 1)].view(np.uint64).copy(),
                ends=raw_ends[:8 * O.nslots].view(np.uint64).copy(), flags=flags, bad=bad, d_cls=d_cls, d_index=d_index,
                d_buf=d_buf, d_offs=d_offs)


def classify_cls(P, d_buf, buf_len, d_offs, n):
    """d_class as srpc_frames_classify writes it for the same buffer."""
    K = P.K
    c = classifier(P)
    d_cls, d_idx = empty(n + GUARD), empty(4 * K * n + GUARD)
    d_counts, d_out_off = empty(8 * (K + 2)), empty(8 * (n + 1))
    sb = c.scratch_bytes(n)
    scratch = torch.empty(max(sb, 16), dtype=torch.uint8, device="cuda:0")
    c.classify(d_buf, buf_len, d_offs, n, d_cls, d_idx, d_counts, d_out_off, scratch, sb)
    return host(d_cls, n).copy()


def compare(P, legs, O, want, src, f0, cap, base, scap, ends=None, flags_bad=None):
    """Every column, offsets array and char column against the host's
    expectation: frame i of class k was built from element src[i] of legs[k] and
    belongs at element f0[k] + rank(i); what no frame owns is still 0xA5."""
    rank = cumcount(want)
    bad, slot = NONE, 0
    for k, (_, rq, _) in enumerate(P.methods):
        idx = np.flatnonzero(want == k)
        e = f0[k] + rank[idx]
        ok = e < cap[k]
        if not ok.all():
            bad = min(bad, int(idx[~ok][0]))
        e, el = e[ok], src[idx[ok]]
        cols, offs, _ = legs[k]
        for f, kind in enumerate(rq.kinds):
            if kind == STRING:
                xo = offs[f].astype(np.int64)
                b0 = base[k] if f0[k] else 0
                ln = np.diff(xo)[el] if len(el) else np.zeros(0, np.int64)
                exp_o = np.full(8 * (O.alloc[k] + 1) + GUARD, 0xA5, np.uint8)
                view = exp_o[:8 * (O.alloc[k] + 1)].view(np.uint64)
                if f0[k] == 0:
                    view[0] = 0
                elif f0[k] <= cap[k]:
                    view[f0[k]] = b0  # what the chunk before left there
                if len(el):
                    view[f0[k] + 1:f0[k] + 1 + len(el)] = b0 + np.cumsum(ln)
                assert np.array_equal(host(O.offs[k][f], len(exp_o)), exp_o), (k, f, "offsets")
                total = int(ln.sum())
                if ends is not None:
                    assert int(ends[slot]) == b0 + total, (k, f, "d_ends")
                slot += 1
                chars = b"".join(cols[f][int(xo[x]):int(xo[x + 1])].tobytes() for x in el)
                exp_c = np.full(O.chars[k][f] + GUARD, 0xA5, np.uint8)
                m = max(min(total, scap[k][f] - b0), 0)
                exp_c[b0:b0 + m] = np.frombuffer(chars[:m], np.uint8)
                assert np.array_equal(host(O.cols[k][f], len(exp_c)), exp_c), (k, f, "chars")
            else:
                dt, sz = oracle.KIND_DTYPE[kind], oracle.KIND_SIZE[kind]
                exp = np.full(O.alloc[k] * sz + GUARD, 0xA5, np.uint8)
                exp[:O.alloc[k] * sz].view(dt)[e] = cols[f][el]
                assert np.array_equal(host(O.cols[k][f], len(exp)), exp), (k, f)
    if flags_bad is not None:
        assert flags_bad == ((BOUNDS, bad) if bad != NONE else (0, NONE))


def check(P, legs, frames, intent, src, buf_len=None, offs=None, first=None, cap=None, alloc=None, base=None, scap_cut=0,
          raw=None, scratch=None):
    """Run the call on the frames and compare everything it wrote with the
    host's expectation.  intent[i]: the class frame i was built to have; src[i]:
    the element of its plan's leg it was built from.  -> the run."""
    if raw is None:
        raw, o = joined(frames)
        offs = o[:-1] if offs is None else offs
        buf_len = len(raw) if buf_len is None else buf_len
    n, K = len(offs), P.K
    want = model(P, raw, buf_len, offs)
    assert np.array_equal(want, intent), "the stream is not what the test meant to build"
    counts = [int((want == k).sum()) for k in range(K)]
    f0 = [0] * K if first is None else list(first)
    base = [0] * K if base is None else list(base)
    cap = [f0[k] + counts[k] for k in range(K)] if cap is None else list(cap)
    alloc = [max(cap[k], f0[k] + counts[k]) for k in range(K)] if alloc is None else list(alloc)
    rank = cumcount(want)
    chars, scap = [], []
    for k, (_, rq, _) in enumerate(P.methods):
        idx = np.flatnonzero(want == k)
        el = src[idx[f0[k] + rank[idx] < cap[k]]]
        row_c, row_s = [], []
        for f, kind in enumerate(rq.kinds):
            if kind != STRING:
                row_c.append(None)
                row_s.append(None)
                continue
            total = int(np.diff(legs[k][1][f].astype(np.int64))[el].sum()) if len(el) else 0
            b0 = base[k] if f0[k] else 0
            row_c.append(b0 + total)
            row_s.append(max(b0 + total - scap_cut, 0))
        chars.append(row_c)
        scap.append(row_s)
    O = Outs(P, alloc, chars)
    for k in range(K):  # the offsets a chunk before would have left at entry first[k]
        if f0[k] and f0[k] <= cap[k]:
            for t in O.offs[k]:
                if t is not None:
                    t[8 * f0[k]:8 * f0[k] + 8] = torch.from_numpy(np.array([base[k]], np.uint64).view(np.uint8).copy())
    got = run(P, O, raw, buf_len, offs, first, cap, scap, scratch=scratch)
    assert np.array_equal(got["cls"], want)
    assert np.array_equal(classify_cls(P, got["d_buf"], buf_len, got["d_offs"], n), want)
    assert got["counts"].tolist() == counts + [int((want == UNKNOWN).sum())]
    compare(P, legs, O, want, src, f0, cap, base, scap, ends=got["ends"], flags_bad=(got["flags"], got["bad"]))
    got["O"], got["scap"], got["want"] = O, scap, want
    return got


def foreign_frame(B, i):
    """Method 0's frame of some element under a method name nobody registered."""
    f = bytearray(B.req[0][2][0][i % B.counts[0]])
    f[4 + 8 + len(B.P.methods[0][0]) - 1] ^= 0x01  # BE32 | u64 length | method: its last char
    return bytes(f)


def stream(B, foreign=0.0, seed=0):
    """The batch's request frames in call order, a share of them replaced by
    foreign frames -> (frames, intent, src)."""
    frames = B.req_frames()
    intent = B.method.copy()
    if foreign > 0:
        assert B.counts[0] > 0
        rng = np.random.default_rng(seed + B.n)
        pick = np.arange(B.n) if foreign >= 1.0 else np.flatnonzero(rng.random(B.n) < foreign)
        for i in pick:
            frames[int(i)] = foreign_frame(B, int(i))
        intent[pick] = UNKNOWN
    return frames, intent, B.rank.copy()


def regime_of(name):
    return "mid" if name != "sixteen" else "short"


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_sizes_and_orders(name, which):
    P = plans(name)
    T = P.req.tile[0]
    for n in sizes(T):
        B = batch(name, n, which, regime_of(name))
        frames, intent, src = stream(B, 0.1 if n > 1 and which != "one_plan" and B.counts[0] else 0.0)
        got = check(P, B.req, frames, intent, src)
        if n >= 255 and which in ("round_robin", "uniform"):
            assert all(got["counts"][k] > 0 for k in range(P.K)), "a frame of every class"
            assert got["counts"][P.K] > 0, "and unknown ones"
    assert P.req.tile[0] == (128 if name == "sixteen" else 256)


@pytest.mark.parametrize("name", sorted(SETS))
def test_50001(name):
    """Several super-rows of the index."""
    B = batch(name, 50_001, "uniform", "short")
    frames, intent, src = stream(B, 0.1)
    got = check(B.P, B.req, frames, intent, src)
    assert all(c > 0 for c in got["counts"].tolist()) and 50_001 > 16 * 256 * 8


@pytest.mark.parametrize("foreign", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("name", sorted(SETS))
def test_foreign_share(name, foreign):
    B = batch(name, 4097, "uniform", "short")
    frames, intent, src = stream(B, foreign, seed=1)
    got = check(B.P, B.req, frames, intent, src)
    unknown = int(got["counts"][B.P.K])
    if foreign == 0.1:
        assert 0 < unknown < 4097 and all(c > 0 for c in got["counts"].tolist())
    else:
        assert unknown == (4097 if foreign else 0)
    own = {len(f) for f in B.req[0][2][0]}
    assert all(len(f) in own for f, c in zip(frames, intent) if c == UNKNOWN)  # the same length as method 0's


REGIMES = ["empty", "short", "mid", "edges", "over_first", "over_mid", "over_last", "over_two"]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["echo", "calc_echo", "two_str"])
def test_length_regimes(name, regime):
    P = plans(name)
    T, image = P.req.tile
    B = batch(name, 4 * T + 5, "uniform" if name != "echo" else "one_plan", regime)
    frames, intent, src = stream(B)
    check(P, B.req, frames, intent, src)
    _, woffs = joined(frames)
    lens = np.diff(woffs)
    if regime == "empty":
        assert set(lens) == {P.req_fixed[k] for k in set(B.method)}
    if regime == "edges":
        A = int(woffs[T]) & ~15
        assert A + image in woffs[T + 1:2 * T + 1], "a frame ending exactly at the image window's end"
        A = int(woffs[3 * T]) & ~15
        assert A + image + 1 in woffs[3 * T + 1:4 * T + 1], "a frame ending one byte past the window"
    if regime.startswith("over"):
        big = np.flatnonzero(lens > image)
        assert len(big) == (2 if regime == "over_two" else 1) and (big // T == 1).all(), "oversize frames in tile 1"
        A = int(woffs[T]) & ~15
        if regime != "over_last":
            after = np.arange(big[0] + 1, 2 * T)
            assert len(after) and (woffs[after + 1] - A > image).all(), "the frames behind it are outside the image"


# ---- hostile frames among good neighbours -----------------------------------------------------

def walk(P, k, g):
    """-> (offset of the first string's length word, offset inside the first fixed field or None)."""
    kinds = P.methods[k][1].kinds
    c, first_str, in_fixed = 4 + len(P.req_prefix[k]), None, None
    for kind in kinds:
        if kind == STRING:
            first_str = c if first_str is None else first_str
            c += 8 + int.from_bytes(g[c:c + 8], "little")
        else:
            sz = oracle.KIND_SIZE[kind]
            if in_fixed is None and sz > 1:
                in_fixed = c + sz // 2
            c += sz
    assert c == len(g)
    return first_str, in_fixed


def reframe(body):
    return struct.pack(">I", len(body)) + body


def with_len(P, k, g, value):
    at, _ = walk(P, k, g)
    b = bytearray(g)
    b[at:at + 8] = struct.pack("<Q", value % 2**64)
    return bytes(b)


def flip(g, at):
    b = bytearray(g)
    b[at] ^= 0x01
    return bytes(b)


# edits of a good frame g of string plan k; every result is nobody's frame
VAR_EDITS = {
    "be32": lambda P, k, g: flip(g, 3),
    "len_2_63": lambda P, k, g: with_len(P, k, g, 2**63),
    "len_2_64m1": lambda P, k, g: with_len(P, k, g, 2**64 - 1),
    "len_one_past": lambda P, k, g: with_len(P, k, g, len(g) - (walk(P, k, g)[0] + 8) + 1),
    "ends_one_early": lambda P, k, g: reframe(g[4:] + b"\x00"),
    "cut_in_prefix": lambda P, k, g: reframe(g[4:4 + len(P.req_prefix[k]) - 2]),
    "cut_in_length_word": lambda P, k, g: reframe(g[4:walk(P, k, g)[0] + 3]),
    "cut_in_fixed_field": lambda P, k, g: reframe(g[4:walk(P, k, g)[1]]),
    "three_bytes": lambda P, k, g: g[:3],
    "last_prefix_byte": lambda P, k, g: flip(g, 4 + len(P.req_prefix[k]) - 1),
}
# edits of a good frame of a fixed plan: the right prefix, the wrong length
FIXED_EDITS = {
    "fixed_one_longer": lambda P, k, g: g + b"\x00",
    "fixed_one_shorter": lambda P, k, g: g[:-1],
}


def hostile_plan(P, what):
    """The plan whose frame the edit is made of: a string plan with a fixed
    field of more than a byte (all of MULTIPLE, MIX), or a fixed plan."""
    want_var = what in VAR_EDITS
    for k, (_, rq, _) in enumerate(P.methods):
        if is_var(rq) == want_var and (not want_var or rq in (MULTIPLE, SETS["two_str"][0][1])):
            return k
    raise AssertionError("no such plan")


@pytest.mark.parametrize("what", sorted(VAR_EDITS) + sorted(FIXED_EDITS))
@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_hostile_frame(name, what):
    """The hostile frame first in a tile, mid-tile, last in a tile, and as the
    final frame of the buffer with nothing behind it."""
    P = plans(name)
    T = P.req.tile[0]
    B = batch(name, 3 * T + 5, "uniform", "mid")
    frames, intent, src = stream(B)
    k = hostile_plan(P, what)
    edit = VAR_EDITS.get(what) or FIXED_EDITS[what]
    spots = [T, T + T // 2, 2 * T - 1, B.n - 1]
    for j, p in enumerate(spots):
        g = B.req[k][2][0][j]  # a good frame of plan k (with chars: element j of a `mid` leg)
        h = edit(P, k, g)
        assert h != g
        frames[p] = h
        intent[p] = UNKNOWN
    got = check(P, B.req, frames, intent, src)
    assert (got["cls"][spots] == UNKNOWN).all() and got["counts"][P.K] == len(spots)
    near = [p + d for p in spots for d in (-1, 1) if 0 <= p + d < B.n and p + d not in spots]
    assert (got["cls"][near] != UNKNOWN).all(), "the neighbours keep their classes"
    # the final frame alone in a buffer that ends with it
    h = frames[-1]
    lone = check(P, B.req, [h], np.array([UNKNOWN], np.uint8), np.zeros(1, np.int64))
    assert lone["counts"].tolist() == [0] * P.K + [1]


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_offsets_out_of_order(name):
    P = plans(name)
    T = P.req.tile[0]
    B = batch(name, 3 * T + 5, "uniform", "mid")
    frames, intent, src = stream(B)
    raw, o = joined(frames)
    offs = o[:-1].copy()
    for p in (T, T + T // 2, 2 * T - 1):
        # frame p - 1 now spans three frames, frame p runs backwards, frame p + 1 is whole
        offs[p] = offs[p + 2]
        intent[p - 1] = intent[p] = UNKNOWN
    got = check(P, B.req, None, intent, src, raw=raw, buf_len=len(raw), offs=offs)
    assert got["counts"][P.K] == 6


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_frames_past_buf_len(name):
    P = plans(name)
    B = batch(name, 700, "uniform", "mid")
    frames, intent, src = stream(B)
    raw, o = joined(frames)
    offs, total = o[:-1].copy(), len(raw)
    # the last frame cut by one byte
    cut = intent.copy()
    cut[-1] = UNKNOWN
    check(P, B.req, None, cut, src, raw=raw[:total - 1], buf_len=total - 1, offs=offs)
    # the last frame starts past buf_len: the one before it now ends past buf_len
    far = offs.copy()
    far[-1] = total + 8
    cut = intent.copy()
    cut[-2:] = UNKNOWN
    check(P, B.req, None, cut, src, raw=raw, buf_len=total, offs=far)
    # buf_len inside frame 650's length word or fixed part (the allocation holds the whole stream): it and
    # every later frame are nobody's
    cut = intent.copy()
    cut[650:] = UNKNOWN
    check(P, B.req, None, cut, src, raw=raw, buf_len=int(offs[650]) + 9, offs=offs)


def test_same_string_plan_twice():
    """The first registration wins, the second counts 0 and writes nothing but
    its empty offsets' entry 0."""
    P = Doubled()
    B = batch("echo", 1000, "one_plan", "mid")
    frames, intent, src = stream(B)
    got = check(P, B.req * 2, frames, intent, src)
    assert got["counts"].tolist() == [1000, 0, 0] and got["ends"][1] == 0 and got["ends"][0] > 0


# ---- h_first / h_cap / h_str_cap --------------------------------------------------------------

@pytest.mark.parametrize("name", ["calc_echo", "two_str", "sixteen"])
def test_three_chunks_equal_the_whole(name):
    P = plans(name)
    B = batch(name, 1000, "uniform", regime_of(name))
    frames, intent, src = stream(B, 0.05, seed=2)
    whole = check(P, B.req, frames, intent, src)
    O = Outs(P, whole["O"].alloc, whole["O"].chars)
    cap = O.alloc
    done = [0] * P.K
    for lo, hi in ((0, 1), (1, 513), (513, 1000)):
        raw, o = joined(frames[lo:hi])
        got = run(P, O, raw, len(raw), o[:-1], list(done), cap, whole["scap"])
        assert (got["flags"], got["bad"]) == (0, NONE) and np.array_equal(got["cls"], intent[lo:hi])
        for k in range(P.K):
            done[k] += int((intent[lo:hi] == k).sum())
    assert np.array_equal(got["ends"], whole["ends"])
    compare(P, B.req, O, intent, src, [0] * P.K, cap, [0] * P.K, whole["scap"])


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_second_chunk_continues_from_entry_first(name):
    """Non-zero h_first: the offsets continue from what entry h_first[k] holds,
    entry 0 and every element before h_first[k] stay untouched."""
    P = plans(name)
    B = batch(name, 1000, "uniform", "mid")
    frames, intent, src = stream(B, 0.05, seed=3)
    check(P, B.req, frames, intent, src, first=[5 + 11 * k for k in range(P.K)], base=[1000 + 7 * k for k in range(P.K)])


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_short_columns(name):
    """h_cap[k] short of the count: the excess frames keep their class and write
    nothing, no offsets entry past h_cap[k]; BOUNDS with the smallest such i."""
    P = plans(name)
    B = batch(name, 1000, "uniform", "mid")
    frames, intent, src = stream(B)
    for k in (1, P.K - 1, 0):  # calc_echo: a fixed plan, the string plan; two_str: a string plan, the fixed one
        cap = list(B.counts)
        cap[k] -= 3
        got = check(P, B.req, frames, intent, src, cap=cap, alloc=B.counts)
        assert got["flags"] == BOUNDS and got["bad"] == int(np.flatnonzero(intent == k)[-3]) and got["cls"][got["bad"]] == k
        first = [3] * P.K
        check(P, B.req, frames, intent, src, first=first, cap=[3 + c for c in cap], alloc=[3 + c for c in B.counts],
              base=[40] * P.K)


@pytest.mark.parametrize("cut", [1, 1000])
def test_string_capacity(cut):
    """h_str_cap below the chars: nothing at or past it is written, d_ends is the
    full total."""
    B = batch("two_str", 1000, "uniform", "mid")
    frames, intent, src = stream(B)
    got = check(B.P, B.req, frames, intent, src, scap_cut=cut)
    caps = [c for row in got["scap"] for c in row if c is not None]
    assert len(caps) == 3 and all(int(e) == c + cut for e, c in zip(got["ends"], caps))


def test_null_status():
    B = batch("calc_echo", 300, "uniform", "mid")
    frames, intent, src = stream(B, 0.1, seed=4)
    raw, o = joined(frames)
    whole = check(B.P, B.req, frames, intent, src)  # the status was reset from a 0x5A fill
    assert (whole["flags"], whole["bad"]) == (0, NONE)
    O = Outs(B.P, whole["O"].alloc, whole["O"].chars)
    got = run(B.P, O, raw, len(raw), o[:-1], None, O.alloc, whole["scap"], status=False)
    assert np.array_equal(got["cls"], intent)
    compare(B.P, B.req, O, intent, src, [0] * B.P.K, O.alloc, [0] * B.P.K, whole["scap"], ends=got["ends"])


def test_no_frames():
    P = plans("calc_echo")
    got = check(P, batch("calc_echo", 0, "uniform", "mid").req, [], np.zeros(0, np.uint8), np.zeros(0, np.int64))
    assert got["counts"].tolist() == [0] * (P.K + 1) and (got["ends"] == 0).all()


# ---- the reply side: srpc_frames_pack_requests_mixed_var over the response plans ----------------

@pytest.mark.parametrize("foreign", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("name", sorted(SETS))
def test_ordered_reply_pack(name, foreign):
    """d_method = d_class, the index the decode wrote: the oracle's replies in
    arrival order, zero bytes at unknown frames, nothing at or past the total."""
    P = plans(name)
    for n in (1, 257, 4097):
        B = batch(name, n, "uniform", "short")
        if foreign and not B.counts[0]:
            continue
        frames, intent, src = stream(B, foreign, seed=5)
        got = check(P, B.req, frames, intent, src)
        good = intent != UNKNOWN
        rank = cumcount(intent)
        # response r of method k answers its r-th request in arrival order; the plans carry code 2
        parts = [B.rep[int(k)][2][2][int(r)] if g else b"" for k, r, g in zip(intent, rank, good)]
        want, woffs = joined(parts)
        legs = [([dev(c) for c in l[0]], [None if o is None else dev(o) for o in l[1]]) for l in B.rep]
        counts = [int((intent == k).sum()) for k in range(P.K)]
        out_cap = len(want)
        d_out, d_offs, d_total = empty(out_cap + GUARD), empty(4 * (n + 1) + GUARD), empty(8 + GUARD)
        sb = P.rep.scratch_bytes(n)
        d_scratch = empty(sb + GUARD)
        st = status_buf()
        st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
        rc = P.rep.pack([l[0] for l in legs], [l[1] for l in legs], None, counts, got["d_cls"], got["d_index"], n, d_out,
                        out_cap, d_offs, d_total, st, d_scratch, sb)
        assert rc == 0
        roffs = host(d_offs, 4 * (n + 1), np.uint32)
        assert (host(d_offs, 4 * (n + 1) + GUARD)[-GUARD:] == 0xA5).all()
        assert np.array_equal(roffs, woffs.astype(np.uint32)) and int(host(d_total, 8, np.uint64)[0]) == len(want)
        assert (roffs[1:][~good] == roffs[:-1][~good]).all()
        rawo = host(d_out, out_cap + GUARD)
        assert rawo[:out_cap].tobytes() == want and (rawo[out_cap:] == 0xA5).all()
        flags, bad = read_status(st)  # the pack's own flag: "unknown frames present", the first of them
        assert (flags, bad) == ((BOUNDS, int(np.flatnonzero(~good)[0])) if (~good).any() else (0, NONE))


@pytest.mark.parametrize("name", sorted(SETS))
def test_round_trip(name):
    """Request frames from srpc_frames_pack_requests_mixed_var, decoded by the
    server's call, give back the columns, chars and offsets; d_class == d_method."""
    for n in (257, 4097):
        B = batch(name, n, "uniform", regime_of(name))
        rc, raw, offs, total, flags, _ = run_pack(B)
        assert rc == 0 and flags == 0 and total == len(raw)
        got = check(B.P, B.req, None, B.method, B.rank.copy(), raw=raw.tobytes(), buf_len=total,
                    offs=offs[:n].astype(np.int64))
        assert np.array_equal(got["cls"], B.method)


# ---- refusals that need real plans -------------------------------------------------------------

def test_refusals_in_order():
    """Every UNSUPPORTED refusal comes before every ALIGN refusal, every ALIGN
    refusal before CAPACITY, nothing launched: a refusal is shown to come first
    by making the later ones true as well."""
    P = plans("calc_echo")
    n = 300
    nb = MixedFrames.index_bytes(n, P.K)
    sb = P.req.scratch_bytes(n)
    buf, offs, cls = empty(64 * n), empty(4 * n + 16), empty(n)
    idx, cnt, ends, scratch = empty(nb + 16), empty(8 * (P.K + 1) + 16), empty(64), empty(sb + 16)
    O = Outs(P, [n] * P.K, [[4096 if kind == STRING else None for kind in rq.kinds] for _, rq, _ in P.methods])
    scap = O.chars
    s17 = Schema.of("S17", *[(f"s{i:02d}", "string") for i in range(17)])  # one string too many
    wide = Schema.of("W", *[(f"w{i}", "int8") for i in range(31)], ("s", "string"))  # 7 x 32 = 224 leaves

    def edited(rows, k, f, by):
        rows = [list(r) for r in rows]
        rows[k][f] = rows[k][f].data_ptr() + by
        return rows

    def call(mv=P.req, buf=buf, offs=offs, idx=idx, nb_given=0, cnt=cnt, ends=ends, scratch=scratch, sb_given=0,
             cols=O.cols, so=O.offs, scap=scap, k_cap=None):
        return mv.unpack_requests(buf, 64 * n, offs, n, cols, so, scap, None, k_cap or [n] * mv.k, cls, idx, nb_given, cnt,
                                  ends, None, scratch, sb_given)

    def outs_for(schemas):
        return ([[empty(8 * n + 16) for _ in s.kinds] for s in schemas],
                [[empty(8 * n + 24) if kind == STRING else None for kind in s.kinds] for s in schemas],
                [[4096 if kind == STRING else None for kind in s.kinds] for s in schemas])

    unsupported = {
        "a string plan without a prefix": (P.req_plans[:4] + [GpuPacker(MULTIPLE, b"")], None),
        "a fixed plan with a prefix under 4 bytes": ([GpuPacker(srpc_amd.NUMBER, b"abc")] + P.req_plans[1:], None),
        "a string plan with 17 strings": ([GpuPacker.for_request(s17, "S_servicer::many")], [s17]),
        "more than 192 leaves": ([GpuPacker.for_request(wide, f"W_servicer::m{j}") for j in range(7)], [wide] * 7),
    }
    for what, (pl, schemas) in unsupported.items():
        mv = MixedVarFrames(pl)
        kw = {}
        if schemas:
            kw["cols"], kw["so"], kw["scap"] = outs_for(schemas)
        assert call(mv=mv, buf=buf.data_ptr() + 1, **kw) == UNSUPPORTED, what  # ahead of ALIGN and CAPACITY
        assert call(mv=mv, nb_given=nb, sb_given=sb, **kw) == UNSUPPORTED, what
    # the same input to the fixed-size call stays UNSUPPORTED
    mf = MixedFrames(P.req_plans)
    assert mf.unpack_requests(buf, 64 * n, offs, n, O.cols, None, [n] * P.K, cls, idx, nb, cnt, None) == UNSUPPORTED
    misaligned = {
        "d_buf (16)": dict(buf=buf.data_ptr() + 8),
        "a fixed column (16)": dict(cols=edited(O.cols, 1, 0, 8)),
        "a string column (16)": dict(cols=edited(O.cols, 4, 3, 8)),
        "a string's offsets array (8)": dict(so=edited(O.offs, 4, 3, 4)),
        "the index (8)": dict(idx=idx.data_ptr() + 4),
        "d_counts (8)": dict(cnt=cnt.data_ptr() + 4),
        "d_ends (8)": dict(ends=ends.data_ptr() + 4),
        "the scratch (8)": dict(scratch=scratch.data_ptr() + 4),
        "d_offs (4)": dict(offs=offs.data_ptr() + 2),
    }
    for what, kw in misaligned.items():
        assert call(**kw) == ALIGN, what  # with no index and no scratch at all: ALIGN comes before CAPACITY
    assert call(nb_given=nb - 1, sb_given=sb) == CAPACITY
    assert call(nb_given=nb, sb_given=sb - 1) == CAPACITY
    assert call(nb_given=0, sb_given=0) == CAPACITY
    torch.cuda.synchronize()
    for t in [cls, idx, cnt, ends] + [c for cc in O.cols for c in cc] + [o for oo in O.offs for o in oo if o is not None]:
        assert (t.cpu().numpy() == 0xA5).all()  # refused: nothing launched
