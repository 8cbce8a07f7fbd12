"""A batch of request frames of several methods decoded in arrival order on the
device, each plan's requests into columns or into one array of structs
(srpc_frames_unpack_requests_mixed_legs, include/srpc_gpu.h), and the ordered
reply pack (srpc_frames_pack_requests_mixed_legs over the response plans with
d_method = d_class and the index the decode wrote).

The servers, `model`, the stream builders and the hostile edits are
tests/test_gpu_requests_mixed_var.py's, used as they are; the assignments of
kinds (`mixed`, `cols`, `recs`) and the struct layouts (`natural`, `tight`,
`s256`) are tests/test_gpu_mixed_legs.py's `Legs`, `layout` and `LAYS`.  A
plan's being a record plan changes where its values go and nothing else, so the
same frames serve every assignment.  Nothing expected comes from the kernel
under test:
- classes are `model`'s, ranks numpy's (`cumcount`);
- a column plan's columns, chars and offsets are the var test's `compare`;
- a record plan's array is numpy: 0xA5, then the fill record over the
  classified elements below the cap, then the leaf bytes from the columns the
  frames were packed from;
- with every plan in columns / every fixed plan in records the outputs are also
  compared with the _mixed_var / _mixed_aos request calls' on the same input.
Outputs start 0xA5-filled with 16 guard bytes behind each.  A record plan's
array has h_first[k] elements in front of the batch's and spare ones behind,
which must keep 0xA5.  The stream is staged as exactly buf_len bytes.  Every
case asserts that its input holds what it names."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import srpc_amd
from srpc_amd import GpuPacker, MixedAosFrames, MixedFrames, MixedLegFrames, _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402
from tests.test_gpu_mixed_var import STRING, batch, cumcount, joined, make_leg, pattern  # noqa: E402
from tests.test_gpu_mixed_legs import LAYS, legs, structs  # noqa: E402
from tests.test_gpu_requests_mixed_var import (FIXED_EDITS, VAR_EDITS, Outs, classify_cls, compare, foreign_frame,  # noqa: E402
                                               hostile_plan, model, regime_of, run, stream)

UNKNOWN = _lib.SRPC_FRAME_UNKNOWN
BOUNDS = _lib.SRPC_STATUS_BOUNDS
INVALID, ALIGN, UNSUPPORTED, CAPACITY = (_lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_UNSUPPORTED,
                                         _lib.SRPC_E_CAPACITY)
NONE = 2**64 - 1
GUARD = 16
IMAGE = 32768
FRONT, SPARE = 2, 3  # elements of a record plan's array before the batch's (h_first) and behind h_cap
# test_gpu_mixed_legs.py's names of tests/test_gpu_mixed_var.py's sets
SETS = {"calc_echo": "calc_text", "sixteen": "sixteen"}
MODES = ["mixed", "cols", "recs"]


class View:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def side(name, lay, mode, upto=None):
    """The request side of a set under an assignment of kinds: test_gpu_mixed_legs.py's
    Legs (L.req over the request plans with the request structs' layouts), the
    plans the call sees (the first `upto`) as `model` and `compare` take them,
    and a fill record per record plan."""
    L = legs(SETS.get(name, name), lay, mode, upto)
    P, K = L.P, L.K
    S = View(L=L, K=K, name=name, methods=P.methods[:K], req_plans=P.req_plans[:K], rep_plans=P.rep_plans[:K],
             req_prefix=P.req_prefix[:K], req_fixed=P.req_fixed[:K], rec=L.rec, recs=L.recs, qlay=L.qlay, slay=L.slay,
             req=L.req, rep=L.rep)
    rng = np.random.default_rng(7 + len(name) + len(lay))
    S.fill = [rng.integers(0, 256, s, dtype=np.uint8) if s else None for s, _ in L.qlay]
    return S


def tables(strides):
    return sum(3 * (-(-s // 16) * 16) + 16 for s in strides if s)


def test_tile_rule():
    for name in SETS:
        for lay in LAYS:
            for mode in MODES:
                S = side(name, lay, mode)
                tb = tables(s for s, _ in S.qlay)
                t = 256
                while t > 16 and t * max(S.req_fixed) > IMAGE - tb:
                    t //= 2
                assert S.req.tile == (t, IMAGE - tb), "the documented tile rule"
                if mode == "cols":
                    assert tb == 0 and S.req.tile == S.L.P.req.tile
    S = side("calc_echo", "natural", "mixed")
    assert S.rec == [False, True, False, True, False] and S.qlay[1] == (16, [8, 12]) and max(S.req_fixed) == 76
    assert S.req.tile == (256, IMAGE - 2 * (3 * 16 + 16)) == (256, 32640)
    assert side("calc_echo", "tight", "mixed").qlay[1] == (8, [0, 4])
    assert side("calc_echo", "tight", "recs").qlay[0] == (4, [0])  # a Number: a 4-byte struct
    assert side("sixteen", "s256", "recs").req.tile[1] == IMAGE - 8 * (3 * 256 + 16)


class LegOuts(Outs):
    """The var test's Outs with a record plan's columns replaced by its array of
    alloc[k] structs."""

    def __init__(self, S, alloc, chars):
        super().__init__(S, alloc, chars)
        self.recs = [empty(alloc[k] * S.qlay[k][0] + GUARD) if S.rec[k] else None for k in range(S.K)]
        for k in S.recs:
            self.cols[k] = self.offs[k] = None


def run_legs(S, O, raw, buf_len, offs, first, cap, scap, status=True, scratch=None, null_buf=False):
    """One call -> dict of what it wrote besides the columns and arrays (guards checked)."""
    n, K = len(offs), S.K
    d_buf = None if null_buf else dev(np.frombuffer(raw, np.uint8)[:buf_len]) if buf_len else empty(16)
    d_offs = None if null_buf else dev(np.asarray(offs, np.uint32)) if n else empty(16)
    nb = MixedFrames.index_bytes(n, K)
    sb = S.req.scratch_bytes(n)
    d_cls, d_index, d_counts = empty(n + GUARD), empty(nb + GUARD), empty(8 * (K + 1) + GUARD)
    d_ends, d_scratch = empty(8 * O.nslots + GUARD), empty(sb + GUARD) if scratch is None else scratch
    behind = d_scratch[sb:].clone()
    st = status_buf()
    st[:] = 0x5A  # the call resets it
    rc = S.req.unpack_requests(d_buf, buf_len, d_offs, n, O.cols, O.offs, scap, O.recs, S.fill, first, cap, d_cls,
                               d_index, nb, d_counts, d_ends, st if status else None, d_scratch, sb)
    assert rc == 0
    flags, bad = read_status(st) if status else (None, None)
    raw_cls = host(d_cls, n + GUARD)
    raw_index = host(d_index, nb + GUARD)
    assert (raw_cls[n:] == 0xA5).all() and (raw_index[nb:] == 0xA5).all()
    raw_counts = host(d_counts, 8 * (K + 1) + GUARD)
    raw_ends = host(d_ends, 8 * O.nslots + GUARD)
    assert (raw_counts[-GUARD:] == 0xA5).all() and (raw_ends[-GUARD:] == 0xA5).all()
    assert torch.equal(d_scratch[sb:], behind), "wrote past the scratch"
    return dict(cls=raw_cls[:n].copy(), counts=raw_counts[:8 * (K + 1)].view(np.uint64).copy(),
                ends=raw_ends[:8 * O.nslots].view(np.uint64).copy(), flags=flags, bad=bad, index=raw_index[:nb].copy(),
                d_cls=d_cls, d_index=d_index, d_buf=d_buf, d_offs=d_offs)


def expected_array(S, leg, k, want, src, f0, cap, alloc):
    """Plan k's array: 0xA5; the fill record over every classified element
    below the cap; the leaves of the elements the frames were packed from."""
    stride, loffs = S.qlay[k]
    exp = np.full((alloc, stride), 0xA5, np.uint8)
    idx = np.flatnonzero(want == k)
    e = f0 + cumcount(want)[idx]
    ok = e < cap
    e, el = e[ok], src[idx[ok]]
    exp[e] = S.fill[k]
    for c, o in zip(leg[0], loffs):
        s = c.dtype.itemsize
        exp[e, o:o + s] = np.ascontiguousarray(c[el]).view(np.uint8).reshape(len(el), s)
    return exp


def compare_legs(S, data, O, want, src, f0, cap, base, scap, ends=None, flags_bad=None):
    """The column plans through the var test's `compare` (as the plans of a call
    of their own: ranks and string slots are per plan, so nothing else changes),
    the record plans' arrays against numpy, the status over both."""
    colk = [k for k in range(S.K) if not S.rec[k]]
    remap = np.full(256, UNKNOWN, np.uint8)
    remap[colk] = np.arange(len(colk))
    pick = lambda rows: [rows[k] for k in colk]  # noqa: E731
    compare(View(methods=pick(S.methods)), pick(data),
            View(alloc=pick(O.alloc), chars=pick(O.chars), cols=pick(O.cols), offs=pick(O.offs)), remap[want], src,
            pick(f0), pick(cap), pick(base), pick(scap), ends=ends)
    rank = cumcount(want)
    bad = NONE
    for k in range(S.K):
        idx = np.flatnonzero(want == k)
        over = idx[f0[k] + rank[idx] >= cap[k]]
        if len(over):
            bad = min(bad, int(over[0]))
    if flags_bad is not None:
        assert flags_bad == ((BOUNDS, bad) if bad != NONE else (0, NONE))
    for k in S.recs:
        stride = S.qlay[k][0]
        raw = host(O.recs[k], O.alloc[k] * stride + GUARD)
        assert (raw[O.alloc[k] * stride:] == 0xA5).all(), "wrote past an array"
        got = raw[:O.alloc[k] * stride].reshape(O.alloc[k], stride)
        exp = expected_array(S, data[k], k, want, src, f0[k], cap[k], O.alloc[k])
        wrong = np.flatnonzero((got != exp).any(axis=1))
        assert wrong.size == 0, f"plan {k} struct {wrong[0]}: {got[wrong[0]].tolist()} != {exp[wrong[0]].tolist()}"


def sized(S, data, want, src, f0, cap, base, scap_cut=0):
    """-> (chars, scap): the bytes every string column gets and may take."""
    rank = cumcount(want)
    chars, scap = [], []
    for k, (_, rq, _) in enumerate(S.methods):
        idx = np.flatnonzero(want == k)
        el = src[idx[f0[k] + rank[idx] < cap[k]]]
        row_c, row_s = [], []
        for f, kind in enumerate(rq.kinds):
            if kind != STRING:
                row_c.append(None)
                row_s.append(None)
                continue
            total = int(np.diff(data[k][1][f].astype(np.int64))[el].sum()) if len(el) else 0
            b0 = base[k] if f0[k] else 0
            row_c.append(b0 + total)
            row_s.append(max(b0 + total - scap_cut, 0))
        chars.append(row_c)
        scap.append(row_s)
    return chars, scap


def check(S, data, frames, intent, src, buf_len=None, offs=None, first=None, cap=None, alloc=None, base=None, raw=None,
          scratch=None, status=True, null_buf=False):
    """Run the call on the frames and compare everything it wrote with the
    host's expectation.  data[k]: the leg plan k's frames were packed from;
    intent[i]: the class frame i was built to have (over S's plans); src[i]: the
    element of its plan's leg it was built from.  -> the run."""
    if raw is None:
        raw, o = joined(frames)
        offs = o[:-1] if offs is None else offs
        buf_len = len(raw) if buf_len is None else buf_len
    n, K = len(offs), S.K
    want = model(S, raw, buf_len, offs)
    assert np.array_equal(want, intent), "the stream is not what the test meant to build"
    counts = [int((want == k).sum()) for k in range(K)]
    f0 = [FRONT if S.rec[k] else 0 for k in range(K)] if first is None else list(first)
    base = [0] * K if base is None else list(base)
    cap = [f0[k] + counts[k] for k in range(K)] if cap is None else list(cap)
    if alloc is None:
        alloc = [max(cap[k], f0[k] + counts[k]) + (SPARE if S.rec[k] else 0) for k in range(K)]
    chars, scap = sized(S, data, want, src, f0, cap, base)
    O = LegOuts(S, alloc, chars)
    for k in range(K):  # the offsets a chunk before would have left at entry first[k]
        if f0[k] and f0[k] <= cap[k] and not S.rec[k]:
            for t in O.offs[k]:
                if t is not None:
                    t[8 * f0[k]:8 * f0[k] + 8] = torch.from_numpy(np.array([base[k]], np.uint64).view(np.uint8).copy())
    got = run_legs(S, O, raw, buf_len, offs, f0, cap, scap, status=status, scratch=scratch, null_buf=null_buf)
    assert np.array_equal(got["cls"], want)
    if n:
        assert np.array_equal(classify_cls(S, got["d_buf"], buf_len, got["d_offs"], n), want)
    assert got["counts"].tolist() == counts + [int((want == UNKNOWN).sum())]
    compare_legs(S, data, O, want, src, f0, cap, base, scap, ends=got["ends"],
                 flags_bad=(got["flags"], got["bad"]) if status else None)
    got.update(O=O, scap=scap, want=want, f0=f0, cap=cap, alloc=alloc, raw=raw, buf_len=buf_len, offs=offs)
    return got


def base_batch(name):
    """A batch whose legs the streams below take their frames from, element
    (rank mod the leg's count) of a frame's plan."""
    B = batch(name, 640, "uniform", regime_of(name))
    assert all(c > 0 for c in B.counts)
    return B


def stream_of(S, B, method, foreign=0.0, seed=0):
    """The frames of a method vector over S's plans -> (frames, intent, src)."""
    method = np.asarray(method, np.uint8)
    src = cumcount(method) % np.array(B.counts)[np.minimum(method, len(B.counts) - 1)]
    frames = [B.req[int(k)][2][0][int(e)] for k, e in zip(method, src)]
    intent = method.copy()
    if foreign > 0:
        rng = np.random.default_rng(seed + len(method))
        pick = np.arange(len(method)) if foreign >= 1.0 else np.flatnonzero(rng.random(len(method)) < foreign)
        for i in pick:
            frames[int(i)] = foreign_frame(B, int(i))
        intent[pick] = UNKNOWN
    return frames, intent, src


ORDERS = ["round_robin", "uniform", "runs", "absent", "single"]


def order(which, n, S, T):
    """absent: uniform without the first record plan; single: that plan alone."""
    if which in ("round_robin", "uniform", "runs"):
        return pattern(which, n, S.K, T, S.name)
    m = pattern("uniform", n, S.K, T, S.name)
    rk = S.recs[0]
    if which == "single":
        return np.full(n, rk, np.uint8)
    m[m == rk] = (rk + 1) % S.K
    return m


def sizes(T):
    return sorted({0, 1, T - 1, T, T + 1, 255, 256, 257, 4097})


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_sizes_and_orders(name, which, lay):
    S = side(name, lay, "mixed")
    B = base_batch(name)
    T = S.req.tile[0]
    rk = S.recs[0]
    for n in sizes(T):
        method = order(which, n, S, T)
        frames, intent, src = stream_of(S, B, method, 0.1 if n > 1 and which != "single" else 0.0)
        got = check(S, B.req, frames, intent, src)
        print(f"{name}/{which}/{lay} n={n} counts={got['counts'].tolist()} flags={got['flags']}")
        if which == "absent":
            assert got["counts"][rk] == 0
        if which == "single":
            assert got["counts"][rk] == n
        if n >= 255 and which in ("round_robin", "uniform"):
            assert all(got["counts"][k] > 0 for k in range(S.K)), "a frame of every class"
            assert got["counts"][S.K] > 0, "and unknown ones"


def test_tight_number_slices_share_pieces_with_neighbouring_tiles():
    """Every fixed plan in records, a Number a 4-byte struct: runs of T - 1, T,
    T + 1 frames of one plan, so a tile's slice starts and ends inside 16-byte
    pieces whose other bytes belong to the tiles before and after it."""
    S = side("calc_echo", "tight", "recs")
    T = S.req.tile[0]
    B = base_batch("calc_echo")
    n = 12 * T + 7
    method = pattern("runs", n, S.K, T, "calc_echo")
    frames, intent, src = stream_of(S, B, method)
    assert S.qlay[0][0] == 4 and S.rec[:4] == [True] * 4
    rank, shared = cumcount(method), 0
    for t in range(n // T):
        el = rank[t * T:(t + 1) * T][method[t * T:(t + 1) * T] == 0] + FRONT
        if len(el) and (4 * int(el[0])) % 16 and (4 * (int(el[-1]) + 1)) % 16:
            shared += 1
    assert shared >= 2, "a slice sharing its first and its last piece"
    check(S, B.req, frames, intent, src)


# ---- equivalence with the calls of one kind ------------------------------------------------------

PAIR = "calc_text2"  # test_gpu_mixed_var.PAIR_SETS: add, multiply and a method with two strings


@pytest.mark.parametrize("name", sorted(SETS) + [PAIR])
def test_all_columns_equals_mixed_var(name):
    """Every output of the two entry points over one all-column stream is the
    same, byte for byte.  PAIR: 600 frames in random order (more than two tiles of
    256, ending inside one), a tenth of them junk, strings of 0..16 bytes."""
    S = side(name, "natural", "cols")
    P = S.L.P
    assert not S.recs and S.K == P.K
    B = base_batch(name) if name != PAIR else batch(PAIR, 640, "uniform", "short")
    for n in ((600,) if name == PAIR else (S.req.tile[0] + 1, 4097)):
        frames, intent, src = stream_of(S, B, pattern("uniform", n, S.K, S.req.tile[0], name), 0.1)
        if name == PAIR:
            text = intent == 2
            lens = np.diff(np.asarray(B.req[2][1][0], np.int64))[src[text]]  # the first string of every string frame
            start = joined(frames)[1][:-1][text] + 4 + len(P.req_prefix[2]) + 8
            assert S.K == 3 and S.req.tile[0] == 256 and (intent == UNKNOWN).any() and (lens == 0).any()
            assert (start // 16 != (start + np.maximum(lens, 1) - 1) // 16).any(), "chars across a 16-byte piece"
        got = check(S, B.req, frames, intent, src)
        chars, scap = sized(S, B.req, got["want"], src, got["f0"], got["cap"], [0] * S.K)
        O = Outs(P, got["alloc"], chars)
        ref = run(P, O, got["raw"], got["buf_len"], got["offs"], got["f0"], got["cap"], scap)
        for key in ("cls", "counts", "ends"):
            assert np.array_equal(got[key], ref[key]), key
        assert (got["flags"], got["bad"]) == (ref["flags"], ref["bad"])
        nb = MixedFrames.index_bytes(n, S.K)
        assert np.array_equal(got["index"], host(ref["d_index"], nb)), "d_index"
        for k in range(S.K):
            for a, b in zip(got["O"].cols[k] + got["O"].offs[k], O.cols[k] + O.offs[k]):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), k


@pytest.mark.parametrize("lay", LAYS)
def test_all_records_equals_mixed_aos(lay):
    """Calculator's four fixed plans alone, all in records; the echo frames of
    the stream are nobody's."""
    S = side("calc_echo", lay, "recs", upto=4)
    assert S.rec == [True] * 4 and S.K == 4
    B = base_batch("calc_echo")
    for n in (257, 4097):
        method = pattern("uniform", n, 5, 256, "calc_echo")
        frames, intent, src = stream_of(S, B, method)
        intent[method == 4] = UNKNOWN
        assert (intent == UNKNOWN).any()
        got = check(S, B.req, frames, intent, src)
        mf = MixedAosFrames(S.req_plans, [s for s, _ in S.qlay], [o for _, o in S.qlay])
        nb = MixedFrames.index_bytes(n, 4)
        recs = [empty(got["alloc"][k] * S.qlay[k][0] + GUARD) for k in range(4)]
        d_cls, d_index, d_counts, st = empty(n), empty(nb), empty(8 * 5), status_buf()
        sb = mf.scratch_bytes
        assert mf.unpack_requests(got["d_buf"], got["buf_len"], got["d_offs"], n, recs, S.fill, got["f0"], got["cap"], d_cls,
                                  d_index, nb, d_counts, empty(sb + GUARD), sb, st) == 0
        assert np.array_equal(host(d_cls, n), got["cls"]) and np.array_equal(host(d_index, nb), got["index"])
        assert np.array_equal(host(d_counts, 40, np.uint64), got["counts"])
        assert read_status(st) == (got["flags"], got["bad"]) == (0, NONE)
        for k in range(4):
            assert torch.equal(recs[k], got["O"].recs[k]), k


# ---- a frame that a long string pushed out of the window ----------------------------------------

@pytest.mark.parametrize("lay", LAYS)
def test_long_string_pushes_record_frames_out_of_the_window(lay):
    """One echo request with a string longer than the image window in the middle
    of a tile, record plans' frames behind it in the same tile: whole fixed
    frames outside the staged span, which the piece step reads from the stream."""
    S = side("calc_echo", lay, "mixed")
    T, window = S.req.tile
    B0 = batch("calc_echo", 2 * T + 5, "uniform", "short")
    echo_calls = np.flatnonzero(B0.method[T:] == 4) + T
    at = int(echo_calls[np.searchsorted(echo_calls, T + T // 4)])  # an echo call in the middle of the second tile
    rq = B0.P.methods[4][1]
    lens = np.diff(np.array(B0.req[4][1][3]).astype(np.int64))[None, :].copy()
    lens[0][B0.rank[at]] = window + 1000
    B = copy.copy(B0)
    B.req = list(B0.req)
    B.req[4] = make_leg(rq, [B0.P.req_prefix[4]], B0.counts[4], lens, 17 + 4)
    frames, intent, src = stream(B)
    raw, offs = joined(frames)
    s0 = int(offs[T]) & ~15
    out = [i for i in range(at + 1, 2 * T) if S.rec[B.method[i]] and offs[i + 1] - s0 > window]
    assert T < at < 2 * T - 8 and len(frames[at]) > window and len(out) >= 3, "record plans' frames past the window"
    assert any(S.rec[B.method[i]] for i in range(T, at)), "and some inside it"
    check(S, B.req, frames, intent, src)


# ---- unknown and hostile frames ------------------------------------------------------------------

@pytest.mark.parametrize("foreign", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("name", sorted(SETS))
def test_foreign_share(name, foreign):
    S = side(name, "natural", "mixed")
    B = batch(name, 4097, "uniform", "short")
    frames, intent, src = stream(B, foreign, seed=1)
    got = check(S, B.req, frames, intent, src)
    unknown = int(got["counts"][S.K])
    if foreign == 0.1:
        assert 0 < unknown < 4097 and all(c > 0 for c in got["counts"].tolist())
    else:
        assert unknown == (4097 if foreign else 0)
    if foreign == 1.0:  # nothing written: every array is as it was allocated
        assert all((host(got["O"].recs[k], got["O"].recs[k].numel()) == 0xA5).all() for k in S.recs)


@pytest.mark.parametrize("what", sorted(VAR_EDITS) + sorted(FIXED_EDITS))
def test_hostile_frame(what):
    """The var test's edits of a good frame first in a tile, mid-tile, last in a
    tile and as the final frame of the buffer, among record plans' frames; the
    fixed edits are made of a record plan's frame."""
    S = side("calc_echo", "tight", "mixed")
    T = S.req.tile[0]
    B = batch("calc_echo", 3 * T + 5, "uniform", "mid")
    frames, intent, src = stream(B)
    k = hostile_plan(B.P, what) if what in VAR_EDITS else 1
    assert S.rec[k] == (what in FIXED_EDITS)
    edit = VAR_EDITS.get(what) or FIXED_EDITS[what]
    spots = [T, T + T // 2, 2 * T - 1, B.n - 1]
    for j, p in enumerate(spots):
        g = B.req[k][2][0][j]
        h = edit(B.P, k, g)
        assert h != g
        frames[p] = h
        intent[p] = UNKNOWN
    got = check(S, B.req, frames, intent, src)
    assert (got["cls"][spots] == UNKNOWN).all() and got["counts"][S.K] == len(spots)
    near = [p + d for p in spots for d in (-1, 1) if 0 <= p + d < B.n and p + d not in spots]
    assert (got["cls"][near] != UNKNOWN).all(), "the neighbours keep their classes"
    lone = check(S, B.req, [frames[-1]], np.array([UNKNOWN], np.uint8), np.zeros(1, np.int64))
    assert lone["counts"].tolist() == [0] * S.K + [1]


@pytest.mark.parametrize("lay", LAYS)
def test_offsets_out_of_order(lay):
    S = side("calc_echo", lay, "mixed")
    T = S.req.tile[0]
    B = batch("calc_echo", 3 * T + 5, "uniform", "mid")
    frames, intent, src = stream(B)
    raw, o = joined(frames)
    offs = o[:-1].copy()
    for p in (T, T + T // 2, 2 * T - 1):
        # frame p - 1 now spans three frames, frame p runs backwards, frame p + 1 is whole
        offs[p] = offs[p + 2]
        intent[p - 1] = intent[p] = UNKNOWN
    got = check(S, B.req, None, intent, src, raw=raw, buf_len=len(raw), offs=offs)
    assert got["counts"][S.K] == 6


def test_frames_past_buf_len():
    S = side("calc_echo", "natural", "mixed")
    B = batch("calc_echo", 700, "uniform", "mid")
    frames, intent, src = stream(B)
    raw, o = joined(frames)
    offs, total = o[:-1].copy(), len(raw)
    # the last frame cut by one byte
    cut = intent.copy()
    cut[-1] = UNKNOWN
    check(S, B.req, None, cut, src, raw=raw[:total - 1], buf_len=total - 1, offs=offs)
    # the last frame starts past buf_len: the one before it now ends past buf_len
    far = offs.copy()
    far[-1] = total + 8
    cut = intent.copy()
    cut[-2:] = UNKNOWN
    check(S, B.req, None, cut, src, raw=raw, buf_len=total, offs=far)
    # buf_len inside a record plan's frame: it and every later frame are nobody's
    at = int(np.flatnonzero((intent == 1) & (np.arange(B.n) >= 650))[0])
    cut = intent.copy()
    cut[at:] = UNKNOWN
    check(S, B.req, None, cut, src, raw=raw, buf_len=int(offs[at]) + 9, offs=offs)


# ---- h_first / h_cap -----------------------------------------------------------------------------

@pytest.mark.parametrize("lay", LAYS)
def test_short_arrays_and_columns(lay):
    """h_cap[k] short of the count for a record plan, a fixed column plan and
    the string plan: the excess frames keep their class and write nothing;
    BOUNDS with the smallest such i."""
    S = side("calc_echo", lay, "mixed")
    B = batch("calc_echo", 1000, "uniform", "mid")
    frames, intent, src = stream(B)
    for k in (1, 2, 4):
        first = [FRONT if S.rec[j] else 0 for j in range(S.K)]
        cap = [first[j] + B.counts[j] for j in range(S.K)]
        alloc = [c + SPARE for c in cap]
        cap[k] -= 3
        got = check(S, B.req, frames, intent, src, first=first, cap=cap, alloc=alloc)
        assert got["flags"] == BOUNDS and got["bad"] == int(np.flatnonzero(intent == k)[-3]) and got["cls"][got["bad"]] == k
        assert S.rec[k] == (k == 1)
    cap = [FRONT + B.counts[j] - (2 if j in (1, 2) else 0) for j in range(S.K)]
    got = check(S, B.req, frames, intent, src, first=[FRONT] * S.K, cap=cap, alloc=[c + SPARE + 2 for c in cap],
                base=[40] * S.K)
    assert got["bad"] == min(int(np.flatnonzero(intent == j)[-2]) for j in (1, 2))


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_three_chunks_equal_the_whole(name, lay):
    S = side(name, lay, "mixed")
    B = batch(name, 1000, "uniform", regime_of(name))
    frames, intent, src = stream(B, 0.05, seed=2)
    whole = check(S, B.req, frames, intent, src, first=[0] * S.K)
    O = LegOuts(S, whole["alloc"], whole["O"].chars)
    cap = whole["cap"]
    done = [0] * S.K
    for lo, hi in ((0, 1), (1, 513), (513, 1000)):
        raw, o = joined(frames[lo:hi])
        got = run_legs(S, O, raw, len(raw), o[:-1], list(done), cap, whole["scap"])
        assert (got["flags"], got["bad"]) == (0, NONE) and np.array_equal(got["cls"], intent[lo:hi])
        for k in range(S.K):
            done[k] += int((intent[lo:hi] == k).sum())
    assert np.array_equal(got["ends"], whole["ends"]) and any(done[k] for k in S.recs)
    compare_legs(S, B.req, O, intent, src, [0] * S.K, cap, [0] * S.K, whole["scap"])
    for k in S.recs:
        assert torch.equal(O.recs[k], whole["O"].recs[k])


# ---- scratch, status, no frames ------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SETS))
def test_scratch_left_by_another_call(name):
    S = side(name, "natural", "mixed")
    B = batch(name, 1000, "uniform", regime_of(name))
    frames, intent, src = stream(B, 0.05, seed=3)
    fresh = check(S, B.req, frames, intent, src)
    sb = S.req.scratch_bytes(4097)
    assert sb >= S.req.scratch_bytes(1000)
    scratch = torch.full((sb + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:0")
    scratch[sb:] = 0xA5
    ones = check(S, B.req, frames, intent, src, scratch=scratch)
    # a different call's contents: another layout's tables, another stream, more frames
    other = side(name, "s256", "recs")
    Bo = batch(name, 4097, "uniform", "short")
    big = torch.full((max(sb, other.req.scratch_bytes(4097)) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    fo, io, so = stream(Bo, 0.1, seed=1)
    check(other, Bo.req, fo, io, so, scratch=big)
    left = check(S, B.req, frames, intent, src, scratch=big)
    for got in (ones, left):
        for key in ("cls", "counts", "ends", "index"):
            assert np.array_equal(got[key], fresh[key]), key
        for k in S.recs:
            assert torch.equal(got["O"].recs[k], fresh["O"].recs[k])


def test_null_status_and_no_frames():
    S = side("calc_echo", "tight", "mixed")
    B = batch("calc_echo", 300, "uniform", "mid")
    frames, intent, src = stream(B, 0.1, seed=4)
    whole = check(S, B.req, frames, intent, src)  # the status was reset from a 0x5A fill
    assert (whole["flags"], whole["bad"]) == (0, NONE)
    check(S, B.req, frames, intent, src, status=False)
    for null_buf in (False, True):  # nframes == 0: d_buf and d_offs may be NULL
        got = check(S, B.req, [], np.zeros(0, np.uint8), np.zeros(0, np.int64), null_buf=null_buf)
        assert got["counts"].tolist() == [0] * (S.K + 1) and (got["ends"] == 0).all() and (got["flags"], got["bad"]) == (0, NONE)


# ---- the reply side: srpc_frames_pack_requests_mixed_legs over the response plans ----------------

@pytest.mark.parametrize("foreign", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("name", sorted(SETS))
def test_ordered_reply_pack(name, foreign):
    """d_method = d_class, the index the decode wrote, a record plan's replies in
    a struct array: the oracle's replies in arrival order, zero bytes at unknown
    frames, nothing at or past the total."""
    S = side(name, "natural", "mixed")
    for n in (1, 257, 4097):
        B = batch(name, n, "uniform", "short")
        if foreign and not B.counts[0]:
            continue
        frames, intent, src = stream(B, foreign, seed=5)
        got = check(S, B.req, frames, intent, src)
        good = intent != UNKNOWN
        rank = cumcount(intent)
        # response r of method k answers its r-th request in arrival order; the plans carry code 2
        parts = [B.rep[int(k)][2][2][int(r)] if g else b"" for k, r, g in zip(intent, rank, good)]
        want, woffs = joined(parts)
        cols, so, recs = [], [], []
        for k in range(S.K):
            if S.rec[k]:
                stride, loffs = S.slay[k]
                a = structs(B.rep[k][0], B.counts[k], stride, loffs, k)
                cols.append(None), so.append(None), recs.append(dev(a) if a.size else empty(16))
            else:
                cols.append([dev(c) for c in B.rep[k][0]])
                so.append([None if o is None else dev(o) for o in B.rep[k][1]])
                recs.append(None)
        counts = [int((intent == k).sum()) for k in range(S.K)]
        out_cap = len(want)
        d_out, d_offs, d_total = empty(out_cap + GUARD), empty(4 * (n + 1) + GUARD), empty(8 + GUARD)
        sb = S.rep.scratch_bytes(n)
        st = status_buf()
        st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
        rc = S.rep.pack(cols, so, recs, None, counts, got["d_cls"], got["d_index"], n, d_out, out_cap, d_offs, d_total, st,
                        empty(sb + GUARD), sb)
        assert rc == 0
        roffs = host(d_offs, 4 * (n + 1), np.uint32)
        assert (host(d_offs, 4 * (n + 1) + GUARD)[-GUARD:] == 0xA5).all()
        assert np.array_equal(roffs, woffs.astype(np.uint32)) and int(host(d_total, 8, np.uint64)[0]) == len(want)
        assert (roffs[1:][~good] == roffs[:-1][~good]).all()
        rawo = host(d_out, out_cap + GUARD)
        assert rawo[:out_cap].tobytes() == want and (rawo[out_cap:] == 0xA5).all()
        flags, bad = read_status(st)  # the pack's own flag: "unknown frames present", the first of them
        assert (flags, bad) == ((BOUNDS, int(np.flatnonzero(~good)[0])) if (~good).any() else (0, NONE))


# ---- refusals that need real plans ---------------------------------------------------------------

def test_refusals_in_order():
    """Past the argument checks (tests/test_requests_mixed_legs_abi.py):
    UNSUPPORTED, then INVALID for the layout, then ALIGN, then CAPACITY, nothing
    launched.  A refusal is shown to come first by making the later ones true as
    well."""
    S = side("calc_echo", "natural", "mixed")
    P = S.L.P
    n = 300
    nb = MixedFrames.index_bytes(n, S.K)
    sb = S.req.scratch_bytes(n)
    buf, offs, cls = empty(64 * n), empty(4 * n + 16), empty(n)
    idx, cnt, ends, scratch = empty(nb + 16), empty(8 * (S.K + 1) + 16), empty(64), empty(sb + 16)
    O = LegOuts(S, [n] * S.K, [[4096 if kind == STRING else None for kind in rq.kinds] for _, rq, _ in S.methods])
    scap = O.chars
    qs, qo = [s for s, _ in S.qlay], [o for _, o in S.qlay]
    z = np.zeros(512, np.uint8)

    def at(x, by):
        return x.data_ptr() + by

    def call(mf=S.req, buf=buf, offs=offs, idx=idx, nb_given=0, cnt=cnt, ends=ends, scratch=scratch, sb_given=0,
             cols=O.cols, so=O.offs, recs=O.recs, fill=S.fill):
        return mf.unpack_requests(buf, 64 * n, offs, n, cols, so, scap, recs, fill, None, [n] * S.K, cls, idx, nb_given,
                                  cnt, ends, None, scratch, sb_given)

    def req(strides=qs, leaf=qo, pl=P.req_plans):
        return MixedLegFrames(pl, strides, leaf)

    # 2. UNSUPPORTED, ahead of a bad layout, ALIGN and CAPACITY
    bad_leaf = [None, [8, 10], None, [8, 12]]  # add's leaves overlap: INVALID, were the plans supported
    for leaf in (qo[:4], bad_leaf):
        strung = req([0, 16, 0, 16, 64], leaf + [[0, 1, 8, 16]])
        kw = dict(mf=strung, recs=O.recs[:4] + [buf], fill=S.fill[:4] + [z])
        assert call(buf=at(buf, 1), **kw) == UNSUPPORTED, "a string plan with a stride"
        assert call(nb_given=nb, sb_given=1 << 20, **kw) == UNSUPPORTED
        wide = req([0, 16, 0, 272, 0], leaf + [None])
        assert call(mf=wide, buf=at(buf, 1), fill=S.fill[:3] + [z, None]) == UNSUPPORTED, "a stride of 272"
        short = [GpuPacker(srpc_amd.NUMBER, b"abc")] + P.req_plans[1:]
        assert call(mf=req(leaf=leaf + [None], pl=short), buf=at(buf, 1)) == UNSUPPORTED, "a prefix under 4 bytes"
    # 3. INVALID for the layout, ahead of ALIGN and CAPACITY
    assert call(mf=req(leaf=bad_leaf + [None]), buf=at(buf, 1)) == INVALID, "overlapping leaves"
    assert call(mf=req(leaf=[None, [8, 16], None, [8, 12], None]), buf=at(buf, 1)) == INVALID, "a leaf past the stride"
    # 4. ALIGN, with no index and no scratch at all: ahead of CAPACITY
    misaligned = {
        "d_buf (16)": dict(buf=at(buf, 8)), "an array (16)": dict(recs=[None, at(O.recs[1], 8), None, O.recs[3], None]),
        "a leaf's offset against its size": dict(mf=req(leaf=[None, [8, 12], None, [6, 12], None])),
        "a stride against its leaves": dict(mf=req(strides=[0, 16, 0, 18, 0])),
        "a fixed column (16)": dict(cols=[[at(O.cols[0][0], 8)]] + O.cols[1:]),
        "a string column (16)": dict(cols=O.cols[:4] + [O.cols[4][:3] + [at(O.cols[4][3], 8)]]),
        "a string's offsets array (8)": dict(so=O.offs[:4] + [O.offs[4][:3] + [at(O.offs[4][3], 4)]]),
        "the index (8)": dict(idx=at(idx, 4)), "d_counts (8)": dict(cnt=at(cnt, 4)), "d_ends (8)": dict(ends=at(ends, 4)),
        "the scratch (16)": dict(scratch=at(scratch, 8)), "d_offs (4)": dict(offs=at(offs, 2)),
    }
    for what, kw in misaligned.items():
        assert call(**kw) == ALIGN, what
    # 5. CAPACITY: the index, the scratch, each one byte short
    assert call(nb_given=nb - 1, sb_given=sb) == CAPACITY
    assert call(nb_given=nb, sb_given=sb - 1) == CAPACITY
    assert call(nb_given=nb, sb_given=P.req.scratch_bytes(n)) == CAPACITY, "the _mixed_var scratch lacks the tables"
    assert call(nb_given=0, sb_given=0) == CAPACITY
    torch.cuda.synchronize()
    outs = [cls, idx, cnt, ends] + [c for cc in O.cols if cc for c in cc] + [o for oo in O.offs if oo for o in oo if o is not None]
    for t in outs + [r for r in O.recs if r is not None]:
        assert (t.cpu().numpy() == 0xA5).all()  # refused: nothing launched
    offs.zero_()
    assert call(nb_given=nb, sb_given=sb) == 0


# ---- the refusals of the six string-aware entry points, one table --------------------------------

def error_table():
    """-> {entry: {wrong call: status}} of srpc_frames_{pack_requests, unpack_replies,
    unpack_requests}_mixed_{var, legs}.  Every entry starts from one valid call
    over 40 calls of Calculator + echo (_legs: add and multiply in records) and
    gets it back wrong in a single way -- a null for each required pointer,
    nplans 0 and 17, each size at 2^32, d_scratch off by 8 and by 4, the stream
    off by 8, the scratch or the index one byte short -- and then in two ways
    at once, which pins the order of the checks."""
    from tests import test_gpu_mixed_legs as lg
    from tests import test_gpu_mixed_var as mv
    lib = _lib.lib()
    S = side("calc_echo", "natural", "mixed")
    L, P, K, n = S.L, S.L.P, S.K, 40
    B = batch("calc_echo", n, "uniform", "short")
    assert all(B.counts) and S.rec == [False, True, False, True, False]
    d_method, d_index, _ = mv.build_index(B.method, K)
    nb = MixedFrames.index_bytes(n, K)
    short_req = GpuPacker(srpc_amd.NUMBER, b"abc")  # a framed prefix has 4 bytes at least: UNSUPPORTED on either side
    bad_plans = (C.c_void_p * K)(short_req._h.value, *[p._h.value for p in P.req_plans[1:]])

    def ptr(t, by=0):
        return t.data_ptr() + by

    def fills(rows):
        keep = [None if f is None else C.create_string_buffer(bytes(f), len(bytes(f))) for f in rows]
        return (C.c_void_p * K)(*[None if b is None else C.cast(b, C.c_void_p).value for b in keep]), keep

    def caps(mf, rows):
        return mf._table(rows, lambda x: 0 if x is None else int(x), C.c_uint64)

    def cases(entry, good, need, sizes, stream_key, legs_form, bad_plans=bad_plans):
        fn = getattr(lib, "srpc_frames_" + entry)

        def call(**edit):
            return int(fn(*dict(good, **edit).values()))  # the arguments in the order of include/srpc_gpu.h
        assert call() == 0, entry
        optional = ("h_first", "d_status", "stream")
        out = {f"null {k}": call(**{k: None}) for k, v in good.items()
               if k not in optional and (k.startswith("d_") or not isinstance(v, int))}
        out.update({"nplans 0": call(nplans=0), "nplans 17": call(nplans=17)})
        out.update({f"{k} 2^32": call(**{k: 1 << 32}) for k in sizes})
        sc = good["d_scratch"]
        out.update({"d_scratch + 8": call(d_scratch=sc + 8), "d_scratch + 4": call(d_scratch=sc + 4),
                    f"{stream_key} + 8": call(**{stream_key: good[stream_key] + 8}),
                    "scratch one byte short": call(scratch_bytes=need - 1)})
        if "index_bytes" in good:
            out["index one byte short"] = call(index_bytes=nb - 1)
        out["null d_index, d_scratch + 4"] = call(d_index=None, d_scratch=sc + 4)
        out["bad plan, scratch short"] = call(plans=bad_plans, scratch_bytes=need - 1)
        if legs_form:
            off = (C.c_void_p * K)(*good["d_recs"])
            off[1] += 8
            out["record array + 8, scratch short"] = call(d_recs=off, scratch_bytes=need - 1)
        table[entry] = out

    table, keep = {}, []
    # the request pack
    out, offs, total = empty(1 << 16), empty(4 * (n + 1)), empty(16)
    for form, mf in (("var", P.req), ("legs", L.req)):
        legs_form = form == "legs"
        cols, so, recs = lg.dev_req(L, B) if legs_form else ([mv.dev_leg(x)[0] for x in B.req],
                                                            [mv.dev_leg(x)[1] for x in B.req], None)
        c_arr, s_arr, _, h_cap = mf._args(cols, so, None, B.counts)
        need = P.req.scratch_bytes(n)  # a pack takes no tables: the _legs form needs what the _var form does
        scratch = empty(mf.scratch_bytes(n) + 64)
        good = dict(plans=mf._plans, nplans=K, d_cols=c_arr, d_str_offs=s_arr)
        if legs_form:
            good.update(d_recs=mf._recs(recs), h_stride=mf._strides, h_leaf_offs=mf._offs)
        good.update(h_first=None, h_cap=h_cap, d_method=ptr(d_method), d_index=ptr(d_index), ncalls=n, d_out=ptr(out),
                    out_cap=1 << 15, d_offs=ptr(offs), d_total=ptr(total), d_status=None, d_scratch=ptr(scratch),
                    scratch_bytes=need, stream=None)
        keep += [cols, so, recs, scratch, mf._keep]
        cases(f"pack_requests_mixed_{form}", good, need, ("ncalls", "out_cap"), "d_out", legs_form)
    # the reply decode
    buf, o = joined(B.rep_frames(np.zeros(n, np.int64)))
    d_buf, d_offs = dev(np.frombuffer(buf, np.uint8)), dev(o[:-1].astype(np.uint32))
    codes, ends = empty(n + 16), empty(8 * 16)
    bad_plans_rep = (C.c_void_p * K)(short_req._h.value, *[p._h.value for p in P.rep_plans[1:]])
    for form, mf, O in (("var", P.rep, mv.Outs(B)), ("legs", L.rep, lg.LegOuts(L, B))):
        legs_form = form == "legs"
        c_arr, s_arr, _, h_cap = mf._args(O.cols, O.offs, None, O.cap)
        cap_arr, k3 = caps(mf, O.scap)
        need = mf.scratch_bytes(n)
        scratch = empty(need + 64)
        good = dict(plans=mf._plans, nplans=K, d_buf=ptr(d_buf), buf_len=len(buf), d_offs=ptr(d_offs), nframes=n,
                    d_method=ptr(d_method), d_index=ptr(d_index), ncalls=n, unanswered=9, d_cols=c_arr, d_str_offs=s_arr,
                    h_str_cap=cap_arr)
        if legs_form:
            h_fill, kf = fills(L.fill)
            good.update(d_recs=mf._recs(O.recs), h_stride=mf._strides, h_leaf_offs=mf._offs, h_fill=h_fill)
            keep += [kf]
        good.update(h_first=None, h_cap=h_cap, d_codes=ptr(codes), d_ends=ptr(ends), d_status=None,
                    d_scratch=ptr(scratch), scratch_bytes=need, stream=None)
        keep += [O, scratch, mf._keep, k3]
        cases(f"unpack_replies_mixed_{form}", good, need, ("ncalls", "nframes", "buf_len"), "d_buf", legs_form,
              bad_plans_rep)
    # the request decode
    frames, intent, src = stream_of(S, B, B.method)
    raw, o = joined(frames)
    d_buf, d_offs = dev(np.frombuffer(raw, np.uint8)), dev(o[:-1].astype(np.uint32))
    cls, counts, index = empty(n + 16), empty(8 * (K + 1)), empty(nb + 16)
    alloc = [c + FRONT + SPARE for c in B.counts]
    chars, scap = sized(S, B.req, intent, src, [0] * K, alloc, [0] * K)
    for form, mf, O in (("var", P.req, Outs(P, alloc, chars)), ("legs", L.req, LegOuts(S, alloc, chars))):
        legs_form = form == "legs"
        c_arr, s_arr, _, h_cap = mf._args(O.cols, O.offs, None, alloc)
        cap_arr, k3 = caps(mf, scap)
        need = mf.scratch_bytes(n)
        scratch = empty(need + 64)
        good = dict(plans=mf._plans, nplans=K, d_buf=ptr(d_buf), buf_len=len(raw), d_offs=ptr(d_offs), nframes=n,
                    d_cols=c_arr, d_str_offs=s_arr, h_str_cap=cap_arr)
        if legs_form:
            h_fill, kf = fills(S.fill)
            good.update(d_recs=mf._recs(O.recs), h_stride=mf._strides, h_leaf_offs=mf._offs, h_fill=h_fill)
            keep += [kf]
        good.update(h_first=None, h_cap=h_cap, d_class=ptr(cls), d_index=ptr(index), index_bytes=nb, d_counts=ptr(counts),
                    d_ends=ptr(ends), d_status=None, d_scratch=ptr(scratch), scratch_bytes=need, stream=None)
        keep += [O, scratch, mf._keep, k3]
        cases(f"unpack_requests_mixed_{form}", good, need, ("nframes", "buf_len"), "d_buf", legs_form)
    torch.cuda.synchronize()
    return table


# What the parent commit (2987039) answers to error_table()'s calls, case by case; the fold keeps every one.
# `d_scratch + 8` is where the forms' scratch alignment shows (8 against 16).
PARENT_STATUS = {
    "pack_requests_mixed_var": {
        INVALID: ["null plans", "null d_cols", "null d_str_offs", "null h_cap", "null d_method", "null d_index",
                  "null d_out", "null d_offs", "null d_total", "null d_scratch", "nplans 0", "nplans 17",
                  "ncalls 2^32", "out_cap 2^32", "null d_index, d_scratch + 4"],
        0: ["d_scratch + 8"],
        ALIGN: ["d_scratch + 4", "d_out + 8"],
        CAPACITY: ["scratch one byte short"],
        UNSUPPORTED: ["bad plan, scratch short"],
    },
    "pack_requests_mixed_legs": {
        INVALID: ["null plans", "null d_cols", "null d_str_offs", "null d_recs", "null h_stride",
                  "null h_leaf_offs", "null h_cap", "null d_method", "null d_index", "null d_out", "null d_offs",
                  "null d_total", "null d_scratch", "nplans 0", "nplans 17", "ncalls 2^32", "out_cap 2^32",
                  "null d_index, d_scratch + 4"],
        ALIGN: ["d_scratch + 8", "d_scratch + 4", "d_out + 8", "record array + 8, scratch short"],
        CAPACITY: ["scratch one byte short"],
        UNSUPPORTED: ["bad plan, scratch short"],
    },
    "unpack_replies_mixed_var": {
        INVALID: ["null plans", "null d_buf", "null d_offs", "null d_method", "null d_index", "null d_cols",
                  "null d_str_offs", "null h_str_cap", "null h_cap", "null d_codes", "null d_ends",
                  "null d_scratch", "nplans 0", "nplans 17", "ncalls 2^32", "nframes 2^32", "buf_len 2^32",
                  "null d_index, d_scratch + 4"],
        0: ["d_scratch + 8"],
        ALIGN: ["d_scratch + 4", "d_buf + 8"],
        CAPACITY: ["scratch one byte short"],
        UNSUPPORTED: ["bad plan, scratch short"],
    },
    "unpack_replies_mixed_legs": {
        INVALID: ["null plans", "null d_buf", "null d_offs", "null d_method", "null d_index", "null d_cols",
                  "null d_str_offs", "null h_str_cap", "null d_recs", "null h_stride", "null h_leaf_offs",
                  "null h_fill", "null h_cap", "null d_codes", "null d_ends", "null d_scratch", "nplans 0",
                  "nplans 17", "ncalls 2^32", "nframes 2^32", "buf_len 2^32", "null d_index, d_scratch + 4"],
        ALIGN: ["d_scratch + 8", "d_scratch + 4", "d_buf + 8", "record array + 8, scratch short"],
        CAPACITY: ["scratch one byte short"],
        UNSUPPORTED: ["bad plan, scratch short"],
    },
    "unpack_requests_mixed_var": {
        INVALID: ["null plans", "null d_buf", "null d_offs", "null d_cols", "null d_str_offs", "null h_str_cap",
                  "null h_cap", "null d_class", "null d_index", "null d_counts", "null d_ends", "null d_scratch",
                  "nplans 0", "nplans 17", "nframes 2^32", "buf_len 2^32", "null d_index, d_scratch + 4"],
        0: ["d_scratch + 8"],
        ALIGN: ["d_scratch + 4", "d_buf + 8"],
        CAPACITY: ["scratch one byte short", "index one byte short"],
        UNSUPPORTED: ["bad plan, scratch short"],
    },
    "unpack_requests_mixed_legs": {
        INVALID: ["null plans", "null d_buf", "null d_offs", "null d_cols", "null d_str_offs", "null h_str_cap",
                  "null d_recs", "null h_stride", "null h_leaf_offs", "null h_fill", "null h_cap", "null d_class",
                  "null d_index", "null d_counts", "null d_ends", "null d_scratch", "nplans 0", "nplans 17",
                  "nframes 2^32", "buf_len 2^32", "null d_index, d_scratch + 4"],
        ALIGN: ["d_scratch + 8", "d_scratch + 4", "d_buf + 8", "record array + 8, scratch short"],
        CAPACITY: ["scratch one byte short", "index one byte short"],
        UNSUPPORTED: ["bad plan, scratch short"],
    },
}


def test_refusals_are_the_parent_commits():
    """Each of the six entry points answers every wrong call of error_table() as
    the parent commit did: the single faults, and the double faults that show
    which check fires first."""
    got = error_table()
    want = {e: {c: rc for rc, cs in by.items() for c in cs} for e, by in PARENT_STATUS.items()}
    assert got.keys() == want.keys()
    for e in want:
        diff = {c: (got[e].get(c), rc) for c, rc in want[e].items() if got[e].get(c) != rc}
        print(e, "differs in (got, parent):", diff)
        assert not diff and got[e].keys() == want[e].keys(), e
