"""Batches of calls of several methods in call order whose plans are held, plan
by plan, in columns (fixed-size or string) or in one device array of structs
(srpc_frames_pack_requests_mixed_legs / _unpack_replies_mixed_legs,
include/srpc_gpu.h).

The reference is tests/test_gpu_mixed_var.py's, used as it is: `batch` (the
method vector, every plan's inputs and the CPU oracle's frames per element),
`model` (the header's two judging tables restated), `check_pack` and
`check_outs`.  A plan's being a record plan changes where its values live and
nothing else, so the same Batch serves every assignment of kinds.  Nothing
expected comes from the kernels under test:
- expected frames are `oracle.pack`'s, interleaved by the method vector;
- expected columns, strings and offsets are `check_outs`'s;
- expected struct arrays are numpy: 0xA5, then for every good call the fill
  record with the call's leaves (zero where `model` finds no full frame);
- with every plan in columns / every plan in records the outputs are also
  compared with the _mixed_var / _mixed_aos calls' on the same values.
Outputs start 0xA5-filled with 16 guard bytes behind each.  Request structs
carry random bytes around their leaves.  Every case asserts that its input
holds the regime it names."""
import copy
import functools
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, MixedAosFrames, MixedLegFrames, _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402
from tests.test_gpu_mixed_aos import place  # noqa: E402
from tests.test_gpu_mixed_var import (BARE, NO_CODE, STRING, TIMEOUT, Outs, batch, build_index, check_outs,  # noqa: E402
                                      check_pack, cumcount, dev_leg, is_var, joined, make_leg, model, plans, run_pack,
                                      run_unpack)

PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
INVALID, ALIGN, UNSUPPORTED, CAPACITY = (_lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_UNSUPPORTED,
                                         _lib.SRPC_E_CAPACITY)
IMAGE = 32768
# calc_text: tests/test_gpu_mixed_var.py's calc_echo -- square, add, subtract, multiply and a string-bodied echo
SETS = {"calc_text": "calc_echo", "sixteen": "sixteen"}
LAYS = ["natural", "tight", "s256"]
ORDERS = ["round_robin", "uniform", "runs"]


def layout(schema, lay):
    """(stride, leaf offsets) of a fixed-size schema's struct:
    natural: the C++ layout behind an 8-byte vtable slot;
    tight:   the leaves packed from byte 0 (Number: a 4-byte struct);
    s256:    the leaves at the far end of 256 bytes, the largest stride a decode takes."""
    sizes = [oracle.KIND_SIZE[k] for k in schema.kinds]
    m = max(sizes)
    up = lambda x, a: -(-x // a) * a  # noqa: E731
    if lay == "natural":
        offs, end = place(sizes, 8)
        return up(end, 8), offs
    offs, end = place(sizes, 0)
    if lay == "tight":
        return up(end, m), offs
    base = (256 - end) // m * m
    return 256, [base + o for o in offs]


class Legs:
    """A set's plans with an assignment of kinds: mode `mixed` (calc_text: add
    and multiply in records; sixteen: every other fixed plan in records),
    `cols` (no record plan) or `recs` (every fixed plan in records); `upto`
    keeps the first plans only."""

    def __init__(self, name, lay, mode, upto=None):
        P = self.P = plans(SETS.get(name, name))
        self.K = K = upto or P.K
        fixed = [k for k in range(K) if not is_var(P.methods[k][1]) and not is_var(P.methods[k][2])]
        rec = {"cols": [], "recs": fixed, "mixed": fixed[1::2] if name == "calc_text" else fixed[0::2]}[mode]
        self.rec = [k in rec for k in range(K)]
        self.recs = [k for k in range(K) if self.rec[k]]
        self.qlay = [layout(P.methods[k][1], lay) if self.rec[k] else (0, None) for k in range(K)]
        self.slay = [layout(P.methods[k][2], lay) if self.rec[k] else (0, None) for k in range(K)]
        self.req = MixedLegFrames(P.req_plans[:K], [s for s, _ in self.qlay], [o for _, o in self.qlay])
        self.rep = MixedLegFrames(P.rep_plans[:K], [s for s, _ in self.slay], [o for _, o in self.slay])
        rng = np.random.default_rng(len(name) + len(lay))
        self.fill = [rng.integers(0, 256, s, dtype=np.uint8) if s else None for s, _ in self.slay]


@functools.lru_cache(maxsize=None)
def legs(name, lay, mode, upto=None):
    return Legs(name, lay, mode, upto)


def regime(name):
    return "mid" if name != "sixteen" else "short"


def sizes(T):
    return sorted({0, 1, T - 1, T, T + 1, 255, 256, 257, 4097})


def variant(B, method, rep=None):
    """B's legs under another method vector with no more calls of any plan (and
    another reply leg for some plans): (k, r) still names element r of plan k."""
    V = copy.copy(B)
    V.method = np.asarray(method, np.uint8)
    V.n = len(method)
    V.rank = cumcount(V.method)
    assert all(int(np.sum(V.method == k)) <= B.counts[k] for k in range(B.P.K))
    if rep:
        V.rep = [rep.get(k, leg) for k, leg in enumerate(B.rep)]
    return V


def test_sets_layouts_and_tile_rule():
    L = legs("calc_text", "natural", "mixed")
    assert [m[0].split("::")[1] for m in L.P.methods] == ["square", "add", "subtract", "multiply", "echo"]
    assert L.rec == [False, True, False, True, False] and is_var(L.P.methods[4][1]) and is_var(L.P.methods[4][2])
    assert L.qlay[1] == (16, [8, 12]) and L.slay[1] == (16, [8])
    assert legs("calc_text", "tight", "mixed").slay[3] == (4, [0])  # a packed 4-byte struct
    assert legs("calc_text", "s256", "mixed").slay[3] == (256, [252])
    S = legs("sixteen", "natural", "mixed")
    assert S.K == 16 and S.recs == [0, 4, 8, 12] and sum(is_var(m[1]) for m in S.P.methods) == 8
    for name in SETS:
        for lay in LAYS:
            for mode in ("mixed", "cols", "recs"):
                L = legs(name, lay, mode)
                tables = sum(3 * (-(-s // 16) * 16) + 16 for s, _ in L.slay if s)
                t = 256
                while t > 16 and t * max(L.P.rep_fixed) > IMAGE - tables:
                    t //= 2
                assert L.rep.tile == (t, IMAGE - tables), "the documented tile rule"
                assert L.rep.scratch_bytes(1000) == -(-L.P.rep.scratch_bytes(1000) // 16) * 16 + tables
                if mode == "cols":
                    assert L.rep.tile == L.P.rep.tile and L.req.tile == L.P.req.tile
    assert legs("sixteen", "s256", "recs").rep.tile[1] == IMAGE - 8 * (3 * 256 + 16)  # eight record plans' tables and fills


# ---- pack -------------------------------------------------------------------------------------------

def structs(cols, n, stride, offs, seed):
    """Elements [0, n) of a plan's columns as structs, random bytes around the leaves."""
    a = np.random.default_rng(seed).integers(0, 256, (max(n, 1), stride), dtype=np.uint8)[:n]
    for c, o in zip(cols, offs):
        s = c.dtype.itemsize
        a[:, o:o + s] = np.ascontiguousarray(c[:n]).view(np.uint8).reshape(n, s)
    return a


def dev_req(L, B):
    """-> (cols, str_offs, recs) of the request side: a record plan has no columns, a column plan no array."""
    cols, so, recs = [], [], []
    for k in range(L.K):
        if L.rec[k]:
            stride, offs = L.qlay[k]
            a = structs(B.req[k][0], B.counts[k], stride, offs, 5 + k)
            cols.append(None), so.append(None), recs.append(dev(a) if a.size else empty(16))
        else:
            c, o = dev_leg(B.req[k])
            cols.append(c), so.append(o), recs.append(None)
    return cols, so, recs


def run_pack_legs(L, B, method=None, out_cap=None, first=None, cap=None, args=None, want=None, scratch=None):
    """As test_gpu_mixed_var.run_pack -> (rc, out bytes, d_offs, total, flags, first bad)."""
    method = B.method if method is None else method
    n = len(method)
    d_method, d_index, _ = build_index(method, L.K)
    cols, so, recs = args or dev_req(L, B)
    if out_cap is None:
        out_cap = sum(len(f) for f in (want if want is not None else B.req_frames()))
    d_out = empty(out_cap + 16)
    d_offs = empty(4 * (n + 1) + 16)
    d_total = empty(8 + 16)
    sb = L.req.scratch_bytes(n)
    d_scratch = empty(sb + 16) if scratch is None else scratch  # the caller's own may be larger
    behind = d_scratch[sb:].clone()
    st = status_buf()
    st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
    rc = L.req.pack(cols, so, recs, first, cap or B.counts[:L.K], d_method, d_index, n, d_out, out_cap, d_offs, d_total,
                    st, d_scratch, sb)
    flags, bad = read_status(st)
    raw = host(d_out, out_cap + 16)
    assert (raw[out_cap:] == 0xA5).all(), "wrote at or past out_cap"
    assert (host(d_offs, 4 * (n + 1) + 16)[-16:] == 0xA5).all() and (host(d_total, 24)[8:] == 0xA5).all()
    assert torch.equal(d_scratch[sb:], behind), "wrote past the scratch"
    return rc, raw[:out_cap], host(d_offs, 4 * (n + 1), np.uint32), int(host(d_total, 8, np.uint64)[0]), flags, bad


@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_pack(name, which):
    T = legs(name, "natural", "mixed").req.tile[0]
    for n in sizes(T):
        B = batch(SETS[name], n, which, regime(name))
        for lay in LAYS:
            L = legs(name, lay, "mixed")
            got = run_pack_legs(L, B)
            print(f"{name}/{lay}/{which} n={n} rc={got[0]} total={got[3]} flags={got[4]}")
            check_pack(B, got)
            if n == 4097:
                assert all(B.counts[k] for k in L.recs) and any(B.counts[k] for k in range(L.K) if not L.rec[k])


def test_pack_50001():
    B = batch("calc_echo", 50_001, "uniform", "short")
    assert len(set(B.method)) == 5
    check_pack(B, run_pack_legs(legs("calc_text", "natural", "mixed"), B))


PAIR = "calc_text2"  # test_gpu_mixed_var.PAIR_SETS: add, multiply and a method with two strings each way


def pair_batch():
    """600 calls of PAIR in random order (more than two tiles of 256, ending
    inside one), strings of 0..16 bytes: some empty, some across a 16-byte
    piece of the stream."""
    B = batch(PAIR, 600, "uniform", "short")
    assert B.P.K == 3 and all(B.counts) and plans(PAIR).req.tile[0] == plans(PAIR).rep.tile[0] == 256
    P = plans(PAIR)
    for leg, frames, pl in ((B.req[2], B.req_frames(), len(P.req_prefix[2])),
                            (B.rep[2], B.rep_frames(np.zeros(600, np.int64)), len(P.rep_prefix[2]))):
        lens = np.diff(np.asarray(leg[1][0], np.int64))  # the first string of every element
        start = joined(frames)[1][:-1][B.method == 2] + 4 + pl + 8  # its chars' stream offset, by call
        assert (lens == 0).any() and (start // 16 != (start + np.maximum(lens, 1) - 1) // 16).any()
    return B


@pytest.mark.parametrize("name", sorted(SETS) + [PAIR])
def test_pack_all_columns_equals_mixed_var(name):
    """Every output of the two entry points over one all-column batch is the
    same, byte for byte: the stream, d_offs, d_total and the status words."""
    T = plans(SETS.get(name, name)).req.tile[0]
    for n in ((600,) if name == PAIR else (T + 1, 4097)):
        B = pair_batch() if name == PAIR else batch(SETS[name], n, "uniform", regime(name))
        L = legs(name, "natural", "cols")
        assert not L.recs and B.n == n
        got, ref = run_pack_legs(L, B), run_pack(B)
        check_pack(B, got)
        assert got[0] == ref[0] == 0 and got[3:] == ref[3:]
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("lay", LAYS)
def test_pack_all_records_equals_mixed_aos(lay):
    """Calculator's four fixed plans, all in records: the frames of the batch's
    calls of those plans, and what srpc_frames_pack_requests_mixed_aos writes."""
    L = legs("calc_text", lay, "recs", upto=4)
    assert L.rec == [True] * 4
    for n in (257, 4097):
        B = batch("calc_echo", n, "uniform", "mid")
        keep = B.method < 4  # dropping the other plan's calls leaves these plans' ranks as they were
        method = B.method[keep]
        V = variant(B, method)
        want = [f for f, k in zip(B.req_frames(), keep) if k]
        args = dev_req(L, B)
        got = run_pack_legs(L, V, args=args, want=want)
        check_pack(V, got)
        mf = MixedAosFrames(L.P.req_plans[:4], [s for s, _ in L.qlay], [o for _, o in L.qlay])
        d_method, d_index, _ = build_index(method, 4)
        total, cap = len(b"".join(want)), len(method) * max(len(f) for f in want)  # the call's own out_cap rule
        d_out, d_offs, st = empty(cap + 16), empty(4 * (len(method) + 1) + 16), status_buf()
        st[8:] = 0xFF
        assert mf.pack(args[2], None, B.counts[:4], d_method, d_index, len(method), d_out, cap, d_offs, st) == 0
        assert np.array_equal(host(d_out, total), got[1])
        assert np.array_equal(host(d_offs, 4 * (len(method) + 1), np.uint32), got[2])
        assert read_status(st)[0] == got[4] == 0


def test_pack_stride_above_what_a_decode_takes():
    """A pack reads leaves at any stride below 2^32; its scratch counts no table for such a plan."""
    B = batch("calc_echo", 1000, "uniform", "mid")
    L = copy.copy(legs("calc_text", "natural", "mixed"))
    L.qlay = list(L.qlay)
    L.qlay[1] = (520, [512, 516])
    L.req = MixedLegFrames(L.P.req_plans, [s for s, _ in L.qlay], [o for _, o in L.qlay])
    assert L.req.scratch_bytes(B.n) == legs("calc_text", "natural", "mixed").req.scratch_bytes(B.n) - (3 * 16 + 16)
    check_pack(B, run_pack_legs(L, B))


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_pack_in_two_chunks(name, lay):
    B = batch(SETS[name], 1000, "uniform", regime(name))
    L = legs(name, lay, "mixed")
    frames = B.req_frames()
    want, woffs = joined(frames)
    args = dev_req(L, B)
    for a in (1, 256, 999):
        counts = [int(np.sum(B.method[:a] == k)) for k in range(L.K)]
        assert any(counts[k] for k in L.recs) or a == 1
        h = run_pack_legs(L, B, method=B.method[:a], args=args, out_cap=int(woffs[a]))
        t = run_pack_legs(L, B, method=B.method[a:], args=args, out_cap=len(want) - int(woffs[a]), first=counts)
        assert h[0] == 0 and t[0] == 0 and h[4] == 0 and t[4] == 0
        assert h[1].tobytes() + t[1].tobytes() == want, a
        assert h[3] == int(woffs[a]) and t[3] == len(want) - int(woffs[a])


@pytest.mark.parametrize("lay", LAYS)
def test_pack_bad_calls(lay):
    """An id >= K, a record plan's and a column plan's rank past h_cap, and a
    decreasing pair of string offsets: no frame for the BAD call, BOUNDS, the
    smallest index."""
    B = batch("calc_echo", 1000, "uniform", "mid")
    L = legs("calc_text", lay, "mixed")
    method = B.method.copy()
    method[[300, 999]] = [5, 200]
    V = variant(B, method)
    cap = list(B.counts)
    cap[1] = int(np.sum(method == 1)) - 1  # add: a record plan
    cap[2] = int(np.sum(method == 2)) - 1  # subtract: a column plan
    good = (method < 5) & ~((method == 1) & (V.rank >= cap[1])) & ~((method == 2) & (V.rank >= cap[2]))
    args = dev_req(L, B)
    e = 7  # echo's element 7: its string's offsets pair decreases
    offs = np.array(B.req[4][1][3])
    assert offs[e + 1] > offs[e] > 0
    offs[e + 1] = offs[e] - 1
    args[1][4][3] = dev(offs)
    i = int(np.flatnonzero((method == 4) & (V.rank == e))[0])
    nxt = int(np.flatnonzero((method == 4) & (V.rank == e + 1))[0])
    good[i] = False
    assert (~good).sum() == 5 and L.rec[1] and not L.rec[2]
    parts = V.req_frames(good)
    rc, raw, got_offs, total, flags, bad = run_pack_legs(L, V, args=args, cap=cap, out_cap=len(b"".join(parts)) + 64)
    first = int(np.flatnonzero(~good)[0])
    assert rc == 0 and (flags, bad) == (BOUNDS, first)
    assert all(got_offs[j + 1] == got_offs[j] for j in np.flatnonzero(~good))
    # the element after the decreasing pair starts at the smaller offset: compare up to its call
    want, woffs = joined(parts[:nxt])
    assert raw[:len(want)].tobytes() == want and np.array_equal(got_offs[:nxt + 1], woffs.astype(np.uint32))


@pytest.mark.parametrize("name", sorted(SETS))
def test_pack_out_cap_one_byte_short(name):
    B = batch(SETS[name], 1000, "uniform", regime(name))
    L = legs(name, "natural", "mixed")
    want, woffs = joined(B.req_frames())
    for cap in (len(want), len(want) - 1):
        got = run_pack_legs(L, B, out_cap=cap)
        check_pack(B, got, out_cap=cap)
        if cap < len(want):
            assert (got[4], got[5]) == (BOUNDS, B.n - 1) and got[3] == len(want)


# ---- decode -----------------------------------------------------------------------------------------

class LegOuts(Outs):
    """test_gpu_mixed_var.Outs, a record plan's columns replaced by its array
    of cap[k] structs (EXTRA of them behind the leg's calls)."""

    def __init__(self, L, B, str_cap_cut=0):
        super().__init__(B, str_cap_cut)
        self.L = L
        self.recs = [empty(self.cap[k] * L.slay[k][0] + 16) if L.rec[k] else None for k in range(L.K)]
        for k in L.recs:
            self.cols[k] = self.offs[k] = self.scap[k] = None


def run_unpack_legs(L, B, O, buf, buf_len, offs, nframes, lo=0, hi=None, first=None, stream=None, scratch=None):
    """One decode of calls [lo, hi) -> (rc, codes, ends, flags, first bad)."""
    method = B.method[lo:hi]
    n = len(method)
    d_method, d_index, _ = build_index(method, L.K)
    d_buf = dev(np.frombuffer(buf, np.uint8)) if buf else empty(16)
    d_offs = dev(np.asarray(offs, np.uint32)) if nframes else empty(16)
    d_codes = empty(n + 16)
    d_ends = empty(8 * O.nslots + 16)
    sb = L.rep.scratch_bytes(n)
    d_scratch = empty(sb + 16) if scratch is None else scratch  # the caller's own may be larger
    behind = d_scratch[sb:].clone()
    st = status_buf()
    rc = L.rep.unpack(d_buf, buf_len, d_offs, nframes, d_method, d_index, n, TIMEOUT, O.cols, O.offs, O.scap, O.recs,
                      L.fill, first, O.cap, d_codes, d_ends, st, d_scratch, sb, stream=stream)
    flags, bad = read_status(st)
    assert (host(d_codes, n + 16)[n:] == 0xA5).all() and (host(d_ends, 8 * O.nslots + 16)[8 * O.nslots:] == 0xA5).all()
    assert torch.equal(d_scratch[sb:], behind), "wrote past the scratch"
    return rc, host(d_codes, n).copy(), host(d_ends, 8 * O.nslots, np.uint64).copy(), flags, bad


def expected_structs(L, B, k, full, touched, ncap):
    """Plan k's array: 0xA5, then for every good call (k, r) decoded so far
    element r = the fill with the call's leaves, zero where it is not full."""
    stride, offs = L.slay[k]
    exp = np.full((ncap, stride), 0xA5, np.uint8)
    calls = np.flatnonzero((B.method == k) & touched)
    el = B.rank[calls]
    keep = el < ncap
    calls, el = calls[keep], el[keep]
    exp[el] = L.fill[k]
    for c, o in zip(B.rep[k][0], offs):
        s = c.dtype.itemsize
        vals = np.ascontiguousarray(np.where(full[calls], c[el], 0).astype(c.dtype))
        exp[el, o:o + s] = vals.view(np.uint8).reshape(len(el), s)
    return exp


def check_legs(L, B, O, full, touched=None, ends=None, cap=None):
    touched = np.ones(B.n, bool) if touched is None else touched
    check_outs(B, O, full, touched=touched, ends=ends, skip=L.recs)
    for k in L.recs:
        stride = L.slay[k][0]
        raw = host(O.recs[k], O.cap[k] * stride + 16)
        assert (raw[O.cap[k] * stride:] == 0xA5).all(), "wrote past an array"
        got = raw[:O.cap[k] * stride].reshape(O.cap[k], stride)
        exp = expected_structs(L, B, k, full, touched, (cap or O.cap)[k])
        exp = np.concatenate([exp, np.full((O.cap[k] - len(exp), stride), 0xA5, np.uint8)])
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, f"plan {k} struct {bad[0]}: {got[bad[0]].tolist()} != {exp[bad[0]].tolist()}"


def decode_and_check(L, B, parts, nframes=None, buf_len_cut=0, offs_edit=None, str_cap_cut=0, scratch=None):
    nframes = B.n if nframes is None else nframes
    buf, offs = joined(parts[:nframes])
    offs = offs[:nframes].copy()
    if offs_edit:
        offs_edit(offs)
    buf_len = len(buf) - buf_len_cut
    O = LegOuts(L, B, str_cap_cut)
    rc, codes, ends, flags, bad = run_unpack_legs(L, B, O, buf, buf_len, offs, nframes, scratch=scratch)
    wc, full, wflags, wbad = model(buf, buf_len, offs, nframes, B, [0] * B.P.K, O.cap)
    print(f"n={B.n} nframes={nframes} rc={rc} flags={flags} first={bad} want flags={wflags} first={wbad}")
    assert rc == 0
    assert np.array_equal(codes[:nframes], wc) and (codes[nframes:] == TIMEOUT).all()
    assert (flags, bad) == (wflags, wbad)
    allfull = np.zeros(B.n, bool)
    allfull[:nframes] = full
    check_legs(L, B, O, allfull, ends=ends)
    return codes, allfull, flags, bad, ends, O


@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_all_full(name, which):
    """All-full streams with codes 0, 1, 2, every size and layout."""
    for lay in LAYS:
        L = legs(name, lay, "mixed")
        for n in sizes(L.rep.tile[0]):
            B = batch(SETS[name], n, which, regime(name))
            codes = np.random.default_rng(n).integers(0, 3, n)
            got, full, flags, _, _, _ = decode_and_check(L, B, B.rep_frames(codes))
            assert full.all() and flags == 0 and np.array_equal(got, codes.astype(np.uint8))


@pytest.mark.parametrize("mode", ["cols", "recs"])
def test_decode_one_kind_only(mode):
    B = batch("calc_echo", 4097, "uniform", "mid")
    L = legs("calc_text", "natural", mode)
    _, full, flags, _, _, _ = decode_and_check(L, B, B.rep_frames(np.zeros(B.n, np.int64)))
    assert full.all() and flags == 0 and len(L.recs) == (4 if mode == "recs" else 0)


def test_decode_all_columns_equals_mixed_var():
    """The two entry points over one all-column batch and one reply stream -- a
    bare error frame, a junk frame, the last 5 calls unanswered -- leave the same
    bytes everywhere: codes, d_ends, the status words, every column and every
    offsets array."""
    B, L = pair_batch(), legs(PAIR, "natural", "cols")
    rng = np.random.default_rng(600)
    parts = B.rep_frames(rng.integers(0, 3, B.n))
    bare, junk, nframes = int(np.flatnonzero(B.method == 0)[40]), int(np.flatnonzero(B.method == 2)[90]), B.n - 5
    parts[bare] = BARE
    parts[junk] = struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091)
    assert not L.recs and 256 < junk < 512 and bare < nframes
    buf, offs = joined(parts[:nframes])
    offs = offs[:nframes]
    O_var, O_legs = Outs(B), LegOuts(L, B)
    ref = run_unpack(B, O_var, buf, len(buf), offs, nframes)
    got = run_unpack_legs(L, B, O_legs, buf, len(buf), offs, nframes)
    wc, full, wflags, wbad = model(buf, len(buf), offs, nframes, B, [0] * 3, O_var.cap)
    assert ref[0] == got[0] == 0 and (wflags, wbad) == (PREFIX, junk) and not full[bare] and not full[junk]
    assert np.array_equal(ref[1][:nframes], wc) and (ref[1][nframes:] == TIMEOUT).all() and ref[1][bare] == BARE[4]
    print(f"codes {np.bincount(ref[1]).tolist()} ends {ref[2].tolist()} status {ref[3:]} / {got[3:]}")
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and got[3:] == ref[3:] == (wflags, wbad)
    for k in range(3):
        for a, b in zip(O_legs.cols[k] + O_legs.offs[k], O_var.cols[k] + O_var.offs[k]):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), k
    check_outs(B, O_var, np.concatenate([full, np.zeros(5, bool)]), ends=ref[2])


def test_decode_50001():
    B = batch("calc_echo", 50_001, "uniform", "short")
    codes = np.random.default_rng(5).integers(0, 3, B.n)
    _, full, flags, _, _, _ = decode_and_check(legs("calc_text", "natural", "mixed"), B, B.rep_frames(codes))
    assert full.all() and flags == 0


@pytest.mark.parametrize("share", [0.1, 0.9])
@pytest.mark.parametrize("lay", LAYS)
def test_decode_bare_error_frames(lay, share):
    B = batch("calc_echo", 4097, "uniform", "mid")
    L = legs("calc_text", lay, "mixed")
    rng = np.random.default_rng(int(share * 10))
    bare = rng.random(B.n) < share
    parts = [struct.pack(">IB", 1, 3) if b else p for b, p in zip(bare, B.rep_frames(np.zeros(B.n, np.int64)))]
    assert abs(bare.mean() - share) < 0.03 and all(bare[B.method == k].any() and not bare[B.method == k].all() for k in range(5))
    codes, full, flags, _, _, _ = decode_and_check(L, B, parts)
    assert flags == 0 and np.array_equal(full, ~bare) and (codes[bare] == 3).all()


BAD_FIXED = ["wrong_name", "bare_code0", "one_longer", "junk_4k", "cut_last", "swapped", "empty_payload", "short_prefix",
             "other_plan"]  # include/srpc_gpu.h: the table of srpc_frames_unpack_replies
BAD_VAR = ["str_past_end", "ends_early", "len_2_63", "len_2_64m1"]  # ... and what srpc_frames_unpack_replies_var adds


def bad_frame(case, B, at, rng):
    """-> (the bad frame or None, bytes cut off the buffer, an edit of the
    offsets or None, (code, flag) expected at `at` or None)."""
    P = B.P
    k = int(B.method[at])
    kinds = P.methods[k][2].kinds
    var = STRING in kinds
    good = B.rep[k][2][0][B.rank[at]]
    pl = len(P.rep_prefix[k])
    first_str = 4 + pl + sum(oracle.KIND_SIZE[x] for x in kinds[:list(kinds).index(STRING)]) if var else 0
    if case == "wrong_name":
        b = bytearray(good)
        b[4 + pl - 1] ^= 0x20
        return bytes(b), 0, None, (0, PREFIX)
    if case == "bare_code0":
        return struct.pack(">IB", 1, 0), 0, None, (0, PREFIX)
    if case == "one_longer":  # a string plan's walk ends before the frame's end
        return struct.pack(">I", len(good) - 3) + good[4:] + b"\x00", 0, None, (0, BOUNDS if var else PREFIX)
    if case == "junk_4k":
        return struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091), 0, None, (7, PREFIX)
    if case == "cut_last":
        return None, 2, None, (NO_CODE, BOUNDS)
    if case == "swapped":
        def edit(o):
            o[at], o[at + 1] = o[at + 1], o[at]
        return None, 0, edit, None
    if case == "empty_payload":
        return struct.pack(">I", 0), 0, None, (NO_CODE, BOUNDS)
    if case == "short_prefix":
        body = good[4:4 + pl - 2]
        return struct.pack(">I", len(body)) + body, 0, None, (0, PREFIX)
    if case == "other_plan":  # a frame that is valid for another plan than its call's
        other = next(j for j in range(P.K) if P.rep_prefix[j] != P.rep_prefix[k] and B.counts[j])
        return B.rep[other][2][0][0], 0, None, (0, PREFIX)
    b = bytearray(good)
    if case == "str_past_end":
        b[first_str:first_str + 8] = struct.pack("<Q", len(good))
        return bytes(b), 0, None, (0, BOUNDS)
    if case == "ends_early":
        return struct.pack(">I", len(good) + 3) + good[4:] + b"\x00" * 7, 0, None, (0, BOUNDS)
    b[first_str:first_str + 8] = struct.pack("<Q", 2**63 if case == "len_2_63" else 2**64 - 1)
    return bytes(b), 0, None, (0, BOUNDS)


@pytest.mark.parametrize("case", BAD_FIXED + BAD_VAR)
def test_decode_one_bad_frame(case):
    """Each bad-frame kind of both judging tables at call 0, T - 1, T and the
    last one, under a record plan's call, a fixed column plan's and (every
    kind) the string plan's, among full frames of mixed codes; every frame
    around it still decodes, and the bad call's struct gets zero leaves."""
    L = legs("calc_text", "tight", "mixed")
    T = L.rep.tile[0]
    B0 = batch("calc_echo", 2 * T + 5, "uniform", "mid")
    rng = np.random.default_rng(len(case))
    codes = rng.integers(0, 3, B0.n)
    for plan in ([4] if case in BAD_VAR else [1, 2, 4]):  # add (records), subtract (columns), echo (strings)
        for at in (0, T - 1, T, B0.n - 1):
            if (case == "cut_last" and at != B0.n - 1) or (case == "swapped" and at == B0.n - 1):
                continue
            method = B0.method.copy()
            j = int(np.flatnonzero(method == plan)[3])  # put a call of `plan` at `at`
            method[j], method[at] = method[at], method[j]
            B = variant(B0, method)
            assert B.method[at] == plan and L.rec[plan] == (plan == 1)
            parts = B.rep_frames(codes)
            frame, cut, edit, want_at = bad_frame(case, B, at, rng)
            if frame is not None:
                parts[at] = frame
            got, full, flags, bad, _, _ = decode_and_check(L, B, parts, buf_len_cut=cut, offs_edit=edit)
            assert not full[at] and flags and bad <= at
            if want_at:
                assert got[at] == want_at[0] and flags & want_at[1] and bad == at
            assert full.sum() >= B.n - 3  # the others decode (a swapped pair spoils the frame before it and both its own)


@pytest.mark.parametrize("lay", LAYS)
def test_decode_nframes_below_ncalls(lay):
    B = batch("calc_echo", 1000, "uniform", "mid")
    L = legs("calc_text", lay, "mixed")
    parts = B.rep_frames(np.zeros(B.n, np.int64))
    for nf in (0, 1, B.n // 2, B.n - 1):
        codes, full, flags, _, _, _ = decode_and_check(L, B, parts, nframes=nf)
        assert flags == 0 and full.sum() == nf and (codes[nf:] == TIMEOUT).all()


@pytest.mark.parametrize("lay", LAYS)
def test_decode_bad_calls_keep_0xa5(lay):
    """Ids >= K and ranks past h_cap (a record plan's, a column plan's): BOUNDS,
    NO_CODE, and not a byte of any struct or column for them."""
    B0 = batch("calc_echo", 1000, "uniform", "mid")
    L = legs("calc_text", lay, "mixed")
    method = B0.method.copy()
    method[[300, 999]] = [5, 200]
    B = variant(B0, method)
    parts = [BARE if k >= 5 else B.rep[k][2][0][r] for k, r in zip(B.method, B.rank)]
    buf, offs = joined(parts)
    O = LegOuts(L, B)
    cap = list(O.cap)
    cap[1] = int(np.sum(method == 1)) - 1
    cap[2] = int(np.sum(method == 2)) - 1
    alloc, O.cap = O.cap, cap  # the buffers keep their size
    rc, codes, ends, flags, bad = run_unpack_legs(L, B, O, buf, len(buf), offs[:-1], B.n)
    badcall = (method >= 5) | ((method == 1) & (B.rank >= cap[1])) | ((method == 2) & (B.rank >= cap[2]))
    assert badcall.sum() == 4
    assert rc == 0 and (flags, bad) == (BOUNDS, int(np.flatnonzero(badcall)[0]))
    assert (codes[badcall] == NO_CODE).all() and (codes[~badcall] == 0).all()
    O.cap = alloc
    check_legs(L, B, O, ~badcall, touched=~badcall, cap=cap)


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_in_two_chunks(name, lay):
    """Two chunks into the same arrays and columns, h_first advanced, the
    absolute string offsets continuing across them."""
    B = batch(SETS[name], 1000, "uniform", regime(name))
    L = legs(name, lay, "mixed")
    codes = np.random.default_rng(3).integers(0, 3, B.n)
    parts = B.rep_frames(codes)
    for a in (1, 256, 999):
        O = LegOuts(L, B)
        buf, offs = joined(parts[:a])
        rc, c1, _, flags, _ = run_unpack_legs(L, B, O, buf, len(buf), offs[:-1], a, lo=0, hi=a)
        assert rc == 0 and flags == 0
        check_legs(L, B, O, np.ones(B.n, bool), touched=np.arange(B.n) < a)
        first = [int(np.sum(B.method[:a] == k)) for k in range(L.K)]
        buf, offs = joined(parts[a:])
        rc, c2, ends, flags, _ = run_unpack_legs(L, B, O, buf, len(buf), offs[:-1], B.n - a, lo=a, first=first)
        assert rc == 0 and flags == 0 and np.array_equal(np.concatenate([c1, c2]), codes.astype(np.uint8))
        check_legs(L, B, O, np.ones(B.n, bool), ends=ends)
        if a == 256:
            assert any(first[k] for k in L.recs) and any(e > 0 for e in ends)


def test_decode_str_cap_one_byte_short():
    B = batch("calc_echo", 1000, "uniform", "mid")
    L = legs("calc_text", "natural", "mixed")
    for cut in (0, 1):
        _, full, flags, _, ends, O = decode_and_check(L, B, B.rep_frames(np.zeros(B.n, np.int64)), str_cap_cut=cut)
        assert full.all() and flags == 0 and len(ends) == 1 and int(ends[0]) == O.scap[4][3] + cut


@pytest.mark.parametrize("lay", LAYS)
def test_decode_long_string_pushes_record_frames_out_of_the_image(lay):
    """A reply with a 40,000-char string, followed in the same tile by record
    plans' frames: full fixed frames outside the image window, whose leaves
    the piece step reads from the stream itself."""
    L = legs("calc_text", lay, "mixed")
    T, window = L.rep.tile
    B0 = batch("calc_echo", 2 * T + 5, "uniform", "short")
    at = int(np.flatnonzero(B0.method[T:] == 4)[0]) + T  # the second tile's first echo call
    rs = B0.P.methods[4][2]
    lens = np.diff(np.array(B0.rep[4][1][3]).astype(np.int64))[None, :].copy()
    lens[0][B0.rank[at]] = 40_000
    echo = make_leg(rs, [oracle.response_prefix(c, rs.name) for c in (0, 1, 2)], B0.counts[4], lens, 91 + 4)
    B = variant(B0, B0.method, rep={4: echo})
    parts = B.rep_frames(np.zeros(B.n, np.int64))
    buf, offs = joined(parts)
    s0 = int(offs[T]) & ~15
    out = [i for i in range(at + 1, 2 * T) if L.rec[B.method[i]] and offs[i + 1] - s0 > window]
    assert at < 2 * T - 8 and len(parts[at]) > 40_000 and len(out) >= 3, "record plans' frames past the window"
    _, full, flags, _, _, _ = decode_and_check(L, B, parts)
    assert full.all() and flags == 0


def test_decode_tight_slices_share_pieces_with_both_neighbours():
    """Runs of T - 1, T, T + 1 calls of one plan over 4-byte structs: a tile's
    slice of a record plan starts and ends inside 16-byte pieces whose other
    bytes belong to the tiles before and after it."""
    L = legs("calc_text", "tight", "recs")
    T = L.rep.tile[0]
    n = 12 * T + 7
    B = batch("calc_echo", n, "runs", "mid")
    assert L.slay[0][0] == 4 and L.rec[:4] == [True] * 4
    shared = 0  # slices whose first and last piece also hold bytes of the plan's slices before and after
    for t in range(n // T):
        for k in L.recs:
            el = B.rank[t * T:(t + 1) * T][B.method[t * T:(t + 1) * T] == k]
            if len(el) and (4 * int(el[0])) % 16 and (4 * (int(el[-1]) + 1)) % 16 and int(el[-1]) + 1 < B.counts[k]:
                shared += 1
    assert shared >= 2, "a slice sharing its first and its last piece"
    codes = np.random.default_rng(9).integers(0, 3, n)
    _, full, flags, _, _, _ = decode_and_check(L, B, B.rep_frames(codes))
    assert full.all() and flags == 0


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_round_trip(name, lay):
    """The pack as a server's ordered reply pack (the response plans, the reply
    values in records and columns), its stream handed back unchanged as the
    replies, then the decode: the values come back, every code is the plans'."""
    B = batch(SETS[name], 1000, "uniform", regime(name))
    L = legs(name, lay, "mixed")
    n = B.n
    d_method, d_index, _ = build_index(B.method, L.K)
    cols, so, recs = [], [], []
    for k in range(L.K):
        if L.rec[k]:
            stride, offs = L.slay[k]
            cols.append(None), so.append(None), recs.append(dev(structs(B.rep[k][0], B.counts[k], stride, offs, k)))
        else:
            c, o = dev_leg(B.rep[k])
            cols.append(c), so.append(o), recs.append(None)
    want, woffs = joined(B.rep_frames(np.full(n, 2)))  # the reply plans were made with code 2
    d_out, d_offs, d_total = empty(len(want) + 16), empty(4 * (n + 1) + 16), empty(24)
    sb = L.rep.scratch_bytes(n)
    st = status_buf()
    assert L.rep.pack(cols, so, recs, None, B.counts, d_method, d_index, n, d_out, len(want), d_offs, d_total, st,
                      empty(sb), sb) == 0
    stream = host(d_out, len(want)).tobytes()
    offs = host(d_offs, 4 * (n + 1), np.uint32)
    assert stream == want and np.array_equal(offs, woffs.astype(np.uint32)) and read_status(st)[0] == 0
    O = LegOuts(L, B)
    rc, codes, ends, flags, _ = run_unpack_legs(L, B, O, stream, len(stream), offs[:-1], n)
    assert rc == 0 and flags == 0 and (codes == 2).all()
    check_legs(L, B, O, np.ones(n, bool), ends=ends)


def test_refusals_in_order():
    """Past the argument checks (tests/test_mixed_legs_abi.py): UNSUPPORTED, then
    INVALID for the layout, then ALIGN, then CAPACITY, nothing launched.  A
    refusal is shown to come first by making the later ones true as well."""
    B = batch("calc_echo", 1000, "uniform", "mid")
    L = legs("calc_text", "natural", "mixed")
    P = B.P
    d_method, d_index, _ = build_index(B.method, P.K)
    cols, so, recs = dev_req(L, B)
    out, offs, total, scratch = empty(1 << 20), empty(4 * 1001), empty(16), empty(1 << 20)
    sb = L.req.scratch_bytes(B.n)
    qs, qo = [s for s, _ in L.qlay], [o for _, o in L.qlay]

    def at(x, by):
        return x.data_ptr() + by

    def pack(mf=L.req, cols=cols, so=so, recs=recs, index=d_index, out=out, offs=offs, total=total, scratch=scratch,
             sb_given=0):
        return mf.pack(cols, so, recs, None, B.counts, d_method, index, B.n, out, 1 << 19, offs, total, None, scratch,
                       sb_given)

    def req(strides=qs, leaf=qo, pl=P.req_plans):
        return MixedLegFrames(pl, strides, leaf)

    assert pack(sb_given=sb) == 0
    short = [GpuPacker(srpc_amd.NUMBER, b"abc")] + P.req_plans[1:]
    rec5 = [None, recs[1], None, recs[3], out]  # an array for the string plan too: past the argument checks
    bad_leaf = [None, [8, 10], None, [8, 12]]   # add's leaves overlap: INVALID, were the plans supported
    for leaf in (qo[:4], bad_leaf):
        strung = req([0, 16, 0, 16, 64], leaf + [[0, 1, 8, 16]])
        assert pack(mf=strung, recs=rec5, out=at(out, 1)) == UNSUPPORTED, "a string plan with a stride"
        assert pack(mf=strung, recs=rec5, sb_given=sb) == UNSUPPORTED
        assert pack(mf=req(leaf=leaf + [None], pl=short), out=at(out, 1)) == UNSUPPORTED, "a prefix under 4 bytes"
    overlap = req(leaf=bad_leaf + [None])
    past = req(leaf=[None, [8, 16], None, [8, 12], None])
    odd_leaf = req(leaf=[None, [8, 12], None, [6, 12], None])
    odd_stride = req(strides=[0, 16, 0, 18, 0])
    assert pack(mf=overlap, out=at(out, 1)) == INVALID and pack(mf=past, out=at(out, 1)) == INVALID  # before ALIGN
    misaligned = {
        "d_out (16)": dict(out=at(out, 8)), "an array (16)": dict(recs=[None, at(recs[1], 8), None, recs[3], None]),
        "a leaf's offset": dict(mf=odd_leaf), "a stride against its leaves": dict(mf=odd_stride),
        "a fixed column (16)": dict(cols=[[at(cols[0][0], 8)]] + cols[1:]),
        "a string's offsets array (8)": dict(so=so[:4] + [so[4][:3] + [at(so[4][3], 4)]]),
        "the index (8)": dict(index=at(d_index, 4)), "d_total (8)": dict(total=at(total, 4)),
        "the scratch (16)": dict(scratch=at(scratch, 8)), "d_offs (4)": dict(offs=at(offs, 2)),
    }
    for what, kw in misaligned.items():
        assert pack(**kw) == ALIGN, what  # with no scratch at all: ALIGN comes before CAPACITY
    assert pack(sb_given=plans("calc_echo").req.scratch_bytes(B.n) - 1) == CAPACITY and pack(sb_given=0) == CAPACITY

    # the decode, in the same way
    O = LegOuts(L, B)
    ss, so_ = [s for s, _ in L.slay], [o for _, o in L.slay]
    rsb = L.rep.scratch_bytes(B.n)
    ends, codes = empty(64), empty(B.n)

    def unpack(mf=L.rep, buf=out, cols=O.cols, so=O.offs, recs=O.recs, fill=L.fill, index=d_index, offs=offs, ends=ends,
               scratch=scratch, sb_given=0):
        return mf.unpack(buf, 100, offs, 3, d_method, index, B.n, TIMEOUT, cols, so, O.scap, recs, fill, None, O.cap,
                         codes, ends, None, scratch, sb_given)

    def rep(strides=ss, leaf=so_, pl=P.rep_plans):
        return MixedLegFrames(pl, strides, leaf)

    z = np.zeros(512, np.uint8)
    assert unpack(mf=rep([0, 16, 0, 16, 64], so_[:4] + [[0, 1, 8, 16]]), recs=O.recs[:4] + [out], fill=L.fill[:4] + [z],
                  buf=at(out, 1)) == UNSUPPORTED, "a string plan with a stride"
    for leaf in ([8], [300]):  # the second: also past the stride
        assert unpack(mf=rep([0, 16, 0, 264, 0], leaf=[None, [8], None, leaf, None]), fill=L.fill[:3] + [z, None],
                      buf=at(out, 1)) == UNSUPPORTED, "a decode stride above 256"
    short = [GpuPacker(srpc_amd.NUMBER, b"abcd")] + P.rep_plans[1:]
    assert unpack(mf=rep(pl=short), buf=at(out, 1)) == UNSUPPORTED, "a fixed reply plan with a prefix under 5 bytes"
    assert unpack(mf=rep(leaf=[None, [14], None, [8], None]), buf=at(out, 1)) == INVALID, "a leaf past the stride"
    two = [P.rep_plans[0], GpuPacker(srpc_amd.TWO_NUMBERS, srpc_amd.framed_response_prefix(srpc_amd.TWO_NUMBERS, 2))] + P.rep_plans[2:]
    assert unpack(mf=rep(pl=two, leaf=[None, [8, 10], None, [8], None]), buf=at(out, 1)) == INVALID, "overlapping leaves"
    misaligned = {
        "d_buf (16)": dict(buf=at(out, 8)), "an array (16)": dict(recs=[None, at(O.recs[1], 8), None, O.recs[3], None]),
        "a leaf's offset": dict(mf=rep(leaf=[None, [8], None, [6], None])),
        "a stride against its leaf": dict(mf=rep(strides=[0, 16, 0, 18, 0])),
        "a fixed column (16)": dict(cols=[[at(O.cols[0][0], 8)]] + O.cols[1:]),
        "a string column (16)": dict(cols=O.cols[:4] + [O.cols[4][:3] + [at(O.cols[4][3], 8)]]),
        "the index (8)": dict(index=at(d_index, 4)), "d_ends (8)": dict(ends=at(ends, 4)),
        "the scratch (16)": dict(scratch=at(scratch, 8)), "d_offs (4)": dict(offs=at(offs, 2)),
    }
    for what, kw in misaligned.items():
        assert unpack(**kw) == ALIGN, what
    assert unpack(sb_given=rsb - 1) == CAPACITY and unpack(sb_given=0) == CAPACITY
    torch.cuda.synchronize()
    # nothing was launched by a refused decode: the outputs are untouched
    assert (host(codes, B.n) == 0xA5).all() and (host(ends, 64) == 0xA5).all()
    assert all((host(O.recs[k], O.recs[k].numel()) == 0xA5).all() for k in L.recs)
    assert unpack(sb_given=rsb) == 0


def test_decode_captured_and_replayed_twice():
    """One decode captured on a single stream (a linear graph), replayed twice."""
    B = batch("calc_echo", 4097, "uniform", "mid")
    L = legs("calc_text", "tight", "mixed")
    n = B.n
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 3, n)
    parts = [struct.pack(">IB", 1, 3) if rng.random() < 0.2 else p for p in B.rep_frames(codes)]
    buf, offs = joined(parts)
    d_method, d_index, _ = build_index(B.method, L.K)
    d_buf, d_offs = dev(np.frombuffer(buf, np.uint8)), dev(offs[:-1].astype(np.uint32))
    O = LegOuts(L, B)
    d_codes, d_ends = empty(n + 16), empty(8 + 16)
    sb = L.rep.scratch_bytes(n)
    d_scratch = empty(sb + 16)
    st = status_buf()
    wc, full, wflags, wbad = model(buf, len(buf), offs[:-1], n, B, [0] * 5, O.cap)
    side_stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side_stream):
        assert L.rep.unpack(d_buf, len(buf), d_offs, n, d_method, d_index, n, TIMEOUT, O.cols, O.offs, O.scap, O.recs,
                            L.fill, None, O.cap, d_codes, d_ends, st, d_scratch, sb,
                            stream=torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()
    assert (host(d_codes, n) == 0xA5).all() and all((host(O.recs[k], 64) == 0xA5).all() for k in L.recs)  # capturing ran nothing
    for _ in range(2):
        d_codes.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(d_codes, n), wc) and read_status(st) == (wflags, wbad)
        check_legs(L, B, O, full, ends=host(d_ends, 8, np.uint64))
    assert (host(d_codes, n + 16)[n:] == 0xA5).all() and (host(d_scratch, sb + 16)[sb:] == 0xA5).all()
