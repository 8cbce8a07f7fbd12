"""A batch of request frames of several methods decoded in arrival order into
one device array of structs per method (srpc_frames_unpack_requests_mixed_aos,
include/srpc_gpu.h), and the ordered reply pack from struct arrays
(srpc_frames_pack_requests_mixed_aos over response plans with d_method =
d_class): the struct-array form of tests/test_gpu_requests_mixed.py, whose
servers (`Srv`: plans, the CPU oracle's frames, the columns they were packed
from, a foreign method's frames), `model`, `stream` and hostile edits are used
as they are.

Nothing expected comes from the kernel under test:
- classes are `model`'s, the header's rule on the host, checked against the
  class each frame was built to have; they are also compared with what
  srpc_frames_classify and the column call write for the same bytes, and the
  index with the column call's, byte for byte;
- ranks are numpy's (`cumcount`);
- expected struct arrays are numpy: 0xA5 everywhere, the fill record tiled over
  the elements of the classified frames below the cap, then each leaf's bytes
  from the columns the frames were packed from.
Layouts are tests/test_gpu_mixed_aos.layout's three and `tight`: packed leaves
from byte 0, the stride their extent rounded to the largest leaf (a Number is 4
bytes), so a tile's slice of an array can lie inside one 16-byte piece that it
shares with both neighbouring tiles' slices.
Every output starts as 0xA5 with 16 guard bytes behind it; arrays have
h_first[k] elements in front of the batch's and EXTRA behind, which must keep
0xA5.  The stream is staged as exactly buf_len bytes, so it ends where its
allocation ends."""
import functools
import struct

import numpy as np
import pytest

import srpc_amd
from srpc_amd import GpuPacker, MixedAosFrames, MixedFrames, Schema, _lib, framed_request_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402
from tests.test_gpu_mixed import BIG, EXTRA, NMAX, cumcount, dtypes, interleave  # noqa: E402
from tests.test_gpu_mixed_aos import layout, order, place  # noqa: E402
from tests.test_gpu_requests_mixed import (EDITS, PLAN_SETS, assemble, classify_cls, frame_list, model,  # noqa: E402
                                           srv, stream, used_methods)
from tests.test_gpu_requests_mixed import run as run_columns  # noqa: E402

UNKNOWN = _lib.SRPC_FRAME_UNKNOWN
BOUNDS = _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
GUARD = 16
LAYS = ["natural", "odd", "far", "tight"]
ORDERS = ["uniform", "runs", "round_robin", "skip_plan", "one_plan"]


def lay_of(schema, lay):
    """(stride, leaf offsets) of a struct a decode takes."""
    if lay != "tight":
        return layout(schema, lay, True)
    sizes = [np.dtype(dt).itemsize for dt in dtypes(schema)]
    offs, end = place(sizes, 0)
    m = max(sizes)
    return -(-end // m) * m, offs


def test_tight_layout():
    assert lay_of(srpc_amd.NUMBER, "tight") == (4, [0])
    assert lay_of(srpc_amd.TWO_NUMBERS, "tight") == (8, [0, 4])
    assert lay_of(BIG, "tight") == (256, list(range(0, 256, 8)))


class Lay:
    """One server's request structs (and its response structs) in one layout."""

    def __init__(self, name, lay):
        self.S = S = srv(name)
        rq = [lay_of(q, lay) for _, q, _ in S.methods]
        rs = [lay_of(r, lay) for _, _, r in S.methods]
        self.stride, self.offs = [x[0] for x in rq], [x[1] for x in rq]
        self.rstride, self.roffs = [x[0] for x in rs], [x[1] for x in rs]
        self.sizes = [[c.dtype.itemsize for c in cols] for cols in S.req_cols]
        self.rsizes = [[c.dtype.itemsize for c in cols] for cols in S.rep_cols]
        self.mf = MixedAosFrames(S.req_plans, self.stride, self.offs)
        self.rep = MixedAosFrames(S.rep_plans, self.rstride, self.roffs)
        rng = np.random.default_rng(len(name) + len(lay))
        self.fill = [rng.integers(0, 256, s, dtype=np.uint8) for s in self.stride]
        self.T = self.mf.tile


@functools.lru_cache(maxsize=None)
def lay_for(name, lay):
    return Lay(name, lay)


def test_tile_rule():
    for name in sorted(PLAN_SETS):
        for lay in LAYS:
            L = lay_for(name, lay)
            desc = sum(3 * (-(-s // 16) * 16) + 16 for s in L.stride)
            assert L.mf.scratch_bytes == desc
            t = 256
            while t > 16 and t * max(L.S.Fq) > 32768 - desc:
                t //= 2
            assert L.T == t  # the documented rule, with the request plans
    assert lay_for("big", "natural").T == 64 and lay_for("calc", "natural").T == 256


def run(L, buf, buf_len, offs, first, cap, alloc, status=True, recs=None, scratch=None):
    """One decode on 0xA5-filled outputs (or into `recs`) -> everything it wrote; guards checked
    (scratch: the caller's own, which may be larger, instead of a fresh one)."""
    S = L.S
    n, K = len(offs), S.K
    d_buf = dev(buf[:buf_len]) if buf_len else empty(16)  # the stream ends with its allocation
    d_offs = dev(offs.astype(np.uint32)) if n else empty(16)
    d_recs = recs or [empty(alloc[k] * L.stride[k] + GUARD) for k in range(K)]
    nb = MixedFrames.index_bytes(n, K)
    d_cls, d_index, d_counts = empty(n + GUARD), empty(nb + GUARD), empty(8 * (K + 1) + GUARD)
    sb = L.mf.scratch_bytes
    d_scratch = empty(sb + GUARD) if scratch is None else scratch
    behind = d_scratch[sb:].clone()
    st = status_buf()
    st[:] = 0x5A  # the call resets it
    rc = L.mf.unpack_requests(d_buf, buf_len, d_offs, n, d_recs, L.fill, first, cap, d_cls, d_index, nb, d_counts,
                              d_scratch, sb, st if status else None)
    assert rc == 0
    flags, bad = read_status(st) if status else (None, None)
    raw_cls = host(d_cls, n + GUARD)
    raw_index = host(d_index, nb + GUARD)
    raw_counts = host(d_counts, 8 * (K + 1) + GUARD)
    assert (raw_cls[n:] == 0xA5).all() and (raw_index[nb:] == 0xA5).all() and (raw_counts[-GUARD:] == 0xA5).all()
    assert torch.equal(d_scratch[sb:], behind)
    out = []
    for k in range(K):
        raw = host(d_recs[k], alloc[k] * L.stride[k] + GUARD)
        assert (raw[alloc[k] * L.stride[k]:] == 0xA5).all(), "wrote past an array"
        out.append(raw[:alloc[k] * L.stride[k]].reshape(alloc[k], L.stride[k]).copy())
    return dict(cls=raw_cls[:n].copy(), index=raw_index[:nb].copy(),
                counts=raw_counts[:8 * (K + 1)].view(np.uint64).copy(), recs=out, flags=flags, bad=bad, d_cls=d_cls,
                d_index=d_index, d_buf=d_buf, d_offs=d_offs, d_recs=d_recs)


def expected(L, want, elem, f0, cap, alloc, base=None):
    """Plan k's array of alloc[k] structs: 0xA5 (or `base`), then for every frame
    of class k with an element below cap[k] the fill with the frame's leaves.
    -> (arrays, the smallest frame without an element or NONE)."""
    S = L.S
    rank = cumcount(want)
    out, bad = [], NONE
    for k in range(S.K):
        exp = np.full((alloc[k], L.stride[k]), 0xA5, np.uint8) if base is None else base[k].copy()
        idx = np.flatnonzero(want == k)
        e = f0[k] + rank[idx]
        ok = e < cap[k]
        if not ok.all():
            bad = min(bad, int(idx[~ok][0]))
        exp[e[ok]] = L.fill[k]
        for c, off, s in zip(S.req_cols[k], L.offs[k], L.sizes[k]):
            vals = np.ascontiguousarray(c[elem[idx[ok]]])
            exp[e[ok], off:off + s] = vals.view(np.uint8).reshape(len(vals), s)
        out.append(exp)
    return out, bad


def same_structs(got, exp):
    for k, (g, e) in enumerate(zip(got, exp)):
        bad = np.flatnonzero((g != e).any(axis=1))
        assert bad.size == 0, f"plan {k} struct {bad[0]}: {g[bad[0]].tolist()} != {e[bad[0]].tolist()}"


def check(L, buf, buf_len, offs, intent, elem, first=None, cap=None, alloc=None, others=True, scratch=None):
    """Run the call and compare everything it wrote with the host's expectation,
    with srpc_frames_classify's classes and with the column call's classes,
    index, counts and status.  cap defaults to the elements the frames need,
    alloc to EXTRA more.  -> the run."""
    S = L.S
    n, K = len(offs), S.K
    want = model(S, buf, buf_len, offs)
    assert np.array_equal(want, intent), "the stream is not what the test meant to build"
    counts = [int((want == k).sum()) for k in range(K)]
    f0 = [0] * K if first is None else list(first)
    cap = [f0[k] + counts[k] for k in range(K)] if cap is None else list(cap)
    alloc = [max(cap[k], f0[k] + counts[k]) + EXTRA for k in range(K)] if alloc is None else list(alloc)
    got = run(L, buf, buf_len, offs, first, cap, alloc, scratch=scratch)
    exp, bad = expected(L, want, elem, f0, cap, alloc)
    print(f"{n} frames, buf_len {buf_len}: counts {got['counts'].tolist()} flags {got['flags']} first bad {got['bad']}")
    assert np.array_equal(got["cls"], want)
    assert got["counts"].tolist() == counts + [int((want == UNKNOWN).sum())]
    same_structs(got["recs"], exp)
    assert (got["flags"], got["bad"]) == ((BOUNDS, bad) if bad != NONE else (0, NONE))
    if others:
        assert np.array_equal(classify_cls(S, got["d_buf"], buf_len, got["d_offs"], n), want)
        col = run_columns(S, buf[:buf_len], buf_len, offs, first, cap, alloc)
        assert np.array_equal(col["cls"], got["cls"]) and np.array_equal(col["counts"], got["counts"])
        assert np.array_equal(host(col["d_index"], len(got["index"])), got["index"])  # byte-identical
        assert (col["flags"], col["bad"]) == (got["flags"], got["bad"])
    return got


def intent_of(name, which, n, T, foreign=0.0, seed=0):
    S = srv(name)
    used = np.arange(S.K) if used_methods(name) is None else np.asarray(used_methods(name))
    m = used[order(which, n, len(used), T)].astype(np.uint8)
    if foreign:
        m[np.random.default_rng(n + seed).random(n) < foreign] = UNKNOWN
    return m


def sizes(T, which):
    ns = sorted({0, 1, T - 1, T, T + 1, 255, 256, 257, 4095, 4096, 4097})  # 4096: the index's second-level row
    return ns + [NMAX] if which in ("uniform", "runs") else ns


@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_sizes_and_orders(name, lay, which):
    L = lay_for(name, lay)
    S = L.S
    for n in sizes(L.T, which):
        intent = intent_of(name, which, n, L.T)
        buf, offs, buf_len, elem = stream(S, intent)
        first = [3 * k + 1 for k in range(S.K)]  # the arrays' elements in front of the batch's keep 0xA5
        got = check(L, buf, buf_len, offs, intent, elem, first=first, others=n <= 4097 or lay == "tight")
        if name == "twice":
            assert got["counts"][2] == 0


@pytest.mark.parametrize("share", [0.1, 0.9])
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds", "big", "twice"])
def test_foreign_frames(name, lay, share):
    """Frames of a method nobody registered, as long as method 0's."""
    L = lay_for(name, lay)
    for n in (L.T + 1, 4097):
        intent = intent_of(name, "uniform", n, L.T, foreign=share, seed=1)
        buf, offs, buf_len, elem = stream(L.S, intent)
        check(L, buf, buf_len, offs, intent, elem)


# ---- hostile frames among good neighbours -----------------------------------------------------

BAD_EDITS = ["three_bytes", "last_prefix_byte", "one_longer", "one_shorter"]


def spots(T, n):
    return [0, T - 1, T, n - 1]


@pytest.mark.parametrize("what", BAD_EDITS)
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "big"])
def test_bad_frame(name, lay, what):
    """A frame under 4 bytes, one wrong prefix byte, a length off by one in either
    direction, at index 0, T - 1, T and last: no struct for any of them, every
    frame around them still decodes."""
    L = lay_for(name, lay)
    S = L.S
    n = 2 * L.T + 5
    intent, elem, frames = frame_list(S, n, seed=len(what))
    for p in spots(L.T, n):
        frames[p] = EDITS[what](S, int(intent[p]), frames[p])
        intent[p] = UNKNOWN
    buf, offs, buf_len = assemble(frames)
    check(L, buf, buf_len, offs, intent, elem)


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "big"])
def test_cut_last_frame_and_ends_past_buf_len(name, lay):
    L = lay_for(name, lay)
    S = L.S
    n = 2 * L.T + 5
    intent, elem, frames = frame_list(S, n, seed=9)
    buf, offs, total = assemble(frames)
    # the last frame cut by one byte
    cut = intent.copy()
    cut[-1] = UNKNOWN
    check(L, buf, total - 1, offs, cut, elem)
    # the last frame starts past buf_len: the one before it now ends past buf_len too
    far = offs.copy()
    far[-1] = total + 8
    cut = intent.copy()
    cut[-2:] = UNKNOWN
    check(L, buf, total, far, cut, elem)
    # buf_len inside frame T: it and every later frame are nobody's
    cut = intent.copy()
    cut[L.T:] = UNKNOWN
    check(L, buf, int(offs[L.T]) + S.Fq[int(intent[L.T])] - 2, offs, cut, elem)
    # an end far past buf_len in the first frame's place: frame 0 is nobody's
    far = offs.copy()
    far[1] = 0xFFFFFFF0
    cut = intent.copy()
    cut[:2] = UNKNOWN
    check(L, buf, total, far, cut, elem)


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "big"])
def test_offsets_out_of_order(name, lay):
    L = lay_for(name, lay)
    T = L.T
    n = 2 * T + 5
    intent, elem, frames = frame_list(L.S, n, seed=7)
    buf, offs, buf_len = assemble(frames)
    for p in (1, T - 1, T + 2, n - 3):  # at the stream's start, across a tile edge, behind it, near the end
        # frame p - 1 now spans three frames, frame p runs backwards, frame p + 1 is whole
        offs[p] = offs[p + 2]
        intent[p - 1] = intent[p] = UNKNOWN
    check(L, buf, buf_len, offs, intent, elem)


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds", "big"])
def test_oversize_junk_mid_tile(name, lay):
    """A junk frame larger than the image in the middle of a tile pushes the
    frames of that tile behind it out of the image: they are read from global
    memory and still decoded."""
    L = lay_for(name, lay)
    S = L.S
    T = L.T
    n = 3 * T + 5
    at = T + T // 2
    intent, elem, frames = frame_list(S, n, seed=40)
    rng = np.random.default_rng(T)
    junk = T * max(S.Fq) + 4096  # more than the T * F_max + 16 bytes a tile stages
    frames[at] = rng.integers(0, 256, junk, dtype=np.uint8)
    frames[at][:4] = np.frombuffer(struct.pack(">I", junk - 4), np.uint8)  # a well-formed frame of nobody's
    intent[at] = UNKNOWN
    buf, offs, buf_len = assemble(frames)
    got = check(L, buf, buf_len, offs, intent, elem)
    assert int(got["counts"][S.K]) == 1


# ---- h_first / h_cap --------------------------------------------------------------------------

@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds", "big"])
def test_short_array(name, lay):
    """h_first non-zero and h_cap short by one and by half: BOUNDS with the
    smallest frame that has no element, the structs below the cap written, the
    allocated ones at or past it untouched."""
    L = lay_for(name, lay)
    S = L.S
    n = 3 * L.T + 5
    intent = intent_of(name, "uniform", n, L.T, foreign=0.05, seed=3)
    buf, offs, buf_len, elem = stream(S, intent)
    counts = [int((intent == k).sum()) for k in range(S.K)]
    first = [5 + 11 * k for k in range(S.K)]
    alloc = [first[k] + counts[k] + EXTRA for k in range(S.K)]
    k = S.K - 1
    for short in (1, counts[k] // 2):
        cap = [first[q] + counts[q] for q in range(S.K)]
        cap[k] -= short
        got = check(L, buf, buf_len, offs, intent, elem, first=first, cap=cap, alloc=alloc)
        assert got["bad"] == int(np.flatnonzero(intent == k)[counts[k] - short]) and got["cls"][got["bad"]] == k
    # every plan short at once, first zero
    cap = [c - c // 2 for c in counts]
    got = check(L, buf, buf_len, offs, intent, elem, cap=cap, alloc=alloc)
    assert got["flags"] == BOUNDS


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_two_chunks(name, lay):
    """A second chunk with h_first = the first chunk's counts into the same arrays equals one call."""
    L = lay_for(name, lay)
    S = L.S
    T = L.T
    n = 3 * T + 5
    intent = intent_of(name, "uniform", n, T, foreign=0.05, seed=2)
    buf, offs, buf_len, elem = stream(S, intent)
    counts = [int((intent == k).sum()) for k in range(S.K)]
    alloc = [c + EXTRA for c in counts]
    whole, _ = expected(L, intent, elem, [0] * S.K, counts, alloc)
    o = np.append(offs.astype(np.int64), buf_len)
    for a in (1, T, n - 1):
        c1 = [int((intent[:a] == k).sum()) for k in range(S.K)]
        g1 = run(L, buf[:o[a]], int(o[a]), offs[:a], None, counts, alloc)
        part, _ = expected(L, intent[:a], elem[:a], [0] * S.K, counts, alloc)
        same_structs(g1["recs"], part)  # the rest still 0xA5
        assert g1["counts"].tolist()[:S.K] == c1
        g2 = run(L, buf[o[a]:], buf_len - int(o[a]), (o[a:n] - o[a]).astype(np.uint32), c1, counts, alloc,
                 recs=g1["d_recs"])
        same_structs(g2["recs"], whole)
        assert (g1["flags"], g2["flags"]) == (0, 0)
        assert np.array_equal(np.concatenate([g1["cls"], g2["cls"]]), intent)


def test_null_status():
    L = lay_for("calc", "natural")
    intent = intent_of("calc", "uniform", 300, L.T, foreign=0.1, seed=4)
    buf, offs, buf_len, elem = stream(L.S, intent)
    counts = [int((intent == k).sum()) for k in range(L.S.K)]
    got = run(L, buf, buf_len, offs, None, counts, counts, status=False)
    assert np.array_equal(got["cls"], intent)
    same_structs(got["recs"], expected(L, intent, elem, [0] * L.S.K, counts, counts)[0])


# ---- the reply side: srpc_frames_pack_requests_mixed_aos over response plans ------------------

def resp_structs(L, k, nelem):
    """Elements [0, nelem) of plan k's response columns as structs, random bytes around the leaves."""
    a = np.random.default_rng(k + nelem).integers(0, 256, (max(nelem, 1), L.rstride[k]), dtype=np.uint8)
    for col, off, s in zip(L.S.rep_cols[k], L.roffs[k], L.rsizes[k]):
        a[:nelem, off:off + s] = np.ascontiguousarray(col[:nelem]).view(np.uint8).reshape(nelem, s)
    return a


@pytest.mark.parametrize("foreign", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds", "big", "sixteen"])
def test_round_trip_on_the_device(name, lay, foreign):
    """Decode, then the reply pack with d_method = d_class and the decode's
    index from Resp arrays built in numpy: the oracle's reply stream in arrival
    order, zero bytes at unknown frames, nothing at or past the total."""
    L = lay_for(name, lay)
    S = L.S
    for n in (1, L.T + 1, 4097):
        intent = intent_of(name, "uniform", n, L.T, foreign=foreign, seed=5)
        if foreign >= 1.0:
            intent[:] = UNKNOWN
        buf, offs, buf_len, elem = stream(S, intent)
        got = check(L, buf, buf_len, offs, intent, elem, others=False)
        counts = [int((intent == k).sum()) for k in range(S.K)]
        d_resp = [dev(resp_structs(L, k, counts[k])) for k in range(S.K)]
        out_cap = n * max(S.Fr)
        d_out, d_offs = empty(out_cap + GUARD), empty(4 * (n + 1) + GUARD)
        st = status_buf()
        st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
        rc = L.rep.pack(d_resp, None, counts, got["d_cls"], got["d_index"], n, d_out, out_cap, d_offs, st)
        assert rc == 0
        good = intent != UNKNOWN
        want, woffs = interleave(S.rep_rows, intent, cumcount(intent), good)  # response r of method k: its r-th request's
        roffs = host(d_offs, 4 * (n + 1), np.uint32)
        assert (host(d_offs, 4 * (n + 1) + GUARD)[-GUARD:] == 0xA5).all()
        assert np.array_equal(roffs, woffs.astype(np.uint32))
        assert (roffs[1:][~good] == roffs[:-1][~good]).all()
        raw = host(d_out, out_cap + GUARD)
        total = int(woffs[n])
        assert np.array_equal(raw[:total], want) and (raw[total:] == 0xA5).all()
        flags, bad = read_status(st)  # the pack's own flag: "unknown frames present", the first of them
        assert (flags, bad) == ((BOUNDS, int(np.flatnonzero(~good)[0])) if (~good).any() else (0, NONE))


# ---- refusals that need real plans -------------------------------------------------------------

def test_refusals_with_real_plans():
    UNS, INV, ALIGN, CAP = (_lib.SRPC_E_UNSUPPORTED, _lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_CAPACITY)
    L = lay_for("kinds", "natural")
    S = L.S
    n = 64
    nb = MixedFrames.index_bytes(n, S.K)
    sb = L.mf.scratch_bytes
    d_buf, d_offs = empty(64 * n), dev(np.zeros(n, np.uint32))
    d_cls, d_idx, d_cnt, d_scratch = empty(n + 16), empty(nb + 16), empty(8 * (S.K + 1) + 16), empty(sb + 16)
    d_recs = [empty(n * s + 16) for s in L.stride]

    def call(mf=L.mf, recs=d_recs, buf=d_buf, offs=d_offs, idx=d_idx, nb=nb, cnt=d_cnt, scratch=d_scratch, sb=sb,
             fills=L.fill):
        return mf.unpack_requests(buf, 64 * n, offs, n, recs, fills, None, [n] * mf.k, d_cls, idx, nb, cnt, scratch, sb)

    def with_layout(k, stride=None, offs=None):
        strides, loffs = list(L.stride), [list(o) for o in L.offs]
        if stride is not None:
            strides[k] = stride
        if offs is not None:
            loffs[k] = offs
        return MixedAosFrames(S.req_plans, strides, loffs)

    # 2. a string plan, a short prefix, 193 leaves, a stride above 256 -- each ahead of alignment and capacity
    string = MixedAosFrames([GpuPacker(Schema("S", (("s", srpc_amd.STRING),)), b"\0\0\0\x08abcd")], [16], [[8]])
    short = MixedAosFrames([GpuPacker(srpc_amd.NUMBER, b"abc")], [16], [[8]])
    bigs = [GpuPacker(BIG, framed_request_prefix(BIG, f"B_servicer::m{j}")) for j in range(6)]
    many = MixedAosFrames(bigs + [GpuPacker(srpc_amd.NUMBER, framed_request_prefix(srpc_amd.NUMBER, "B_servicer::n"))],
                          [256] * 6 + [4], [list(range(0, 256, 8))] * 6 + [[0]])
    fits = MixedAosFrames(bigs, [256] * 6, [list(range(0, 256, 8))] * 6)  # 192 leaves are taken
    for mf in (string, short):
        assert call(mf=mf, recs=[d_recs[0]], fills=[bytes(16)], buf=d_buf.data_ptr() + 8, nb=0) == UNS
    assert call(mf=many, recs=[d_recs[0]] * 7, fills=[bytes(256)] * 6 + [bytes(4)], buf=d_buf.data_ptr() + 8, nb=0) == UNS
    assert call(mf=with_layout(1, stride=257), nb=0) == UNS
    assert call(mf=with_layout(1, stride=264), nb=0) == UNS
    assert call(mf=with_layout(1, stride=264, offs=[300] * 8), nb=0) == UNS  # before its leaves are looked at
    # 3. overlapping leaves, a leaf past the stride (before any alignment)
    o = L.offs[0]  # all_kinds: bool, int8, char, int16, int32, int64 at 8, 9, 10, 12, 16, 24
    assert o == [8, 9, 10, 12, 16, 24] and L.stride[0] == 32
    assert call(mf=with_layout(0, offs=[8, 9, 10, 12, 16, 16]), nb=0) == INV   # int64 over the int32
    assert call(mf=with_layout(0, offs=[8, 8, 10, 12, 16, 24]), nb=0) == INV
    assert call(mf=with_layout(0, offs=[8, 9, 10, 9, 16, 24]), nb=0) == INV    # misaligned too: INVALID first
    assert call(mf=with_layout(0, offs=[8, 9, 10, 12, 16, 28]), nb=0) == INV   # past the stride
    # 4. alignment: an offset, the stride, an array, the buffers -- ahead of capacity
    assert call(mf=with_layout(0, offs=[8, 9, 10, 13, 16, 24]), nb=0) == ALIGN
    assert call(mf=with_layout(0, stride=36), nb=0) == ALIGN                    # the int64 against the stride
    recs = list(d_recs)
    recs[1] = recs[1].data_ptr() + 8
    assert call(recs=recs, nb=0) == ALIGN
    assert call(buf=d_buf.data_ptr() + 8, nb=0) == ALIGN
    assert call(offs=d_offs.data_ptr() + 2, nb=0) == ALIGN
    assert call(idx=d_idx.data_ptr() + 4, nb=0) == ALIGN
    assert call(cnt=d_cnt.data_ptr() + 4, nb=0) == ALIGN
    assert call(scratch=d_scratch.data_ptr() + 8, nb=0) == ALIGN
    # 5. capacity
    assert call(nb=nb - 1) == CAP
    assert call(sb=sb - 1) == CAP
    torch.cuda.synchronize()
    for t in [d_cls, d_idx, d_cnt, d_scratch] + d_recs:
        assert (t.cpu().numpy() == 0xA5).all()  # refused: nothing launched
    assert call() == 0
    nb6 = MixedFrames.index_bytes(n, 6)
    assert call(mf=fits, recs=[empty(n * 256 + 16) for _ in range(6)], fills=[bytes(256)] * 6, idx=empty(nb6), nb=nb6,
                cnt=empty(8 * 7), sb=fits.scratch_bytes, scratch=empty(fits.scratch_bytes)) == 0
    torch.cuda.synchronize()


def test_captured_and_replayed_twice():
    """One decode captured on a single stream (a linear graph) and replayed twice onto re-poisoned arrays."""
    L = lay_for("calc", "odd")
    S = L.S
    n = 4097
    intent = intent_of("calc", "uniform", n, L.T, foreign=0.1, seed=6)
    buf, offs, buf_len, elem = stream(S, intent)
    counts = [int((intent == k).sum()) for k in range(S.K)]
    cap = list(counts)
    cap[1] -= 3  # BOUNDS as well
    exp, bad = expected(L, intent, elem, [0] * S.K, cap, counts)
    exp0 = [np.zeros_like(e) for e in exp]
    nb = MixedFrames.index_bytes(n, S.K)
    sb = L.mf.scratch_bytes
    d_buf, d_offs = dev(buf), dev(offs)
    z = lambda b: torch.zeros(b, dtype=torch.uint8, device="cuda")
    d_recs = [z(c * s + 16) for c, s in zip(counts, L.stride)]
    d_cls, d_index, d_counts, d_scratch = z(n + 16), z(nb), z(8 * (S.K + 1)), z(sb)
    st = status_buf()
    side_stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side_stream):
        assert L.mf.unpack_requests(d_buf, buf_len, d_offs, n, d_recs, L.fill, None, cap, d_cls, d_index, nb, d_counts,
                                    d_scratch, sb, st, stream=torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()
    assert not d_cls.any() and not any(t.any() for t in d_recs) and not d_scratch.any()  # capturing ran nothing
    for _ in range(2):
        for t in d_recs + [d_cls, d_index, d_counts, d_scratch]:
            t.fill_(0xA5)
        st[:] = 0x5A
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(d_cls, n), intent) and read_status(st) == (BOUNDS, bad)
        assert host(d_counts, 8 * (S.K + 1), np.uint64).tolist() == counts + [int((intent == UNKNOWN).sum())]
        base = [np.full_like(e, 0xA5) for e in exp0]
        want, _ = expected(L, intent, elem, [0] * S.K, cap, counts, base=base)
        same_structs([host(t, c * s).reshape(c, s) for t, c, s in zip(d_recs, counts, L.stride)], want)
        assert (host(d_cls, n + 16)[n:] == 0xA5).all()
        assert all((host(t, c * s + 16)[c * s:] == 0xA5).all() for t, c, s in zip(d_recs, counts, L.stride))
