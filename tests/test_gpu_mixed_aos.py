"""Batches of calls of several methods in call order, every plan's calls held
as one device array of structs (srpc_frames_pack_requests_mixed_aos /
_unpack_replies_mixed_aos, include/srpc_gpu.h): the struct-array form of
tests/test_gpu_mixed.py, whose reference (`Ref`: plans, inputs, the CPU oracle's
frames), `cumcount`, `interleave`, `model` and method orders are used as they
are.

Nothing expected comes from the kernels under test:
- expected request bytes are the oracle's frames interleaved by the method
  vector; expected codes, flags and first bad index are `model`'s;
- expected struct arrays are numpy: 0xA5 everywhere, the fill record tiled over
  the elements of the chunk's good calls, then each leaf's bytes from the
  column values (zero where `model` says zero fields);
- both are also compared with what the column calls return on the same input.
Every output starts as 0xA5 with 16 guard bytes behind it; arrays have
h_first[k] elements in front of the chunk's and EXTRA behind, which must keep
0xA5.  Fill records and the non-leaf bytes of request structs are random."""
import functools
import struct

import numpy as np
import pytest

import srpc_amd
from srpc_amd import GpuPacker, MixedAosFrames, Schema, _lib, framed_response_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402
from tests.test_gpu_replies import BAD  # noqa: E402
from tests.test_gpu_mixed import (EXTRA, NMAX, SETS, TIMEOUT, Ref, build_index, cumcount, dtypes,  # noqa: E402
                                  interleave, model, pattern, ref, reply_stream, run_pack, run_unpack)

assert Ref and SETS  # the shared reference: ref(name) is a cached Ref over SETS[name]
PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
NAMES = ["calc", "kinds", "big", "sixteen"]
LAYS = ["natural", "odd", "far"]
ORDERS = ["uniform", "runs", "round_robin", "skip_plan", "one_plan"]
FAR_PACK = 520  # a request struct larger than any decode takes


def place(sizes, start):
    """Leaves in this order from byte `start`, each naturally aligned -> (offsets, end)."""
    offs, at = [], start
    for s in sizes:
        at = -(-at // s) * s
        offs.append(at)
        at += s
    return offs, at


def layout(schema, lay, decode):
    """(stride, leaf offsets) -- as tests/test_gpu_replies_aos.py's three:
    natural: the C++ layout behind an 8-byte vtable slot;
    odd:     a stride that is no multiple of 16, the leaves out of wire order
             (last leaf first, behind a gap of the largest leaf's size);
    far:     the leaves at the far end of 256 bytes (decode) or of FAR_PACK bytes
             (pack: above what a decode takes).
    A reply whose leaves alone fill 256 bytes (Big) has no room for the slot,
    the gap or the odd stride in a decode: it then starts at byte 0."""
    sizes = [np.dtype(dt).itemsize for dt in dtypes(schema)]
    m = max(sizes)
    up = lambda x, a: -(-x // a) * a
    if lay == "natural":
        offs, end = place(sizes, 8)
        stride = up(end, 8)
        if decode and stride > 256:
            offs, end = place(sizes, 0)
            stride = up(end, m)
    elif lay == "odd":
        offs, end = place(sizes[::-1], m)
        stride = up(end, m)
        if stride % 16 == 0:
            stride += m
        if decode and stride > 256:
            offs, end = place(sizes[::-1], 0)
            stride = up(end, m)
        offs = offs[::-1]
    else:
        stride = 256 if decode else FAR_PACK
        offs, end = place(sizes, 0)
        base = (stride - end) // m * m
        offs = [base + o for o in offs]
    assert stride <= 256 or not decode
    assert all(o % s == 0 and stride % s == 0 and o + s <= stride for o, s in zip(offs, sizes))
    return stride, offs


class Side:
    """One set's request or reply structs in one layout."""

    def __init__(self, name, lay, decode):
        self.R = ref(name)
        schemas = [(rs if decode else rq) for _, rq, rs in self.R.methods]
        self.sizes = [[np.dtype(dt).itemsize for dt in dtypes(s)] for s in schemas]
        lays = [layout(s, lay, decode) for s in schemas]
        self.stride = [l[0] for l in lays]
        self.offs = [l[1] for l in lays]
        self.mf = MixedAosFrames(self.R.rep_plans if decode else self.R.req_plans, self.stride, self.offs)
        rng = np.random.default_rng(len(name) + len(lay))
        self.fill = [rng.integers(0, 256, s, dtype=np.uint8) for s in self.stride]
        self.cols = self.R.rep_cols if decode else self.R.req_cols


@functools.lru_cache(maxsize=None)
def side(name, lay, decode):
    return Side(name, lay, decode)


def test_layouts_are_the_three():
    assert layout(srpc_amd.NUMBER, "natural", True) == (16, [8])
    assert layout(srpc_amd.TWO_NUMBERS, "natural", False) == (16, [8, 12])
    assert layout(srpc_amd.NUMBER, "far", True) == (256, [252])
    for name in NAMES:
        for dec in (False, True):
            S = side(name, "odd", dec)
            assert any(s % 16 for s in S.stride)
            assert any(o != sorted(o) for o in S.offs) or all(len(o) == 1 for o in S.offs)
    assert side("kinds", "far", False).stride == [FAR_PACK] * 3


def order(which, n, K, T):
    if which == "skip_plan":  # a plan with no call
        m = pattern("uniform", n, max(K - 1, 1), T) + (1 if K > 1 else 0)
        return m.astype(np.uint8)
    return pattern(which, n, K, T)


def sizes(T, which):
    ns = sorted({0, 1, T - 1, T, T + 1, 255, 256, 257, 4097})
    return ns + [NMAX] if which in ("uniform", "runs") else ns


# ---- pack ---------------------------------------------------------------------------------------

def req_structs(S, k, nelem):
    """Elements [0, nelem) of plan k's request columns as structs, random bytes around the leaves."""
    a = np.random.default_rng(k + nelem).integers(0, 256, (nelem, S.stride[k]), dtype=np.uint8)
    for col, off, s in zip(S.cols[k], S.offs[k], S.sizes[k]):
        a[:, off:off + s] = np.ascontiguousarray(col[:nelem]).view(np.uint8).reshape(nelem, s)
    return a


def run_pack_aos(S, method, first=None, cap=None, index=None, short=0):
    """As test_gpu_mixed.run_pack; the arrays hold exactly cap[k] structs."""
    R = S.R
    n = len(method)
    d_method, d_index = index or build_index(method, R.K)[:2]
    first = first or [0] * R.K
    cap = cap or [min(NMAX, int(first[k] + np.sum(method == k))) for k in range(R.K)]
    d_recs = [dev(req_structs(S, k, cap[k])) if cap[k] else empty(16) for k in range(R.K)]
    out_cap = n * max(R.Fq) - short
    d_out = empty(out_cap + 16)
    d_offs = empty(4 * (n + 1) + 16)
    st = status_buf()
    st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
    rc = S.mf.pack(d_recs, first, cap, d_method, d_index, n, d_out, out_cap, d_offs, st)
    flags, bad = read_status(st)
    if rc:
        assert (host(d_out, out_cap + 16) == 0xA5).all() and (host(d_offs, 4 * (n + 1) + 16) == 0xA5).all()
        return rc, None, None, flags, bad
    offs = host(d_offs, 4 * (n + 1), np.uint32)
    assert (host(d_offs, 4 * (n + 1) + 16)[-16:] == 0xA5).all()
    total = int(offs[n])
    raw = host(d_out, out_cap + 16)
    assert (raw[total:] == 0xA5).all(), "wrote at or past the total"
    return rc, raw[:total], offs, flags, bad


@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", NAMES)
def test_pack(name, lay, which):
    S = side(name, lay, False)
    R = S.R
    T = R.req.tile
    for n in sizes(T, which):
        method = order(which, n, R.K, T)
        index = build_index(method, R.K)[:2]
        rc, raw, offs, flags, _ = run_pack_aos(S, method, index=index)
        want, woffs = interleave(R.req_rows, method, cumcount(method), np.ones(n, bool))
        print(f"{name}/{lay}/{which} n={n} rc={rc} flags={flags} bytes={len(want)}")
        assert rc == 0 and flags == 0
        assert np.array_equal(offs, woffs.astype(np.uint32)), n
        assert np.array_equal(raw, want), n
        if n in (T + 1, 4097):  # and the column call's on the same values
            crc, craw, coffs, cflags, _ = run_pack(R, method, index=index)
            assert crc == 0 and np.array_equal(craw, raw) and np.array_equal(coffs, offs) and cflags == flags


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_pack_in_two_chunks(name, lay):
    S = side(name, lay, False)
    R = S.R
    T = R.req.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    whole = run_pack_aos(S, method)[1]
    for a in (1, T, n - 1):
        counts = build_index(method[:a], R.K)[2]
        head = run_pack_aos(S, method[:a])[1]
        rc, tail, _, flags, _ = run_pack_aos(S, method[a:], first=[int(c) for c in counts[:R.K]])
        assert rc == 0 and flags == 0
        assert np.array_equal(np.concatenate([head, tail]), whole), a


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_pack_bad_calls(name, lay):
    """Ids >= K and a leg one element short: no frame for the BAD call, BOUNDS, the smallest index."""
    S = side(name, lay, False)
    R = S.R
    T = R.req.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    method[[T + 7, n - 1]] = [R.K, 200]
    rank = cumcount(method)
    k = 1
    cap = [int(np.sum(method == q)) for q in range(R.K)]
    cap[k] -= 1
    good = (method < R.K) & ~((method == k) & (rank >= cap[k]))
    p = int(np.flatnonzero(~good)[0])
    assert (~good).sum() == 3
    index = build_index(method, R.K)[:2]
    rc, raw, offs, flags, first = run_pack_aos(S, method, cap=cap, index=index)
    want, woffs = interleave(R.req_rows, method, rank, good)
    assert rc == 0 and (flags, first) == (BOUNDS, p)
    assert np.array_equal(offs, woffs.astype(np.uint32)) and np.array_equal(raw, want)
    assert all(offs[i + 1] == offs[i] for i in np.flatnonzero(~good))
    crc, craw, coffs, cflags, cfirst = run_pack(R, method, cap=cap, index=index)
    assert (crc, cflags, cfirst) == (rc, flags, first) and np.array_equal(craw, raw) and np.array_equal(coffs, offs)


def test_pack_out_cap_one_byte_short():
    S = side("calc", "natural", False)
    method = pattern("uniform", 300, 4, 256)
    assert run_pack_aos(S, method, short=1)[0] == _lib.SRPC_E_CAPACITY
    assert run_pack_aos(S, method, short=0)[0] == 0


# ---- decode -------------------------------------------------------------------------------------

def run_unpack_aos(S, method, buf, buf_len, offs, nframes, first=None, cap=None, index=None, recs=None,
                   scratch_bytes=None, stream=None, scratch=None):
    """One decode on 0xA5-filled outputs (or into `recs`) -> (rc, codes, recs[k] as
    (cap[k], stride) bytes, flags, first bad, the device arrays); guards checked
    (scratch: the caller's own, which may be larger, instead of a fresh one)."""
    R = S.R
    n = len(method)
    d_method, d_index = index or build_index(method, R.K)[:2]
    first = first or [0] * R.K
    cap = cap or [int(first[k] + np.sum(method == k)) + EXTRA for k in range(R.K)]
    d_buf = dev(np.frombuffer(buf, np.uint8)) if buf else empty(16)
    d_offs = dev(offs) if nframes else empty(16)
    d_recs = recs or [empty(cap[k] * S.stride[k] + 16) for k in range(R.K)]
    d_codes = empty(n + 16)
    sb = S.mf.scratch_bytes
    d_scratch = empty(sb + 16) if scratch is None else scratch
    behind = d_scratch[sb:].clone()
    st = status_buf()
    rc = S.mf.unpack(d_buf, buf_len, d_offs, nframes, d_method, d_index, n, TIMEOUT, d_recs, S.fill, first, cap,
                     d_codes, d_scratch, sb if scratch_bytes is None else scratch_bytes, st, stream=stream)
    flags, bad = read_status(st)
    out = []
    for k in range(R.K):
        raw = host(d_recs[k], cap[k] * S.stride[k] + 16)
        assert (raw[cap[k] * S.stride[k]:] == 0xA5).all(), "wrote past an array"
        out.append(raw[:cap[k] * S.stride[k]].reshape(cap[k], S.stride[k]))
    assert (host(d_codes, n + 16)[n:] == 0xA5).all() and torch.equal(d_scratch[sb:], behind)
    return rc, host(d_codes, n), out, flags, bad, d_recs


def expected_structs(S, method, zero, ncap, first=None, base=None):
    """Plan k's array of ncap[k] structs: 0xA5 (or `base`), then for every good
    call (k, r) element first[k] + r = the fill with the call's leaves, zero
    where `zero` says so for that call."""
    R = S.R
    first = first or [0] * R.K
    rank = cumcount(method)
    out = []
    for k in range(R.K):
        exp = np.full((ncap[k], S.stride[k]), 0xA5, np.uint8) if base is None else base[k].copy()
        calls = np.flatnonzero(method == k)
        el = first[k] + rank[calls]
        keep = el < ncap[k]
        calls, el = calls[keep], el[keep]
        exp[el] = S.fill[k]
        for x, off, s in zip(S.cols[k], S.offs[k], S.sizes[k]):
            vals = np.ascontiguousarray(np.where(zero[calls], 0, x[np.minimum(el, NMAX - 1)]).astype(x.dtype))
            exp[el, off:off + s] = vals.view(np.uint8).reshape(len(el), s)
        out.append(exp)
    return out


def same_structs(got, exp):
    for k, (g, e) in enumerate(zip(got, exp)):
        bad = np.flatnonzero((g != e).any(axis=1))
        assert bad.size == 0, f"plan {k} struct {bad[0]}: {g[bad[0]].tolist()} != {e[bad[0]].tolist()}"


def check(S, method, buf, buf_len, offs, nframes, first=None, cap=None, columns=True, scratch=None):
    """The AoS decode against `model` and numpy, and against the column call on the same bytes."""
    R = S.R
    n = len(method)
    first = first or [0] * R.K
    index = build_index(method, R.K)[:2]
    rc, codes, recs, flags, bad, _ = run_unpack_aos(S, method, buf, buf_len, offs, nframes, first, cap, index,
                                                    scratch=scratch)
    ncap = [len(r) for r in recs]
    want, full, wflags, wbad = model(buf, buf_len, offs, nframes, method, first, ncap, R)
    print(f"{R.name} n={n} nframes={nframes} rc={rc} flags={flags} first={bad} want flags={wflags} first={wbad}")
    assert rc == 0
    assert np.array_equal(codes[:nframes], want) and (codes[nframes:] == TIMEOUT).all()
    assert (flags, bad) == (wflags, wbad)
    zero = np.ones(n, bool)
    zero[:nframes] = ~full
    same_structs(recs, expected_structs(S, method, zero, ncap, first))
    if columns:
        crc, ccodes, _, cflags, cbad = run_unpack(R, method, buf, buf_len, offs, nframes, first=first, cap=ncap,
                                                  index=index)
        assert (crc, cflags, cbad) == (rc, flags, bad) and np.array_equal(ccodes, codes)
    return want, full, wflags, wbad


def test_tile_rule():
    for name in NAMES:
        for lay in LAYS:
            S = side(name, lay, True)
            desc = sum(3 * (-(-s // 16) * 16) + 16 for s in S.stride)
            assert S.mf.scratch_bytes == desc
            t = 256
            while t > 16 and t * max(S.R.Fr) > 32768 - desc:
                t //= 2
            assert S.mf.tile == t  # the documented rule
    assert side("big", "natural", True).mf.tile < 256 and side("calc", "natural", True).mf.tile == 256


@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", NAMES)
def test_decode_all_full(name, lay, which):
    S = side(name, lay, True)
    R = S.R
    T = S.mf.tile
    for n in sizes(T, which):
        method = order(which, n, R.K, T)
        codes = np.random.default_rng(n).integers(0, 3, n)
        first = [3 * k + 1 for k in range(R.K)]  # the arrays' elements in front of the chunk's keep 0xA5
        elem = np.minimum(np.array(first)[method] + cumcount(method), NMAX - 1) if n else cumcount(method)
        buf, offs = reply_stream(R, method, elem, codes)
        want, full, flags, _ = check(S, method, buf, len(buf), offs, n, first=first, columns=n in (T + 1, 4097))
        assert full.all() and flags == 0 and np.array_equal(want, codes)


@pytest.mark.parametrize("share", [0.1, 0.9])
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_bare_frames(name, lay, share):
    S = side(name, lay, True)
    R = S.R
    n = 4097
    method = pattern("uniform", n, R.K, S.mf.tile)
    rng = np.random.default_rng(int(100 * share))
    codes = rng.integers(0, 3, n)
    bare = rng.random(n) < share
    special = {int(i): struct.pack(">IB", 1, int(rng.integers(1, 256))) for i in np.flatnonzero(bare)}
    buf, offs = reply_stream(R, method, cumcount(method), codes, special)
    _, full, flags, _ = check(S, method, buf, len(buf), offs, n)
    assert np.array_equal(full, ~bare) and flags == 0


@pytest.mark.parametrize("case", BAD)
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_one_bad_frame(name, lay, case):
    """One bad frame at index 0, T - 1, T and last among full frames of mixed
    codes and a few bare ones: every full frame around it must still decode."""
    S = side(name, lay, True)
    R = S.R
    T = S.mf.tile
    n = 2 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    for at in (0, T - 1, T, n - 1):
        if case == "cut_last":
            at = n - 1
        if case == "swapped":
            at = min(max(at, 1), n - 2)
        rng = np.random.default_rng(BAD.index(case) + at)
        codes = rng.integers(0, 3, n)
        k = int(method[at])
        F = R.Fr[k]
        good = R.rep_rows[0][k][rank[at]].tobytes()
        special = {int(i): struct.pack(">IB", 1, 1) for i in rng.choice(n, 9, replace=False) if abs(int(i) - at) > 1}
        cut = 0
        if case == "wrong_name":
            b = bytearray(good)
            b[len(R.rep_prefix[k]) - 1] ^= 0x20
            special[at] = bytes(b)
        elif case == "bare_code0":
            special[at] = struct.pack(">IB", 1, 0)
        elif case == "one_longer":
            special[at] = struct.pack(">I", F - 3) + good[4:] + b"\x00"
        elif case == "junk_4k":
            special[at] = struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091)
        elif case == "empty_payload":
            special[at] = struct.pack(">I", 0)
        elif case == "cut_last":
            cut = 3
        buf, offs = reply_stream(R, method, rank, codes, special)
        if case == "swapped":
            offs[at], offs[at + 1] = offs[at + 1], offs[at]
        _, full, wflags, wbad = check(S, method, buf, len(buf) - cut, offs, n)
        assert wflags and not full[at]
        if case != "swapped":  # swapping also breaks the frames beside it
            assert wbad == at and full.sum() == n - 1 - len(special) + (at in special)
        if case == "cut_last":
            break


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds", "big"])
def test_decode_oversize_junk_mid_tile(name, lay):
    """A junk frame larger than the image in the middle of a tile: the frames of
    that tile behind it are read from global memory."""
    S = side(name, lay, True)
    R = S.R
    T = S.mf.tile
    n = 3 * T + 5
    at = T + T // 2
    method = pattern("uniform", n, R.K, T)
    rng = np.random.default_rng(T)
    codes = rng.integers(0, 3, n)
    junk = T * max(R.Fr) + 4096  # more than the T * F_max + 16 bytes a tile stages
    special = {at: struct.pack(">I", junk - 4) + b"\x07" + rng.bytes(junk - 5)}
    buf, offs = reply_stream(R, method, cumcount(method), codes, special)
    want, full, flags, first = check(S, method, buf, len(buf), offs, n)
    assert want[at] == 7 and (flags, first) == (PREFIX, at) and full.sum() == n - 1


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_unanswered_calls(name, lay):
    """nframes < ncalls: the unanswered code, zero leaves, the fill."""
    S = side(name, lay, True)
    R = S.R
    T = S.mf.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    codes = np.random.default_rng(4).integers(0, 3, n)
    for nf in (0, 1, n - 1):
        buf, offs = reply_stream(R, method[:nf], rank[:nf], codes[:nf])
        want, full, flags, _ = check(S, method, buf if nf else b"", len(buf), offs, nf)
        assert full.all() and flags == 0
    # no frames at all needs no buffer
    index = build_index(method, R.K)[:2]
    cap = [int(np.sum(method == k)) for k in range(R.K)]
    d_recs = [empty(cap[k] * S.stride[k] + 16) for k in range(R.K)]
    d_codes, d_scratch = empty(n), empty(S.mf.scratch_bytes)
    assert S.mf.unpack(None, 0, None, 0, index[0], index[1], n, TIMEOUT, d_recs, S.fill, None, cap, d_codes, d_scratch,
                       S.mf.scratch_bytes) == 0
    assert (host(d_codes, n) == TIMEOUT).all()
    got = [host(d_recs[k], cap[k] * S.stride[k]).reshape(cap[k], S.stride[k]) for k in range(R.K)]
    same_structs(got, expected_structs(S, method, np.ones(n, bool), cap))


@pytest.mark.parametrize("lay", LAYS)
def test_decode_bad_calls_keep_their_structs(lay):
    """Ids >= K, and first / cap leaving plan 1 three elements and plan 2 none:
    those calls are the table's first row and nothing is written for them."""
    S = side("kinds", lay, True)
    R = S.R
    T = S.mf.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    method[[5, T, n - 2]] = [R.K, 255, R.K + 1]
    rank = cumcount(method)
    codes = np.random.default_rng(5).integers(0, 3, n)
    n0 = int(np.sum(method == 0))
    first, cap = [7, 10, 40], [7 + n0 + EXTRA, 13, 30]
    known = method < R.K
    elem = np.where(known, np.array(first + [0] * 256)[method] + rank, 0)
    good = known & (elem < np.array(cap + [0] * 256)[method])
    assert (~good).sum() > 10 and good[method == 0].all()
    buf, offs = reply_stream(R, np.where(known, method, 0), np.minimum(elem, NMAX - 1), codes)
    want, full, wflags, wbad = check(S, method, buf, len(buf), offs, n, first=first, cap=cap)
    assert np.array_equal(full, good) and wflags == BOUNDS and wbad == int(np.flatnonzero(~good)[0])
    assert (want[~good] == 0xFF).all()


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_in_two_chunks(name, lay):
    """A second chunk with h_first = the first chunk's counts into the same arrays equals one call."""
    S = side(name, lay, True)
    R = S.R
    T = S.mf.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    codes = np.random.default_rng(8).integers(0, 3, n)
    special = {int(i): struct.pack(">IB", 1, 4) for i in range(3, n, 17)}
    cap = [int(np.sum(method == k)) + EXTRA for k in range(R.K)]
    buf, offs = reply_stream(R, method, rank, codes, special)
    rc, wcodes, whole, wflags, _, _ = run_unpack_aos(S, method, buf, len(buf), offs, n, cap=cap)
    assert rc == 0 and wflags == 0
    zero = np.zeros(n, bool)
    zero[list(special)] = True
    same_structs(whole, expected_structs(S, method, zero, cap))
    for a in (1, T, n - 1):
        counts = [int(c) for c in build_index(method[:a], R.K)[2][:R.K]]
        b1, o1 = reply_stream(R, method[:a], rank[:a], codes[:a], {i: f for i, f in special.items() if i < a})
        rc1, c1, part, f1, _, d_recs = run_unpack_aos(S, method[:a], b1, len(b1), o1, a, cap=cap)
        same_structs(part, expected_structs(S, method[:a], zero[:a], cap))  # the rest still 0xA5
        b2, o2 = reply_stream(R, method[a:], rank[a:], codes[a:], {i - a: f for i, f in special.items() if i >= a})
        rc2, c2, both, f2, _, _ = run_unpack_aos(S, method[a:], b2, len(b2), o2, n - a, first=counts, cap=cap,
                                                 recs=d_recs)
        assert (rc1, rc2, f1, f2) == (0, 0, 0, 0) and np.array_equal(np.concatenate([c1, c2]), wcodes)
        same_structs(both, whole)


@pytest.mark.parametrize("lay", ["natural", "odd"])
@pytest.mark.parametrize("name", ["calc", "kinds", "sixteen"])
def test_round_trip(name, lay):
    """Pack from structs, answer every request on the host with the oracle's
    response row of the same element, decode into structs."""
    Q, S = side(name, lay, False), side(name, lay, True)
    R = S.R
    n = 4097
    method = pattern("uniform", n, R.K, 256)
    rank = cumcount(method)
    rc, raw, offs, flags, _ = run_pack_aos(Q, method)
    assert rc == 0 and flags == 0
    codes = np.random.default_rng(9).integers(0, 3, n)
    parts = []
    for i in range(n):  # the request frame names its method and carries its element's fields
        k = int(method[i])
        frame = raw[offs[i]:offs[i + 1]]
        e = int(np.flatnonzero((R.req_rows[k][rank[i]:rank[i] + 1] == frame).all(axis=1))[0]) + int(rank[i])
        parts.append(R.rep_rows[codes[i]][k][e].tobytes())
    roffs = np.zeros(n, np.uint32)
    roffs[1:] = np.cumsum([len(p) for p in parts[:-1]])
    _, full, wflags, _ = check(S, method, b"".join(parts), sum(map(len, parts)), roffs, n)
    assert full.all() and wflags == 0


def test_refusals_with_real_plans():
    UNS, INV, ALIGN, CAP = (_lib.SRPC_E_UNSUPPORTED, _lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_CAPACITY)
    R = ref("kinds")
    n = 64
    method = pattern("uniform", n, R.K, 256)
    d_method, d_index = build_index(method, R.K)[:2]
    cap = [n] * R.K
    Sq, Sp = side("kinds", "natural", False), side("kinds", "natural", True)
    d_out, d_offs, d_codes = empty(n * max(R.Fq) + 32), empty(4 * (n + 1) + 16), empty(n + 16)
    d_req = [dev(req_structs(Sq, k, n)) for k in range(R.K)]
    d_rep = [empty(n * s + 16) for s in Sp.stride]
    d_buf, d_roffs, d_scratch = empty(256), dev(np.zeros(4, np.uint32)), empty(Sp.mf.scratch_bytes + 16)
    sb = Sp.mf.scratch_bytes

    def pack(mf=Sq.mf, recs=d_req, out=d_out, offs=d_offs, index=d_index, out_cap=n * max(R.Fq)):
        return mf.pack(recs, None, cap, d_method, index, n, out, out_cap, offs)

    def unpack(mf=Sp.mf, recs=d_rep, buf=d_buf, offs=d_roffs, index=d_index, scratch=d_scratch, scratch_bytes=sb,
               fills=Sp.fill):
        return mf.unpack(buf, 100, offs, 1, d_method, index, n, TIMEOUT, recs, fills, None, cap, d_codes, scratch,
                         scratch_bytes)

    def with_layout(S, plans, k, stride=None, offs=None):
        strides, loffs = list(S.stride), [list(o) for o in S.offs]
        if stride is not None:
            strides[k] = stride
        if offs is not None:
            loffs[k] = offs
        return MixedAosFrames(plans, strides, loffs)

    # 2. a string plan, a short prefix, too many leaves, a decode stride above 256
    sp = GpuPacker(Schema("S", (("s", srpc_amd.STRING),)), framed_response_prefix(srpc_amd.NUMBER))
    tiny = GpuPacker(srpc_amd.NUMBER, b"\0\0\0\5")  # room for the BE32, none for a reply's code byte
    bare = GpuPacker(srpc_amd.NUMBER)
    for p, want_req, want_rep in ((sp, UNS, UNS), (tiny, 0, UNS), (bare, UNS, UNS)):
        mf = MixedAosFrames([p], [16], [[8]])
        z = dev(np.zeros(n, np.uint8))
        idx = build_index(np.zeros(n, np.uint8), 1)[1]
        assert mf.pack([d_req[0]], None, [n], z, idx, n, empty(n * 64 + 16), n * 64) == want_req
        assert mf.unpack(d_buf, 23, d_roffs, 1, z, idx, n, TIMEOUT, [d_rep[0]], [bytes(16)], None, [n], d_codes,
                         d_scratch, sb) == want_rep
    big = ref("big").req_plans[0]
    many = MixedAosFrames([big] * 7, [264] * 7, [list(range(8, 264, 8))] * 7)  # 224 leaf fields in all
    assert many.pack([d_req[0]] * 7, None, [1] * 7, d_method, d_index, n, empty(n * 400), n * 400) == UNS
    assert unpack(mf=with_layout(Sp, R.rep_plans, 1, stride=264)) == UNS
    assert unpack(mf=with_layout(Sp, R.rep_plans, 1, stride=264, offs=[300])) == UNS  # before its leaves are looked at
    wide = [d_req[0], empty(n * 264), d_req[2]]
    assert pack(mf=with_layout(Sq, R.req_plans, 1, stride=264), recs=wide) == 0       # the pack takes any stride
    # 3. overlapping leaves, a leaf past the stride (before any alignment)
    o = Sq.offs[0]  # all_kinds: bool, int8, char, int16, int32, int64 at 8, 9, 10, 12, 16, 24
    assert o == [8, 9, 10, 12, 16, 24] and Sp.offs[2] == o
    for S, plans, call, k in ((Sq, R.req_plans, pack, 0), (Sp, R.rep_plans, unpack, 2)):
        assert call(mf=with_layout(S, plans, k, offs=[8, 9, 10, 12, 16, 16])) == INV   # int64 over the int32
        assert call(mf=with_layout(S, plans, k, offs=[8, 8, 10, 12, 16, 24])) == INV
        assert call(mf=with_layout(S, plans, k, offs=[8, 9, 10, 9, 16, 24])) == INV    # misaligned too: INVALID first
        assert call(mf=with_layout(S, plans, k, offs=[8, 9, 10, 12, 16, 28])) == INV   # past the stride
        # 4. alignment: an offset, the stride, an array
        assert call(mf=with_layout(S, plans, k, offs=[8, 9, 10, 13, 16, 24])) == ALIGN
        assert call(mf=with_layout(S, plans, k, stride=36)) == ALIGN                   # the int64 against the stride
        recs = list(d_req if call is pack else d_rep)
        recs[1] = recs[1].data_ptr() + 8
        assert call(recs=recs) == ALIGN
        assert call(index=d_index.data_ptr() + 4) == ALIGN
    assert pack(out=d_out.data_ptr() + 8) == ALIGN
    assert pack(offs=d_offs.data_ptr() + 2) == ALIGN
    assert unpack(buf=d_buf.data_ptr() + 8) == ALIGN
    assert unpack(offs=d_roffs.data_ptr() + 2) == ALIGN
    assert unpack(scratch=d_scratch.data_ptr() + 8) == ALIGN
    # 5. capacity
    assert pack(out_cap=n * max(R.Fq) - 1) == CAP
    assert unpack(scratch_bytes=sb - 1) == CAP
    torch.cuda.synchronize()
    assert (host(d_codes, n + 16) == 0xA5).all() and (host(d_scratch, sb + 16) == 0xA5).all()
    for t, s in zip(d_rep, Sp.stride):
        assert (host(t, n * s + 16) == 0xA5).all()  # nothing was launched
    assert pack() == 0 and unpack(scratch_bytes=sb) == 0


def test_decode_captured_and_replayed():
    """One decode captured on a single stream (a linear graph) and replayed once."""
    S = side("calc", "odd", True)
    R = S.R
    n = 4097
    method = pattern("uniform", n, R.K, 256)
    rank = cumcount(method)
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 3, n)
    special = {int(i): struct.pack(">IB", 1, 3) for i in np.flatnonzero(rng.random(n) < 0.2)}
    buf, offs = reply_stream(R, method, rank, codes, special)
    cap = [int(np.sum(method == k)) for k in range(R.K)]
    want, full, wflags, wbad = model(buf, len(buf), offs, n, method, [0] * R.K, cap, R)
    exp = expected_structs(S, method, ~full, cap, base=[np.zeros((c, s), np.uint8) for c, s in zip(cap, S.stride)])
    d_method, d_index = build_index(method, R.K)[:2]
    d_buf, d_offs = dev(np.frombuffer(buf, np.uint8)), dev(offs)
    d_recs = [torch.zeros(c * s + 16, dtype=torch.uint8, device="cuda") for c, s in zip(cap, S.stride)]
    d_codes = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    sb = S.mf.scratch_bytes
    d_scratch = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    st = status_buf()
    side_stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side_stream):
        assert S.mf.unpack(d_buf, len(buf), d_offs, n, d_method, d_index, n, TIMEOUT, d_recs, S.fill, None, cap, d_codes,
                           d_scratch, sb, st, stream=torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()
    assert not d_codes.any() and not any(t.any() for t in d_recs) and not d_scratch.any()  # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(d_codes, n), want) and read_status(st) == (wflags, wbad)
    same_structs([host(t, c * s).reshape(c, s) for t, c, s in zip(d_recs, cap, S.stride)], exp)
    assert not d_codes[n:].any() and not any(t[c * s:].any() for t, c, s in zip(d_recs, cap, S.stride))
