"""Batches of calls of several methods in call order, string-bodied methods
included (srpc_frames_pack_requests_mixed_var / _unpack_replies_mixed_var,
include/srpc_gpu.h): the client-side mirror of batch_server's mixed traffic
with register_var_method legs.

Nothing expected comes from the kernels under test:
- every frame is `BE32 | payload`, the payload the CPU oracle's pack of one
  plan's elements in rank order (`oracle.pack(..., str_offsets=...)`) cut at
  record boundaries computed from the string lengths, the frames then
  interleaved by the method vector in numpy / Python;
- bare and bad reply frames are literal bytes; the expected codes, flags and
  first bad index are the header's two tables restated per frame (`model`);
- the expected fields and strings are the inputs where a frame is full, zero /
  empty elsewhere.
Outputs are 0xA5-filled with 16 guard bytes behind each; the guards must
survive.  Every case asserts that its input holds the rows or regimes it names."""
import functools
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, MixedFrames, MixedVarFrames, Schema, _lib, framed_request_prefix, framed_response_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import MULTIPLE, _rec_offsets, dev, empty, host, read_status, status_buf  # noqa: E402

NO_CODE = 0xFF
PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
INVALID, ALIGN, UNSUPPORTED, CAPACITY = (_lib.SRPC_E_INVALID, _lib.SRPC_E_ALIGN, _lib.SRPC_E_UNSUPPORTED,
                                         _lib.SRPC_E_CAPACITY)
NONE = 2**64 - 1
STRING = oracle.STRING
TIMEOUT = srpc_amd.RPC_ERR_RECV_TIMEOUT
MAXSTR = 16

FLAG = Schema.of("Flag", ("on", "bool"))
TEXT = Schema.of("Text", ("text", "string"))
TEXT2 = Schema.of("Text2", ("a", "string"), ("b", "string"))
MIX = Schema.of("Mix", ("a", "string"), ("b", "int32"), ("n", "int64"), ("c", "string"), ("d", "int16"))
S16 = Schema.of("S16", *[(f"s{i:02d}", "string") for i in range(16)])
SVC = "Calculator_servicer::"
CALC = [(SVC + "square", srpc_amd.NUMBER, srpc_amd.NUMBER), (SVC + "add", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER),
        (SVC + "subtract", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER), (SVC + "multiply", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER)]
ECHO = ("Echo_servicer::echo", MULTIPLE, MULTIPLE)
_STR16 = [TEXT, MIX, TEXT2, MULTIPLE, TEXT, MIX, TEXT2, S16]
# set -> [(method, request schema, reply schema)]
SETS = {
    "echo": [ECHO],
    "calc_echo": CALC + [ECHO],
    "two_str": [("T_servicer::mix", MIX, TEXT2), ("T_servicer::text", TEXT, MIX), ("T_servicer::flag", FLAG, FLAG)],
    "sixteen": [(f"S_servicer::m{j:02d}" + "x" * j,
                 _STR16[j // 2] if j % 2 else (srpc_amd.TWO_NUMBERS if j % 4 else srpc_amd.NUMBER),
                 _STR16[7 - j // 2] if j % 2 else srpc_amd.NUMBER) for j in range(16)],
}
# a set that only the tests naming it use (it stays out of every case parametrised over SETS): two fixed
# Calculator methods and one method with two string fields each way
PAIR_SETS = {"calc_text2": [CALC[1], CALC[3], ("T_servicer::both", TEXT2, TEXT2)]}


def is_var(schema):
    return STRING in schema.kinds


def nstr(schema):
    return sum(k == STRING for k in schema.kinds)


def fixed_part(schema, prefix_len):
    """The frame without its chars: BE32, prefix, fixed fields, 8 per string."""
    return 4 + prefix_len + sum(8 if k == STRING else oracle.KIND_SIZE[k] for k in schema.kinds)


class Plans:
    def __init__(self, name):
        self.methods = SETS.get(name) or PAIR_SETS[name]
        self.K = len(self.methods)
        self.req_plans = [GpuPacker.for_request(rq, m) if is_var(rq) else GpuPacker(rq, framed_request_prefix(rq, m))
                          for m, rq, _ in self.methods]
        self.rep_plans = [GpuPacker.for_response(rs, 2) if is_var(rs) else GpuPacker(rs, framed_response_prefix(rs, 2))
                          for _, _, rs in self.methods]  # the plans' own code byte is ignored
        self.req, self.rep = MixedVarFrames(self.req_plans), MixedVarFrames(self.rep_plans)
        self.req_prefix = [oracle.request_prefix(m, rq.name) for m, rq, _ in self.methods]
        self.rep_prefix = [oracle.response_prefix(0, rs.name) for _, _, rs in self.methods]
        self.req_fixed = [fixed_part(rq, len(p)) for (_, rq, _), p in zip(self.methods, self.req_prefix)]
        self.rep_fixed = [fixed_part(rs, len(p)) for (_, _, rs), p in zip(self.methods, self.rep_prefix)]


@functools.lru_cache(maxsize=None)
def plans(name):
    return Plans(name)


def test_sets_and_tile_rule():
    assert plans("echo").req_plans[0].path == srpc_amd.SRPC_PATH_VAR
    S = plans("sixteen")
    assert S.K == 16 and max(nstr(rq) for _, rq, _ in S.methods) == 16 and max(nstr(rs) for _, _, rs in S.methods) == 16
    assert sum(is_var(rq) for _, rq, _ in S.methods) == 8
    for name in SETS:
        P = plans(name)
        for mv, fixed in ((P.req, P.req_fixed), (P.rep, P.rep_fixed)):
            t = 256
            while t > 16 and t * max(fixed) > 32768:
                t //= 2
            assert mv.tile == (t, 32768)  # the documented rule
    assert plans("sixteen").req.tile[0] == 128  # a tile smaller than the index's 256 calls


PATTERNS = ["one_plan", "round_robin", "uniform", "skew99", "runs"]


def pattern(which, n, K, T, name):
    rng = np.random.default_rng(n + K)
    if which == "one_plan":  # a string plan
        m = np.full(n, K - 1 if name != "two_str" else 0)
    elif which == "round_robin":
        m = np.arange(n) % K
    elif which == "uniform":
        m = rng.integers(0, K, n)
    elif which == "skew99":  # 99 % of the calls are one string plan's
        hot = K - 1 if name != "two_str" else 0
        m = np.where(rng.random(n) < 0.99, hot, rng.integers(0, K, n))
    else:  # runs of T - 1, T, T + 1 calls of one plan
        runs, j = [], 0
        while sum(runs) < n:
            runs.append(T - 1 + j % 3)
            j += 1
        m = np.repeat(np.arange(len(runs)) % K, runs)[:n]
    return m.astype(np.uint8)


def cumcount(method):
    rank = np.zeros(len(method), np.int64)
    for k in np.unique(method):
        idx = np.flatnonzero(method == k)
        rank[idx] = np.arange(len(idx))
    return rank


REGIMES = ["empty", "short", "mid", "edges", "over_first", "over_mid", "over_last", "over_two"]


def call_lens(regime, method, schemas, fixed, T, image):
    """lens[t][i]: the length of call i's t-th string (ignored past its plan's
    strings).  `edges` and `over_*` place their frames by the stream offsets,
    which follow from the lengths chosen so far."""
    n = len(method)
    rng = np.random.default_rng(n + len(regime))
    if regime == "empty":
        return np.zeros((MAXSTR, n), np.int64)
    if regime == "short":
        return rng.integers(0, 17, (MAXSTR, n))
    lens = rng.integers(0, 301, (MAXSTR, n)) if regime == "mid" else rng.integers(0, 41, (MAXSTR, n))
    if regime == "mid":
        return lens
    var = np.array([is_var(s) for s in schemas])[method]
    ns = np.array([nstr(s) for s in schemas])[method]
    base = np.array(fixed)[method]  # frame bytes without chars
    for t in range(MAXSTR):
        lens[t][ns <= t] = 0
    if regime.startswith("over"):
        tile = np.flatnonzero(var[T:2 * T]) + T  # the string calls of the second tile
        assert len(tile) >= 2, "the second tile needs string calls"
        pick = {"over_first": [tile[0]], "over_mid": [tile[len(tile) // 2]], "over_last": [tile[-1]],
                "over_two": [tile[0], tile[-1]]}[regime]
        for i in pick:
            lens[ns[i] - 1][i] = image + 1000  # the call's last string
        return lens
    # edges: every third string call ends its frame on a 16-byte edge; in tile 1 a frame ends exactly at the
    # end of the image window, in tile 3 one byte past it
    o, A, done = 0, 0, set()
    for i in range(n):
        if i % T == 0:
            A = o & ~15
        if var[i]:
            rest = base[i] + int(lens[1:, i].sum())
            tile = i // T
            if tile in (1, 3) and tile not in done and i % T >= T // 2:
                want = A + image + (tile == 3) - o - rest
                if want >= 0:
                    lens[0][i] = want
                    done.add(tile)
            elif i % 3 == 0:
                lens[0][i] = (-(o + rest)) % 16 + 16 * (i % 2)
        o += base[i] + (int(lens[:, i].sum()) if var[i] else 0)
    assert done == {1, 3} or n < 4 * T
    return lens


def make_leg(schema, prefix_of_code, n, lens, seed):
    """n elements of a schema -> (cols, offs, frames[code][e]); lens[t][e]."""
    kinds = schema.kinds
    rng = np.random.default_rng(seed)
    cols, offs, t = [], [], 0
    for k in kinds:
        if k == STRING:
            o = np.zeros(n + 1, np.uint64)
            o[1:] = np.cumsum(np.asarray(lens[t][:n], np.uint64))
            c = ((np.arange(max(int(o[n]), 1), dtype=np.uint64) * 7 + 3 + 11 * t + seed) % 256).astype(np.uint8)
            t += 1
        else:
            dt = np.dtype(oracle.KIND_DTYPE[k])
            c = rng.integers(0, 256, max(n, 1) * dt.itemsize, dtype=np.uint8).view(dt)[:n].copy()
            if k == srpc_amd.BOOL:
                c &= 1
            o = None
        c.setflags(write=False)
        cols.append(c)
        offs.append(o)
    frames = []
    for pre in prefix_of_code:
        rec = _rec_offsets(kinds, offs, n, len(pre))
        w = oracle.pack(kinds, [np.array(c) for c in cols], n, pre, [None if o is None else np.array(o) for o in offs]) \
            if n else b""
        assert len(w) == int(rec[n])
        frames.append([struct.pack(">I", int(rec[e + 1] - rec[e])) + w[int(rec[e]):int(rec[e + 1])] for e in range(n)])
    return cols, offs, frames


class Batch:
    """n calls of a set: the method vector, per plan the request and reply legs
    (inputs and the oracle's frames per element)."""

    def __init__(self, name, n, which, regime):
        P = self.P = plans(name)
        self.n = n
        T, image = P.req.tile
        self.method = pattern(which, n, P.K, T, name)
        self.rank = cumcount(self.method)
        self.counts = [int(np.sum(self.method == k)) for k in range(P.K)]
        qlens = call_lens(regime, self.method, [m[1] for m in P.methods], P.req_fixed, T, image)
        T2, _ = P.rep.tile
        slens = call_lens(regime, self.method, [m[2] for m in P.methods], P.rep_fixed, T2, image)
        self.req, self.rep = [], []
        for k, (m, rq, rs) in enumerate(P.methods):
            idx = np.flatnonzero(self.method == k)
            self.req.append(make_leg(rq, [P.req_prefix[k]], len(idx), qlens[:, idx], 17 + k))
            self.rep.append(make_leg(rs, [oracle.response_prefix(c, rs.name) for c in (0, 1, 2)], len(idx),
                                     slens[:, idx], 91 + k))

    def req_frames(self, good=None):
        return [self.req[k][2][0][r] if good is None or good[i] else b""
                for i, (k, r) in enumerate(zip(self.method, self.rank))]

    def rep_frames(self, codes):
        return [self.rep[k][2][c][r] for k, r, c in zip(self.method, self.rank, codes)]


@functools.lru_cache(maxsize=16)
def batch(name, n, which, regime):
    return Batch(name, n, which, regime)


def joined(parts):
    offs = np.zeros(len(parts) + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    return b"".join(parts), offs


def build_index(method, K):
    n = len(method)
    nb = MixedFrames.index_bytes(n, K)
    d_method = dev(method) if n else empty(16)
    d_index = empty(nb + 16)
    d_counts = empty(8 * (K + 1) + 16)
    assert MixedFrames.index(d_method, n, K, d_index, nb, d_counts, None) == 0
    return d_method, d_index, host(d_counts, 8 * (K + 1), np.uint64)


def dev_leg(leg):
    cols, offs, _ = leg
    return [dev(c) for c in cols], [None if o is None else dev(o) for o in offs]


def run_pack(B, method=None, out_cap=None, first=None, cap=None, legs=None, scratch=None):
    """-> (rc, the out buffer's bytes, d_offs, total, flags, first bad).  The
    guards behind the outputs are checked."""
    P = B.P
    method = B.method if method is None else method
    n = len(method)
    d_method, d_index, _ = build_index(method, P.K)
    legs = legs or [dev_leg(l) for l in B.req]
    full = sum(len(f) for f in B.req_frames())
    out_cap = full if out_cap is None else out_cap
    d_out = empty(out_cap + 16)
    d_offs = empty(4 * (n + 1) + 16)
    d_total = empty(8 + 16)
    sb = P.req.scratch_bytes(n)
    d_scratch = scratch if scratch is not None else empty(sb + 16)
    st = status_buf()
    st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
    rc = P.req.pack([l[0] for l in legs], [l[1] for l in legs], first, cap or B.counts, d_method, d_index, n, d_out,
                    out_cap, d_offs, d_total, st, d_scratch, sb)
    flags, bad = read_status(st)
    raw = host(d_out, out_cap + 16)
    assert (raw[out_cap:] == 0xA5).all(), "wrote at or past out_cap"
    assert (host(d_offs, 4 * (n + 1) + 16)[-16:] == 0xA5).all() and (host(d_total, 24)[8:] == 0xA5).all()
    end = d_scratch.numel() - 16  # a caller's scratch may be larger than this chunk needs
    assert end >= sb and (host(d_scratch, end + 16)[end:] == 0xA5).all(), "wrote past the scratch"
    return rc, raw[:out_cap], host(d_offs, 4 * (n + 1), np.uint32), int(host(d_total, 8, np.uint64)[0]), flags, bad


def check_pack(B, got, good=None, out_cap=None):
    rc, raw, offs, total, flags, bad = got
    want, woffs = joined(B.req_frames(good))
    cap = len(want) if out_cap is None else out_cap
    assert rc == 0 and total == len(want)
    assert np.array_equal(offs, np.minimum(woffs, cap).astype(np.uint32))
    ends = woffs[1:]
    fit = int(ends[ends <= cap].max()) if (ends <= cap).any() else 0  # the frames ending at or before the cap are complete
    assert raw[:fit].tobytes() == want[:fit]
    assert (raw[max(fit, min(cap, len(want))):] == 0xA5).all(), "wrote at or past the total"
    over = np.flatnonzero(ends > cap)
    bads = np.flatnonzero(~good) if good is not None else np.zeros(0, np.int64)
    first = min([int(x[0]) for x in (over, bads) if len(x)], default=NONE)
    assert (flags, bad) == ((BOUNDS, first) if first != NONE else (0, NONE))
    return want, woffs


def sizes(T):
    return sorted({0, 1, 255, 256, 257, T - 1, T, T + 1, 4097})


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_pack(name, which):
    T = plans(name).req.tile[0]
    for n in sizes(T):
        B = batch(name, n, which, "mid" if name != "sixteen" else "short")
        check_pack(B, run_pack(B))


@pytest.mark.parametrize("name", sorted(SETS))
def test_pack_50001(name):
    B = batch(name, 50_001, "uniform", "short")
    assert len(set(B.method)) == B.P.K
    check_pack(B, run_pack(B))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["echo", "calc_echo", "two_str"])
def test_pack_length_regimes(name, regime):
    P = plans(name)
    T, image = P.req.tile
    B = batch(name, 4 * T + 5, "uniform" if name != "echo" else "one_plan", regime)
    want, woffs = check_pack(B, run_pack(B))
    lens = np.diff(woffs)
    if regime == "empty":
        assert set(lens) == {P.req_fixed[k] for k in set(B.method)}
    if regime == "edges":
        nvar = sum(is_var(P.methods[k][1]) for k in B.method)
        assert (woffs[1:] % 16 == 0).sum() >= nvar // 4, "every third string call's frame ends on a 16-byte edge"
        A = int(woffs[T]) & ~15
        assert A + image in woffs[T + 1:2 * T + 1], "a frame ending exactly at the image window's end"
        A = int(woffs[3 * T]) & ~15
        assert A + image + 1 in woffs[3 * T + 1:4 * T + 1], "a frame ending one byte past the window"
    if regime.startswith("over"):
        big = np.flatnonzero(lens > image)
        assert len(big) == (2 if regime == "over_two" else 1) and (big // T == 1).all(), "oversize frames in tile 1"
        var = np.flatnonzero([is_var(P.methods[k][1]) for k in B.method][T:2 * T]) + T
        where = {"over_first": var[:1], "over_mid": var[len(var) // 2:len(var) // 2 + 1], "over_last": var[-1:],
                 "over_two": var[[0, -1]]}[regime]
        assert np.array_equal(big, where)


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_pack_out_cap(name):
    B = batch(name, 1000, "uniform", "mid")
    want, woffs = joined(B.req_frames())
    for cap in (len(want), len(want) - 1, int(woffs[1]) - 1, int(woffs[500]) + 3):
        got = run_pack(B, out_cap=cap)
        check_pack(B, got, out_cap=cap)
        if cap < len(want):
            assert got[4] == BOUNDS and got[5] == int(np.flatnonzero(woffs[1:] > cap)[0])


def test_pack_decreasing_offsets_pair():
    B = batch("two_str", 1000, "uniform", "mid")
    legs = [dev_leg(l) for l in B.req]
    k, e = 0, 77  # plan 0 (Mix), element 77: its second string's offsets pair decreases
    offs = np.array(B.req[k][1][3])
    assert offs[e + 1] > offs[e] > 0
    offs[e + 1] = offs[e] - 1
    legs[k][1][3] = dev(offs)
    i = int(np.flatnonzero((B.method == k) & (B.rank == e))[0])
    good = np.ones(B.n, bool)
    good[i] = False
    # the element after it starts at the smaller offset: its frame is the oracle's of those chars
    nxt = int(np.flatnonzero((B.method == k) & (B.rank == e + 1))[0])
    rc, raw, got_offs, total, flags, bad = run_pack(B, legs=legs)
    parts = B.req_frames(good)
    assert rc == 0 and (flags, bad) == (BOUNDS, i) and got_offs[i + 1] == got_offs[i]
    want, woffs = joined(parts[:nxt])
    assert raw[:len(want)].tobytes() == want and np.array_equal(got_offs[:nxt + 1], woffs.astype(np.uint32))


def test_pack_cap_one_element_short():
    B = batch("calc_echo", 1000, "uniform", "mid")
    for k in (1, 4):  # a fixed plan, the string plan
        cap = list(B.counts)
        cap[k] -= 1
        good = ~((B.method == k) & (B.rank >= cap[k]))
        assert (~good).sum() == 1
        check_pack(B, run_pack(B, cap=cap), good=good)


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_pack_in_two_chunks(name):
    B = batch(name, 1000, "uniform", "mid")
    want, woffs = joined(B.req_frames())
    legs = [dev_leg(l) for l in B.req]
    for a in (1, 256, 999):
        counts = [int(np.sum(B.method[:a] == k)) for k in range(B.P.K)]
        h = run_pack(B, method=B.method[:a], legs=legs, out_cap=int(woffs[a]))
        t = run_pack(B, method=B.method[a:], legs=legs, out_cap=len(want) - int(woffs[a]), first=counts)
        assert h[0] == 0 and t[0] == 0 and h[4] == 0 and t[4] == 0
        assert h[1].tobytes() + t[1].tobytes() == want, a
        assert h[3] == int(woffs[a]) and t[3] == len(want) - int(woffs[a])


def test_pack_dirty_scratch_same_output():
    """The scratch another batch left behind (more calls, another method mix,
    another length regime: a stale word equal to the right one would hide a
    missing reset), then the same batch twice."""
    B = batch("calc_echo", 1000, "uniform", "mid")
    A = batch("calc_echo", 1537, "skew99", "short")
    assert A.n != B.n and A.counts != B.counts
    sb = max(B.P.req.scratch_bytes(B.n), A.P.req.scratch_bytes(A.n))
    scratch = empty(sb + 16)
    check_pack(A, run_pack(A, scratch=scratch))
    assert (host(scratch, B.P.req.scratch_bytes(B.n)) != 0xA5).any(), "the first batch left the scratch untouched"
    a = run_pack(B, scratch=scratch)
    check_pack(B, a)
    b = run_pack(B, scratch=scratch)
    check_pack(B, b)
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


# ---- decode -----------------------------------------------------------------------------------

def model(buf, buf_len, offs, nframes, B, first, cap):
    """The two per-frame tables of include/srpc_gpu.h, each call judged under
    its own plan: (codes, full, flags, first bad) over the frames."""
    P = B.P
    codes = np.full(nframes, NO_CODE, np.uint8)
    full = np.zeros(nframes, bool)
    flags, bad = 0, NONE
    for i in range(nframes):
        k = int(B.method[i])
        flag = 0
        if k >= P.K or first[k] + B.rank[i] >= cap[k]:
            flag = BOUNDS
        else:
            kinds, prefix = P.methods[k][2].kinds, P.rep_prefix[k]
            o = int(offs[i])
            e = int(offs[i + 1]) if i + 1 < nframes else buf_len
            if o > e or e > buf_len or e - o < 5:
                flag = BOUNDS
            else:
                f, ln = buf[o:e], e - o
                if int.from_bytes(f[:4], "big") != ln - 4:
                    flag = BOUNDS
                else:
                    codes[i] = f[4]
                    Pn = len(prefix)
                    if ln == 5 and f[4] != 0:
                        pass  # bare
                    elif STRING not in kinds:
                        if ln == P.rep_fixed[k] and f[5:4 + Pn] == prefix[1:]:
                            full[i] = True
                        else:
                            flag = PREFIX
                    elif ln - 4 < Pn or f[5:4 + Pn] != prefix[1:]:
                        flag = PREFIX
                    else:
                        c, ok = 4 + Pn, True
                        for kind in kinds:
                            if kind == STRING:
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
                                if oracle.KIND_SIZE[kind] > ln - c:
                                    ok = False
                                    break
                                c += oracle.KIND_SIZE[kind]
                        if ok and c == ln:
                            full[i] = True
                        else:
                            flag = BOUNDS
        if flag:
            flags |= flag
            bad = min(bad, i)
    return codes, full, flags, bad


EXTRA = 3  # elements every reply column has beyond the leg's calls: they must keep 0xA5


class Outs:
    """The reply side's device buffers of a whole batch (all chunks)."""

    def __init__(self, B, str_cap_cut=0):
        P = B.P
        self.B = B
        self.cap = [c + EXTRA for c in B.counts]
        self.cols, self.offs, self.scap = [], [], []
        for k, (_, _, rs) in enumerate(P.methods):
            cs, os_, caps = [], [], []
            for f, kind in enumerate(rs.kinds):
                if kind == STRING:
                    total = int(B.rep[k][1][f][-1])
                    caps.append(max(total - str_cap_cut, 0))
                    cs.append(empty(caps[-1] + 16))
                    os_.append(empty(8 * (self.cap[k] + 1) + 16))
                else:
                    caps.append(None)
                    cs.append(empty(self.cap[k] * oracle.KIND_SIZE[kind] + 16))
                    os_.append(None)
            self.cols.append(cs)
            self.offs.append(os_)
            self.scap.append(caps)
        self.nslots = sum(nstr(rs) for _, _, rs in P.methods)


def run_unpack(B, O, buf, buf_len, offs, nframes, lo=0, hi=None, first=None, scratch=None, null_buf=False):
    """One decode of calls [lo, hi) -> (rc, codes, ends, flags, first bad)."""
    P = B.P
    method = B.method[lo:hi]
    n = len(method)
    d_method, d_index, _ = build_index(method, P.K)
    d_buf = None if null_buf else (dev(np.frombuffer(buf, np.uint8)) if buf else empty(16))
    d_offs = None if null_buf else (dev(np.asarray(offs, np.uint32)) if nframes else empty(16))
    d_codes = empty(n + 16)
    d_ends = empty(8 * O.nslots + 16)
    sb = P.rep.scratch_bytes(n)
    d_scratch = scratch if scratch is not None else empty(sb + 16)
    st = status_buf()
    rc = P.rep.unpack(d_buf, buf_len, d_offs, nframes, d_method, d_index, n, TIMEOUT, O.cols, O.offs, O.scap, first,
                      O.cap, d_codes, d_ends, st, d_scratch, sb)
    flags, bad = read_status(st)
    assert (host(d_codes, n + 16)[n:] == 0xA5).all() and (host(d_ends, 8 * O.nslots + 16)[8 * O.nslots:] == 0xA5).all()
    end = d_scratch.numel() - 16  # a caller's scratch may be larger than this chunk needs
    assert end >= sb and (host(d_scratch, end + 16)[end:] == 0xA5).all(), "wrote past the scratch"
    return rc, host(d_codes, n).copy(), host(d_ends, 8 * O.nslots, np.uint64).copy(), flags, bad


def check_outs(B, O, full, touched=None, ends=None, skip=()):
    """Plan k's element r is the input's where call (k, r) is full, zero / empty
    where it is not, and 0xA5 where no good call maps (`touched`: the calls
    decoded so far, default all)."""
    P = B.P
    touched = np.ones(B.n, bool) if touched is None else touched
    slot = 0
    for k, (_, _, rs) in enumerate(P.methods):
        if k in skip:
            slot += nstr(rs)
            continue
        calls = np.flatnonzero((B.method == k) & touched)
        el = B.rank[calls]
        keep = el < O.cap[k]
        calls, el = calls[keep], el[keep]
        cnt = len(el)
        assert np.array_equal(el, np.arange(cnt))  # chunks are decoded in order
        cols, offs, _ = B.rep[k]
        for f, kind in enumerate(rs.kinds):
            if kind == STRING:
                xo = offs[f].astype(np.int64)
                ln = np.where(full[calls], np.diff(xo)[el], 0)
                want_o = np.zeros(cnt + 1, np.uint64)
                want_o[1:] = np.cumsum(ln)
                raw_o = host(O.offs[k][f], 8 * (O.cap[k] + 1) + 16)
                assert np.array_equal(raw_o[:8 * (cnt + 1)].view(np.uint64), want_o), (k, f)
                assert (raw_o[8 * (cnt + 1):] == 0xA5).all(), "wrote past the leg's offsets"
                if ends is not None:
                    assert int(ends[slot]) == int(want_o[cnt])
                slot += 1
                want_c = b"".join(cols[f][int(xo[e]):int(xo[e + 1])].tobytes() for c, e in zip(calls, el) if full[c])
                scap = O.scap[k][f]
                raw_c = host(O.cols[k][f], scap + 16)
                m = min(len(want_c), scap)
                assert raw_c[:m].tobytes() == want_c[:m], (k, f)
                assert (raw_c[m:] == 0xA5).all(), "wrote past the chars or the column's capacity"
            else:
                dt = oracle.KIND_DTYPE[kind]
                sz = oracle.KIND_SIZE[kind]
                raw = host(O.cols[k][f], O.cap[k] * sz + 16)
                assert (raw[O.cap[k] * sz:] == 0xA5).all(), "wrote past a column"
                want = np.frombuffer(b"\xa5" * (O.cap[k] * sz), dt).copy()
                want[el] = np.where(full[calls], cols[f][el], 0).astype(dt)
                assert np.array_equal(raw[:O.cap[k] * sz].view(dt), want), (k, f)


def decode_and_check(B, parts, nframes=None, buf_len_cut=0, offs_edit=None, str_cap_cut=0, scratch=None):
    nframes = B.n if nframes is None else nframes
    buf, offs = joined(parts[:nframes])
    offs = offs[:nframes].copy()
    if offs_edit:
        offs_edit(offs)
    buf_len = len(buf) - buf_len_cut
    O = Outs(B, str_cap_cut)
    rc, codes, ends, flags, bad = run_unpack(B, O, buf, buf_len, offs, nframes, scratch=scratch)
    wc, full, wflags, wbad = model(buf, buf_len, offs, nframes, B, [0] * B.P.K, O.cap)
    assert rc == 0
    assert np.array_equal(codes[:nframes], wc) and (codes[nframes:] == TIMEOUT).all()
    assert (flags, bad) == (wflags, wbad)
    allfull = np.zeros(B.n, bool)
    allfull[:nframes] = full
    check_outs(B, O, allfull, ends=ends)
    return codes, allfull, flags, bad, ends, O


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_all_full(name, which):
    """All-full streams with codes 0, 1, 2."""
    T = plans(name).rep.tile[0]
    for n in sizes(T):
        B = batch(name, n, which, "mid" if name != "sixteen" else "short")
        codes = np.random.default_rng(n).integers(0, 3, n)
        got, full, flags, _, _, _ = decode_and_check(B, B.rep_frames(codes))
        assert full.all() and flags == 0 and np.array_equal(got, codes.astype(np.uint8))
        if n > 2:
            assert set(codes) == {0, 1, 2}


@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_50001(name):
    B = batch(name, 50_001, "uniform", "short")
    codes = np.random.default_rng(5).integers(0, 3, B.n)
    _, full, flags, _, _, _ = decode_and_check(B, B.rep_frames(codes))
    assert full.all() and flags == 0


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["echo", "calc_echo", "two_str"])
def test_decode_length_regimes(name, regime):
    P = plans(name)
    T, image = P.rep.tile
    B = batch(name, 4 * T + 5, "uniform" if name != "echo" else "one_plan", regime)
    parts = B.rep_frames(np.zeros(B.n, np.int64))
    _, full, flags, _, _, _ = decode_and_check(B, parts)
    assert full.all() and flags == 0
    lens = np.array([len(p) for p in parts])
    if regime.startswith("over"):
        assert (lens > image).sum() == (2 if regime == "over_two" else 1)
    if regime == "edges":
        nvar = sum(is_var(P.methods[k][2]) for k in B.method)
        assert (np.cumsum(lens) % 16 == 0).sum() >= nvar // 4


BARE = struct.pack(">IB", 1, 1)
BAD = ["wrong_name", "bare_code0", "one_longer", "junk_4k", "cut_last", "swapped", "empty_payload",  # test_gpu_replies
       "str_past_end", "ends_early", "len_2_63", "len_2_64m1", "short_prefix", "other_plan"]  # test_gpu_replies_var


@pytest.mark.parametrize("case", BAD)
@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_decode_one_bad_frame(name, case):
    """One bad frame in the second tile (the last frame for cut_last) among full
    frames of mixed codes and a few bare ones, once under a fixed plan's call and
    once under a string plan's; every frame around it must still decode."""
    P = plans(name)
    T = P.rep.tile[0]
    B = batch(name, 3 * T + 5, "uniform", "mid")
    rng = np.random.default_rng(BAD.index(case))
    codes = rng.integers(0, 3, B.n)
    for want_var in (False, True):
        var = np.array([is_var(P.methods[k][2]) for k in B.method])
        at = int(np.flatnonzero(var[T + T // 2:] == want_var)[0]) + T + T // 2
        if case == "cut_last":
            at = B.n - 1
            if var[at] != want_var:
                continue
        k = int(B.method[at])
        kinds = P.methods[k][2].kinds
        if case in ("str_past_end", "ends_early", "len_2_63", "len_2_64m1") and not want_var:
            continue
        parts = B.rep_frames(codes)
        for i in rng.choice(B.n, 9, replace=False):
            if abs(int(i) - at) > 1:
                parts[int(i)] = BARE
        good = B.rep[k][2][0][B.rank[at]]
        pl = len(P.rep_prefix[k])
        cut, edit, want_at = 0, None, None  # (code, flag) of the bad frame
        first_str = 4 + pl + sum(oracle.KIND_SIZE[x] for x in kinds[:list(kinds).index(STRING)]) if want_var else 0
        if case == "wrong_name":
            b = bytearray(good)
            b[4 + pl - 1] ^= 0x20
            parts[at], want_at = bytes(b), (0, PREFIX)
        elif case == "bare_code0":
            parts[at], want_at = struct.pack(">IB", 1, 0), (0, PREFIX)
        elif case == "one_longer":
            parts[at] = struct.pack(">I", len(good) - 3) + good[4:] + b"\x00"
            want_at = (0, BOUNDS if want_var else PREFIX)  # a string plan's walk ends before the frame's end
        elif case == "junk_4k":
            parts[at], want_at = struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091), (7, PREFIX)
        elif case == "cut_last":
            cut, want_at = 2, (NO_CODE, BOUNDS)
        elif case == "swapped":
            def edit(o):
                o[at], o[at + 1] = o[at + 1], o[at]
        elif case == "empty_payload":
            parts[at], want_at = struct.pack(">I", 0), (NO_CODE, BOUNDS)
        elif case == "str_past_end":
            b = bytearray(good)
            b[first_str:first_str + 8] = struct.pack("<Q", len(good))
            parts[at], want_at = bytes(b), (0, BOUNDS)
        elif case == "ends_early":
            parts[at] = struct.pack(">I", len(good) + 3) + good[4:] + b"\x00" * 7
            want_at = (0, BOUNDS)
        elif case in ("len_2_63", "len_2_64m1"):
            b = bytearray(good)
            b[first_str:first_str + 8] = struct.pack("<Q", 2**63 if case == "len_2_63" else 2**64 - 1)
            parts[at], want_at = bytes(b), (0, BOUNDS)
        elif case == "short_prefix":
            body = good[4:4 + pl - 2]
            parts[at], want_at = struct.pack(">I", len(body)) + body, (0, PREFIX)
        elif case == "other_plan":  # a frame that is valid for another plan than its call's
            other = next(j for j in range(P.K) if P.rep_prefix[j] != P.rep_prefix[k] and B.counts[j])
            parts[at], want_at = B.rep[other][2][0][0], (0, PREFIX)
        got, full, flags, bad, _, _ = decode_and_check(B, parts, buf_len_cut=cut, offs_edit=edit)
        assert not full[at] and flags and bad <= at
        if want_at:
            assert got[at] == want_at[0] and flags & want_at[1]
        bare = np.array([i for i in range(B.n) if parts[i] is BARE], np.int64)
        assert len(bare) >= 6  # 9 drawn, at most 3 within a call of the bad frame
        assert (got[bare] == 1).all() and not full[bare].any()  # bare frames keep their code and decode to nothing
        assert full.sum() >= B.n - len(bare) - 3  # the others decode


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_decode_nframes(name):
    B = batch(name, 1000, "uniform", "mid")
    parts = B.rep_frames(np.zeros(B.n, np.int64))
    for nf in (B.n // 2, B.n):
        codes, full, flags, _, _, _ = decode_and_check(B, parts, nframes=nf)
        assert flags == 0 and full.sum() == nf
    O = Outs(B)
    rc, codes, ends, flags, bad = run_unpack(B, O, b"", 0, None, 0, null_buf=True)
    assert rc == 0 and (codes == TIMEOUT).all() and (flags, bad) == (0, NONE) and (ends == 0).all()
    check_outs(B, O, np.zeros(B.n, bool), ends=ends)


@pytest.mark.parametrize("cut", [0, 1])
def test_decode_str_cap(cut):
    """h_str_cap exact and one byte short: the offsets still count every full
    frame, d_ends shows the overflow, nothing at or past the capacity is written."""
    B = batch("two_str", 1000, "uniform", "mid")
    _, full, flags, _, ends, O = decode_and_check(B, B.rep_frames(np.zeros(B.n, np.int64)), str_cap_cut=cut)
    caps = [c for k in range(B.P.K) for c in O.scap[k] if c is not None]
    assert full.all() and flags == 0 and all(int(e) == c + cut for e, c in zip(ends, caps)) and len(caps) == 4


def test_decode_cap_one_element_short():
    B = batch("calc_echo", 1000, "uniform", "mid")
    parts = B.rep_frames(np.zeros(B.n, np.int64))
    buf, offs = joined(parts)
    for k in (1, 4):
        O = Outs(B)
        O.cap[k] = B.counts[k] - 1  # the buffers keep their size: the last element must stay 0xA5
        rc, codes, ends, flags, bad = run_unpack(B, O, buf, len(buf), offs[:-1], B.n)
        last = int(np.flatnonzero((B.method == k) & (B.rank == B.counts[k] - 1))[0])
        assert rc == 0 and (flags, bad) == (BOUNDS, last) and codes[last] == NO_CODE
        full = np.ones(B.n, bool)
        full[last] = False
        touched = np.ones(B.n, bool)
        touched[last] = False
        O.cap[k] = B.counts[k] + EXTRA
        check_outs(B, O, full, touched=touched)


@pytest.mark.parametrize("name", ["calc_echo", "two_str"])
def test_decode_in_two_chunks_and_dirty_scratch(name):
    """Two chunks with continuing offsets equal the whole; the same call on
    dirty scratch gives the same outputs."""
    B = batch(name, 1000, "uniform", "mid")
    codes = np.random.default_rng(3).integers(0, 3, B.n)
    parts = B.rep_frames(codes)
    # the scratch starts as another batch's decode left it: more calls, another mix and length regime
    A = batch(name, 1537, "skew99", "short")
    assert A.n != B.n and A.counts != B.counts
    for a in (1, 256, 999):
        O = Outs(B)
        scratch = empty(max(B.P.rep.scratch_bytes(B.n), A.P.rep.scratch_bytes(A.n)) + 16)
        decode_and_check(A, A.rep_frames(np.random.default_rng(a).integers(0, 3, A.n)), scratch=scratch)
        assert (host(scratch, B.P.rep.scratch_bytes(B.n)) != 0xA5).any(), "the first batch left the scratch untouched"
        buf, offs = joined(parts[:a])
        rc, c1, _, flags, _ = run_unpack(B, O, buf, len(buf), offs[:-1], a, lo=0, hi=a, scratch=scratch)
        assert rc == 0 and flags == 0
        touched = np.arange(B.n) < a
        check_outs(B, O, np.ones(B.n, bool), touched=touched)
        first = [int(np.sum(B.method[:a] == k)) for k in range(B.P.K)]
        buf, offs = joined(parts[a:])
        for _ in range(2):  # again on the scratch the calls before left behind
            rc, c2, ends, flags, _ = run_unpack(B, O, buf, len(buf), offs[:-1], B.n - a, lo=a, hi=None, first=first,
                                                scratch=scratch)
            assert rc == 0 and flags == 0
            assert np.array_equal(np.concatenate([c1, c2]), codes.astype(np.uint8))
            check_outs(B, O, np.ones(B.n, bool), ends=ends)


def test_refusals_in_order():
    """Past the argument checks (tests/test_mixed_var_abi.py): every UNSUPPORTED
    refusal comes before every ALIGN refusal, every ALIGN refusal before
    CAPACITY, nothing launched.  A refusal is shown to come first by making the
    later ones true as well: a misaligned d_out / d_buf under every UNSUPPORTED
    case, a scratch size of 0 under every ALIGN case."""
    B = batch("calc_echo", 1000, "uniform", "mid")
    P = B.P
    d_method, d_index, _ = build_index(B.method, P.K)
    legs = [dev_leg(l) for l in B.req]
    cols, so = [l[0] for l in legs], [l[1] for l in legs]
    out, offs, total, scratch = empty(1 << 20), empty(4 * 1001), empty(16), empty(1 << 20)
    sb = P.req.scratch_bytes(B.n)
    s17 = Schema.of("S17", *[(f"s{i:02d}", "string") for i in range(17)])  # one string too many
    wide = Schema.of("W", *[(f"w{i}", "int8") for i in range(31)], ("s", "string"))  # 7 x 32 = 224 leaves

    def edited(rows, k, f, by):
        rows = [list(r) for r in rows]
        rows[k][f] = rows[k][f].data_ptr() + by
        return rows

    def pack(mv=P.req, cols=cols, so=so, index=d_index, out=out, offs=offs, total=total, scratch=scratch, sb_given=0):
        return mv.pack(cols, so, None, B.counts, d_method, index, B.n, out, 1 << 19, offs, total, None, scratch, sb_given)

    odd_out = out.data_ptr() + 1
    assert pack(sb_given=sb) == 0
    unsupported = {
        "a string plan without a prefix": P.req_plans[:4] + [GpuPacker(MULTIPLE, b"")],
        "a fixed plan with a prefix under 4 bytes": [GpuPacker(srpc_amd.NUMBER, b"abc")] + P.req_plans[1:],
        "a string plan with 17 strings": P.req_plans[:4] + [GpuPacker.for_request(s17, "S_servicer::many")],
        "more than 192 leaves": [GpuPacker.for_request(wide, f"W_servicer::m{j}") for j in range(7)],
    }
    for what, pl in unsupported.items():
        mv = MixedVarFrames(pl)
        assert pack(mv=mv, out=odd_out) == UNSUPPORTED, what
        assert pack(mv=mv, sb_given=sb) == UNSUPPORTED, what
        out64, t, img = _lib.C.c_uint64(7), _lib.C.c_uint32(7), _lib.C.c_uint32(7)
        assert _lib.lib().srpc_frames_mixed_var_scratch_bytes(mv._plans, mv.k, 10, _lib.C.byref(out64)) == UNSUPPORTED, what
        assert _lib.lib().srpc_frames_mixed_var_tile(mv._plans, mv.k, _lib.C.byref(t), _lib.C.byref(img)) == UNSUPPORTED
        assert (out64.value, t.value, img.value) == (7, 7, 7)
    misaligned = {
        "d_out (16)": dict(out=out.data_ptr() + 8),
        "a fixed column (16)": dict(cols=edited(cols, 1, 0, 8)),
        "a string column (16)": dict(cols=edited(cols, 4, 3, 8)),
        "a string's offsets array (8)": dict(so=edited(so, 4, 3, 4)),
        "the index (8)": dict(index=d_index.data_ptr() + 4),
        "d_total (8)": dict(total=total.data_ptr() + 4),
        "the scratch (8)": dict(scratch=scratch.data_ptr() + 4),
        "d_offs (4)": dict(offs=offs.data_ptr() + 2),
    }
    for what, kw in misaligned.items():
        assert pack(**kw) == ALIGN, what  # with no scratch at all: ALIGN comes before CAPACITY
    assert pack(sb_given=sb - 1) == CAPACITY
    assert pack(sb_given=0) == CAPACITY
    torch.cuda.synchronize()
    # the existing mixed calls still refuse string plans
    t = _lib.C.c_uint32()
    assert _lib.lib().srpc_frames_mixed_tile(P.req._plans, P.K, _lib.C.byref(t)) == UNSUPPORTED
    mf = MixedFrames(P.req_plans)
    assert mf.pack(cols, None, B.counts, d_method, d_index, B.n, out, 1 << 20, offs, None) == UNSUPPORTED
    O = Outs(B)
    mr = MixedFrames(P.rep_plans)
    assert mr.unpack(out, 100, offs, 3, d_method, d_index, B.n, TIMEOUT, O.cols, None, O.cap, empty(B.n), None) == UNSUPPORTED

    # the decode, in the same way
    rsb = P.rep.scratch_bytes(B.n)
    ends, codes = empty(64), empty(B.n)

    def unpack(mv=P.rep, buf=out, cols=O.cols, so=O.offs, index=d_index, offs=offs, ends=ends, scratch=scratch, sb_given=0):
        return mv.unpack(buf, 100, offs, 3, d_method, index, B.n, TIMEOUT, cols, so, O.scap, None, O.cap, codes, ends, None,
                         scratch, sb_given)

    unsupported = {
        "a string plan without a prefix": P.rep_plans[:4] + [GpuPacker(MULTIPLE, b"")],
        "a fixed reply plan with a prefix under 5 bytes": [GpuPacker(srpc_amd.NUMBER, b"abcd")] + P.rep_plans[1:],
        "a string plan with 17 strings": P.rep_plans[:4] + [GpuPacker.for_response(s17, 0)],
        "more than 192 leaves": [GpuPacker.for_response(wide, 0) for j in range(7)],
    }
    for what, pl in unsupported.items():
        mv = MixedVarFrames(pl)
        assert unpack(mv=mv, buf=odd_out) == UNSUPPORTED, what
        assert unpack(mv=mv, sb_given=rsb) == UNSUPPORTED, what
    misaligned = {
        "d_buf (16)": dict(buf=out.data_ptr() + 8),
        "a fixed column (16)": dict(cols=edited(O.cols, 1, 0, 8)),
        "a string column (16)": dict(cols=edited(O.cols, 4, 3, 8)),
        "a string's offsets array (8)": dict(so=edited(O.offs, 4, 3, 4)),
        "the index (8)": dict(index=d_index.data_ptr() + 4),
        "d_ends (8)": dict(ends=ends.data_ptr() + 4),
        "the scratch (8)": dict(scratch=scratch.data_ptr() + 4),
        "d_offs (4)": dict(offs=offs.data_ptr() + 2),
    }
    for what, kw in misaligned.items():
        assert unpack(**kw) == ALIGN, what
    assert unpack(sb_given=rsb - 1) == CAPACITY
    assert unpack(sb_given=0) == CAPACITY
    torch.cuda.synchronize()
    # nothing was launched by a refused decode: the outputs are untouched
    assert (host(codes, B.n) == 0xA5).all() and (host(ends, 64) == 0xA5).all()


def test_first_past_the_capacity():
    """h_first[k] > h_cap[k] is h_first[k] == h_cap[k]: every call of the plan is
    BAD, its columns and offsets stay untouched, the other plans decode."""
    B = batch("calc_echo", 1000, "uniform", "mid")
    parts = B.rep_frames(np.zeros(B.n, np.int64))
    buf, offs = joined(parts)
    O = Outs(B)
    first = [0] * B.P.K
    first[4] = O.cap[4] + 1000  # the string plan
    rc, codes, ends, flags, bad = run_unpack(B, O, buf, len(buf), offs[:-1], B.n, first=first)
    echo = B.method == 4
    assert rc == 0 and (flags, bad) == (BOUNDS, int(np.flatnonzero(echo)[0]))
    assert (codes[echo] == NO_CODE).all() and (codes[~echo] == 0).all()
    check_outs(B, O, ~echo, touched=~echo, skip=(4,))
    for c, o in zip(O.cols[4], O.offs[4]):  # not an element, not an offsets entry
        assert (host(c, c.numel()) == 0xA5).all() and (o is None or (host(o, o.numel()) == 0xA5).all())
    got = run_pack(B, first=first)  # the pack: no frame for the plan's calls
    check_pack(B, got, good=~echo)


def test_scratch_bytes_monotone():
    for name in SETS:
        P = plans(name)
        for mv in (P.req, P.rep):
            sizes_ = [mv.scratch_bytes(n) for n in (0, 1, 255, 256, 257, 4097, 50_001, 1_000_000)]
            assert sizes_ == sorted(sizes_) and all(s % 8 == 0 for s in sizes_)
