"""Batches of calls of several methods in call order on the device
(srpc_frames_mixed_index / _pack_requests_mixed / _unpack_replies_mixed,
include/srpc_gpu.h): the client-side mirror of the batched server's mixed
traffic.

Nothing expected comes from the kernels under test:
- ranks and counts are numpy's (`cumcount`);
- every frame is the CPU oracle's pack of one plan's calls in rank order with
  the framed prefix (as tests/test_gpu_replies.py builds `oracle_prefix` and
  `reference`), the rows then interleaved by the method vector in numpy;
- bare and bad reply frames are literal bytes; the expected codes, flags and
  first bad index are the header's table written out per frame (`model`, a
  restatement of test_gpu_replies.model with F and the prefix taken per call).
Outputs are 0xA5-filled with 16 guard bytes behind each; the guards must
survive."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, MixedFrames, Schema, _lib, framed_request_prefix, framed_response_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_parity import ALL_KINDS, dev, empty, host, read_status, status_buf  # noqa: E402
from tests.test_gpu_replies import BAD  # noqa: E402

NO_CODE = 0xFF
PREFIX, BOUNDS = _lib.SRPC_STATUS_PREFIX, _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
NMAX = 50_001
TIMEOUT = srpc_amd.RPC_ERR_RECV_TIMEOUT

I64X8 = Schema.of("Wide", *[(f"w{i}", "int64") for i in range(8)])
FLAG = Schema.of("Flag", ("on", "bool"))
BIG = Schema.of("Big", *[(f"b{i}", "int64") for i in range(32)])  # frames of ~300 bytes: tiles under 256 calls
SVC = "Calculator_servicer::"
# set -> [(method, request schema, reply schema)]
SETS = {
    "calc": [(SVC + "square", srpc_amd.NUMBER, srpc_amd.NUMBER), (SVC + "add", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER),
             (SVC + "subtract", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER),
             (SVC + "multiply", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER)],
    "kinds": [("K_servicer::all", ALL_KINDS, I64X8), ("K_servicer::wide", I64X8, FLAG),
              ("K_servicer::flag", FLAG, ALL_KINDS)],
    "big": [("B_servicer::big", BIG, FLAG), ("B_servicer::flag", FLAG, BIG)],
    "one": [(SVC + "square", srpc_amd.NUMBER, srpc_amd.NUMBER)],
    "sixteen": [(f"S_servicer::m{j:02d}" + "x" * j, srpc_amd.TWO_NUMBERS if j % 2 else srpc_amd.NUMBER,
                 srpc_amd.NUMBER if j % 3 else srpc_amd.TWO_NUMBERS) for j in range(16)],
}
REQ_BYTES = {"calc": [57, 62, 67, 67]}
REPLY_BYTES = {"calc": [23, 23, 23, 23]}


def dtypes(schema):
    return [oracle.KIND_DTYPE[k] for k in schema.kinds]


def random_cols(schema, rng):
    cols = []
    for k, dt in zip(schema.kinds, dtypes(schema)):
        if k == srpc_amd.BOOL:
            c = rng.integers(0, 2, NMAX).astype(dt)
        else:
            info = np.iinfo(dt)
            c = rng.integers(info.min, info.max, NMAX, dtype=np.int64, endpoint=True).astype(dt)
        c.setflags(write=False)
        cols.append(c)
    return cols


class Ref:
    """One set's plans, NMAX elements of every column and the oracle's frames
    of every element: req_rows[k] (NMAX, Fq_k), rep_rows[code][k] (NMAX, Fr_k)."""

    def __init__(self, name):
        self.name = name
        self.methods = SETS[name]
        self.K = len(self.methods)
        rng = np.random.default_rng(len(name))
        self.req_cols, self.rep_cols, self.req_rows, self.rep_prefix = [], [], [], []
        self.rep_rows = [[], [], []]
        for method, rq, rs in self.methods:
            qc, sc = random_cols(rq, rng), random_cols(rs, rng)
            self.req_cols.append(qc)
            self.rep_cols.append(sc)
            pre = oracle.request_prefix(method, rq.name)
            pre = struct.pack(">I", len(pre) + rq.body_bytes) + pre
            w = oracle.pack(rq.kinds, [np.array(c) for c in qc], NMAX, pre)
            self.req_rows.append(np.frombuffer(w, np.uint8).reshape(NMAX, len(pre) + rq.body_bytes))
            for code in (0, 1, 2):
                pre = oracle.response_prefix(code, rs.name)
                pre = struct.pack(">I", len(pre) + rs.body_bytes) + pre
                w = oracle.pack(rs.kinds, [np.array(c) for c in sc], NMAX, pre)
                self.rep_rows[code].append(np.frombuffer(w, np.uint8).reshape(NMAX, len(pre) + rs.body_bytes))
                if code == 0:
                    self.rep_prefix.append(pre)
        self.Fq = [r.shape[1] for r in self.req_rows]
        self.Fr = [r.shape[1] for r in self.rep_rows[0]]
        self.req_plans = [GpuPacker(rq, framed_request_prefix(rq, m)) for m, rq, _ in self.methods]
        self.rep_plans = [GpuPacker(rs, framed_response_prefix(rs, 2)) for _, _, rs in self.methods]  # code ignored
        for p, F in zip(self.req_plans + self.rep_plans, self.Fq + self.Fr):
            assert p.record_bytes == F
        self.req = MixedFrames(self.req_plans)
        self.rep = MixedFrames(self.rep_plans)
        self.d_req_cols = [[dev(c) for c in cols] for cols in self.req_cols]  # read-only on the device


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)


def cumcount(method):
    rank = np.zeros(len(method), np.int64)
    for k in np.unique(method):
        idx = np.flatnonzero(method == k)
        rank[idx] = np.arange(len(idx))
    return rank


def interleave(rows, method, elem, good):
    """The frames rows[method[i]][elem[i]] of the good calls, in call order ->
    (bytes, offsets[n + 1])."""
    n = len(method)
    lens = np.zeros(n, np.int64)
    for k, r in enumerate(rows):
        lens[(method == k) & good] = r.shape[1]
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    flat = np.zeros(int(offs[n]), np.uint8)
    for k, r in enumerate(rows):
        idx = np.flatnonzero((method == k) & good)
        if len(idx):
            flat[(offs[idx][:, None] + np.arange(r.shape[1])[None, :]).reshape(-1)] = r[elem[idx]].reshape(-1)
    return flat, offs


PATTERNS = ["one_plan", "round_robin", "uniform", "skew99", "runs"]


def pattern(which, n, K, T):
    rng = np.random.default_rng(n + K)
    if which == "one_plan":
        m = np.full(n, K - 1)
    elif which == "round_robin":
        m = np.arange(n) % K
    elif which == "uniform":
        m = rng.integers(0, K, n)
    elif which == "skew99":
        m = np.where(rng.random(n) < 0.99, 0, rng.integers(0, K, n))
    else:  # runs of T - 1, T, T + 1 calls of one plan: ranks and offsets cross tile edges at every phase
        runs, j = [], 0
        while sum(runs) < n:
            runs.append(T - 1 + j % 3)
            j += 1
        m = np.repeat(np.arange(len(runs)) % K, runs)[:n]
    return m.astype(np.uint8)


def sizes(T):
    return [0, 1, 2, T - 1, T, T + 1, 3 * T + 5, NMAX]


def build_index(method, K):
    """-> (d_method, d_index, counts[K + 1], flags, first)"""
    n = len(method)
    nb = MixedFrames.index_bytes(n, K)
    d_method = dev(method) if n else empty(16)
    d_index = empty(nb + 16)
    d_counts = empty(8 * (K + 1) + 16)
    st = status_buf()
    assert MixedFrames.index(d_method, n, K, d_index, nb, d_counts, st) == 0
    assert (host(d_index, nb + 16)[nb:] == 0xA5).all() and (host(d_counts, 8 * (K + 1) + 16)[-16:] == 0xA5).all()
    flags, first = read_status(st)
    return d_method, d_index, host(d_counts, 8 * (K + 1), np.uint64), flags, first


def run_pack(R, method, first=None, cap=None, index=None):
    """-> (rc, bytes written up to the total, offsets, flags, first bad); checks
    that nothing at or past the total is written."""
    n = len(method)
    d_method, d_index = index or build_index(method, R.K)[:2]
    out_cap = n * max(R.Fq)
    d_out = empty(out_cap + 16)
    d_offs = empty(4 * (n + 1) + 16)
    st = status_buf()
    st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
    rc = R.req.pack(R.d_req_cols, first, cap or [NMAX] * R.K, d_method, d_index, n, d_out, out_cap, d_offs, st)
    flags, bad = read_status(st)
    offs = host(d_offs, 4 * (n + 1), np.uint32)
    assert (host(d_offs, 4 * (n + 1) + 16)[-16:] == 0xA5).all()
    total = int(offs[n])
    raw = host(d_out, out_cap + 16)
    assert (raw[total:] == 0xA5).all(), "wrote at or past the total"
    return rc, raw[:total], offs, flags, bad


def test_frame_bytes_and_tile():
    R = ref("calc")
    assert R.Fq == REQ_BYTES["calc"] and R.Fr == REPLY_BYTES["calc"]
    K = ref("kinds")
    assert len(set(K.Fq)) == 3 and len(set(K.Fr)) == 3
    assert ref("big").req.tile == ref("big").rep.tile == 64  # a tile smaller than the index's 256 calls
    for name in SETS:
        S = ref(name)
        for mf, F in ((S.req, S.Fq), (S.rep, S.Fr)):
            t = 256
            while t > 16 and t * max(F) > 32768:
                t //= 2
            assert mf.tile == t  # the documented rule


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_ranks_and_counts(name, which):
    R = ref(name)
    T = R.req.tile
    for n in sizes(T):
        method = pattern(which, n, R.K, T)
        d_method, d_index, counts, flags, first = build_index(method, R.K)
        assert (flags, first) == (0, NONE)
        assert np.array_equal(counts, np.append(np.bincount(method, minlength=R.K), 0).astype(np.uint64))
        d_rank = empty(4 * n + 16)
        assert MixedFrames.ranks(d_index, d_method, n, R.K, d_rank) == 0
        assert np.array_equal(host(d_rank, 4 * n, np.uint32), cumcount(method).astype(np.uint32))
        assert (host(d_rank, 4 * n + 16)[-16:] == 0xA5).all()


@pytest.mark.parametrize("p", [0, 300, NMAX - 1])
def test_bad_id(p):
    R = ref("calc")
    method = pattern("uniform", NMAX, R.K, 256)
    method[p] = 200 if p else R.K
    d_method, d_index, counts, flags, first = build_index(method, R.K)
    assert (flags, first) == (BOUNDS, p) and counts[R.K] == 1
    good = method < R.K
    assert np.array_equal(counts[:R.K], np.bincount(method[good], minlength=R.K).astype(np.uint64))
    d_rank = empty(4 * NMAX)
    assert MixedFrames.ranks(d_index, d_method, NMAX, R.K, d_rank) == 0
    got = host(d_rank, 4 * NMAX, np.uint32)
    assert got[p] == 0xFFFFFFFF and np.array_equal(got[good], cumcount(method)[good].astype(np.uint32))
    # the pack leaves the call out and keeps every other frame in order
    rc, raw, offs, flags, first = run_pack(R, method, index=(d_method, d_index))
    want, woffs = interleave(R.req_rows, method, cumcount(method), good)
    assert rc == 0 and (flags, first) == (BOUNDS, p)
    assert np.array_equal(offs, woffs.astype(np.uint32)) and offs[p + 1] == offs[p]
    assert np.array_equal(raw, want)


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_pack(name, which):
    R = ref(name)
    T = R.req.tile
    for n in sizes(T):
        method = pattern(which, n, R.K, T)
        rc, raw, offs, flags, first = run_pack(R, method)
        want, woffs = interleave(R.req_rows, method, cumcount(method), np.ones(n, bool))
        assert rc == 0 and flags == 0
        assert np.array_equal(offs, woffs.astype(np.uint32)), n
        assert np.array_equal(raw, want), n


def test_pack_one_plan_equals_srpc_gpu_pack():
    R = ref("one")
    for n in sizes(R.req.tile):
        rc, raw, _, _, _ = run_pack(R, np.zeros(n, np.uint8))
        wire = empty(n * R.Fq[0])
        R.req_plans[0].pack(R.d_req_cols[0], n, wire)
        assert rc == 0 and np.array_equal(raw, host(wire, n * R.Fq[0]))


@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_pack_in_two_chunks(name):
    R = ref(name)
    T = R.req.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    whole = run_pack(R, method)[1]
    for a in (1, T, n - 1):
        counts = build_index(method[:a], R.K)[2]
        head = run_pack(R, method[:a])[1]
        rc, tail, _, flags, _ = run_pack(R, method[a:], first=[int(c) for c in counts[:R.K]])
        assert rc == 0 and flags == 0
        assert np.array_equal(np.concatenate([head, tail]), whole), a


@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_pack_short_column(name):
    R = ref(name)
    T = R.req.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    k = 1
    cap = [NMAX] * R.K
    cap[k] = int(np.sum(method == k)) - 1
    good = ~((method == k) & (rank >= cap[k]))
    p = int(np.flatnonzero(~good)[0])
    rc, raw, offs, flags, first = run_pack(R, method, cap=cap)
    want, woffs = interleave(R.req_rows, method, rank, good)
    assert rc == 0 and (flags, first) == (BOUNDS, p)
    assert np.array_equal(offs, woffs.astype(np.uint32)) and np.array_equal(raw, want)


# ---- decode -----------------------------------------------------------------------------------

def model(buf, buf_len, offs, nframes, method, first, cap, R):
    """The per-frame table of include/srpc_gpu.h with F and the prefix taken per
    call: (codes, full, flags, first bad) over the frames."""
    rank = cumcount(method)
    codes = np.full(nframes, NO_CODE, np.uint8)
    full = np.zeros(nframes, bool)
    flags, bad = 0, NONE
    for i in range(nframes):
        k = int(method[i])
        flag = 0
        if k >= R.K or first[k] + rank[i] >= cap[k]:
            flag = BOUNDS
        else:
            F, prefix = R.Fr[k], R.rep_prefix[k]
            o = int(offs[i])
            e = int(offs[i + 1]) if i + 1 < nframes else buf_len
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
            bad = min(bad, i)
    return codes, full, flags, bad


def reply_stream(R, method, elem, codes, special=None):
    """Reply frames of the calls: the well-formed frame of plan method[i],
    element elem[i], code codes[i], or special[i] (literal bytes)."""
    special = special or {}
    parts = [special[i] if i in special else R.rep_rows[codes[i]][method[i]][elem[i]].tobytes()
             for i in range(len(method))]
    offs = np.zeros(len(parts), np.uint32)
    if parts:
        offs[1:] = np.cumsum([len(p) for p in parts[:-1]])
    return b"".join(parts), offs


EXTRA = 5  # elements every reply column has beyond the plan's calls: they must keep 0xA5


def run_unpack(R, method, buf, buf_len, offs, nframes, first=None, cap=None, index=None):
    """One decode on fresh 0xA5-filled outputs -> (rc, codes, cols[k][f] as bytes
    of cap[k] elements, flags, first bad); the guards behind every output are
    checked."""
    n = len(method)
    d_method, d_index = index or build_index(method, R.K)[:2]
    first = first or [0] * R.K
    cap = cap or [int(first[k] + np.sum(method == k)) + EXTRA for k in range(R.K)]
    d_buf = dev(np.frombuffer(buf, np.uint8)) if buf else empty(16)
    d_offs = dev(offs) if nframes else empty(16)
    sizes_ = [[np.dtype(dt).itemsize for dt in dtypes(rs)] for _, _, rs in R.methods]
    d_cols = [[empty(cap[k] * s + 16) for s in sizes_[k]] for k in range(R.K)]
    d_codes = empty(n + 16)
    st = status_buf()
    rc = R.rep.unpack(d_buf, buf_len, d_offs, nframes, d_method, d_index, n, TIMEOUT, d_cols, first, cap, d_codes, st)
    flags, bad = read_status(st)
    cols = []
    for k in range(R.K):
        cols.append([])
        for c, s in zip(d_cols[k], sizes_[k]):
            raw = host(c, cap[k] * s + 16)
            assert (raw[cap[k] * s:] == 0xA5).all(), "wrote past a column"
            cols[k].append(raw[:cap[k] * s])
    assert (host(d_codes, n + 16)[n:] == 0xA5).all()
    return rc, host(d_codes, n), cols, flags, bad


def check_cols(R, method, cols, zero, first=None, cap=None):
    """Plan k's element first[k] + r is the input's where call (k, r) decoded,
    zero where `zero` says so for that call, and 0xA5 where no good call maps."""
    first = first or [0] * R.K
    rank = cumcount(method)
    for k, (_, _, rs) in enumerate(R.methods):
        calls = np.flatnonzero(method == k)
        cap_k = len(cols[k][0]) // np.dtype(dtypes(rs)[0]).itemsize
        el = first[k] + rank[calls]
        keep = el < cap_k
        calls, el = calls[keep], el[keep]
        for c, x, dt in zip(cols[k], R.rep_cols[k], dtypes(rs)):
            got = c.view(dt)
            want = np.frombuffer(b"\xa5" * len(c), dt).copy()
            want[el] = np.where(zero[calls], 0, x[el]).astype(dt)
            assert np.array_equal(got, want), (k, dt)


@pytest.mark.parametrize("which", PATTERNS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_decode_all_full(name, which):
    """All-full streams with codes 0, 1, 2; elements beyond a plan's count keep 0xA5."""
    R = ref(name)
    T = R.rep.tile
    for n in sizes(T):
        method = pattern(which, n, R.K, T)
        codes = np.random.default_rng(n).integers(0, 3, n)
        buf, offs = reply_stream(R, method, cumcount(method), codes)
        rc, got, cols, flags, bad = run_unpack(R, method, buf, len(buf), offs, n)
        assert rc == 0 and (flags, bad) == (0, NONE)
        assert np.array_equal(got, codes.astype(np.uint8))
        check_cols(R, method, cols, np.zeros(n, bool))


@pytest.mark.parametrize("share", [0.01, 0.5])
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_bare_frames(name, share):
    R = ref(name)
    n = NMAX
    method = pattern("uniform", n, R.K, R.rep.tile)
    rng = np.random.default_rng(int(100 * share))
    codes = rng.integers(0, 3, n)
    bare = rng.random(n) < share
    special = {int(i): struct.pack(">IB", 1, int(rng.integers(1, 256))) for i in np.flatnonzero(bare)}
    buf, offs = reply_stream(R, method, cumcount(method), codes, special)
    want, full, wflags, wbad = model(buf, len(buf), offs, n, method, [0] * R.K, [NMAX] * R.K, R)
    assert np.array_equal(full, ~bare) and wflags == 0
    rc, got, cols, flags, bad = run_unpack(R, method, buf, len(buf), offs, n)
    assert rc == 0 and (flags, bad) == (0, NONE) and np.array_equal(got, want)
    check_cols(R, method, cols, bare)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("case", BAD)
@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_one_bad_frame(name, case, where):
    R = ref(name)
    T = R.rep.tile
    n = 3 * T + 5
    at = {"first": 0, "middle": T + T // 2, "last": n - 1}[where]
    if case == "cut_last":
        at = n - 1
    if case == "swapped":
        at = min(max(at, 1), n - 2)
    rng = np.random.default_rng(BAD.index(case))
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
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
    buf_len = len(buf) - cut
    want, full, wflags, wbad = model(buf, buf_len, offs, n, method, [0] * R.K, [NMAX] * R.K, R)
    assert wflags and not full[at]
    if case != "swapped":  # swapping also breaks the frames beside it
        assert wbad == at and full.sum() == n - 1 - len(special) + (at in special)
    rc, got, cols, flags, bad = run_unpack(R, method, buf, buf_len, offs, n)
    assert rc == 0 and (flags, bad) == (wflags, wbad)
    assert np.array_equal(got, want)
    check_cols(R, method, cols, ~full)


def test_decode_wrong_plan():
    """Another plan's well-formed reply of another length: PREFIX, zero fields, code payload[0]."""
    R = ref("kinds")
    T = R.rep.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    codes = np.random.default_rng(3).integers(0, 3, n)
    at = T + 3
    other = (int(method[at]) + 1) % R.K
    assert R.Fr[other] != R.Fr[int(method[at])]
    special = {at: R.rep_rows[2][other][0].tobytes()}
    buf, offs = reply_stream(R, method, rank, codes, special)
    rc, got, cols, flags, bad = run_unpack(R, method, buf, len(buf), offs, n)
    want = codes.astype(np.uint8)
    want[at] = 2
    zero = np.zeros(n, bool)
    zero[at] = True
    assert rc == 0 and (flags, bad) == (PREFIX, at) and np.array_equal(got, want)
    check_cols(R, method, cols, zero)


def test_decode_one_plan_equals_unpack_replies():
    R = ref("one")
    T = R.rep.tile
    n = 3 * T + 5
    method = np.zeros(n, np.uint8)
    rng = np.random.default_rng(12)
    codes = rng.integers(0, 3, n)
    special = {int(i): struct.pack(">IB", 1, 9) for i in rng.choice(n, 20, replace=False)}
    special[T + 1] = struct.pack(">I", 4092) + b"\x07" + rng.bytes(4091)
    buf, offs = reply_stream(R, method, np.arange(n), codes, special)
    rc, got, cols, flags, bad = run_unpack(R, method, buf, len(buf), offs, n, cap=[n])
    d_col, d_codes, st = empty(4 * n + 16), empty(n + 16), status_buf()
    assert R.rep_plans[0].unpack_replies(dev(np.frombuffer(buf, np.uint8)), len(buf), dev(offs), n, [d_col], d_codes,
                                         st) == 0
    assert rc == 0 and (flags, bad) == read_status(st) == (PREFIX, T + 1)
    assert np.array_equal(got, host(d_codes, n)) and np.array_equal(cols[0][0], host(d_col, 4 * n))


@pytest.mark.parametrize("name", ["calc", "kinds"])
def test_decode_unanswered_calls(name):
    R = ref(name)
    T = R.rep.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    codes = np.random.default_rng(4).integers(0, 3, n)
    index = build_index(method, R.K)[:2]
    for nf in (0, 1, T, n - 1):
        buf, offs = reply_stream(R, method[:nf], rank[:nf], codes[:nf])
        rc, got, cols, flags, bad = run_unpack(R, method, buf if nf else b"", len(buf), offs, nf, index=index)
        assert rc == 0 and (flags, bad) == (0, NONE)
        assert np.array_equal(got[:nf], codes[:nf].astype(np.uint8)) and (got[nf:] == TIMEOUT).all()
        check_cols(R, method, cols, np.arange(n) >= nf)
    # no frames at all needs no buffer
    d_codes = empty(n)
    cap = [int(np.sum(method == k)) for k in range(R.K)]
    d_cols = [[empty(cap[k] * np.dtype(dt).itemsize + 16) for dt in dtypes(rs)] for k, (_, _, rs) in enumerate(R.methods)]
    assert R.rep.unpack(None, 0, None, 0, index[0], index[1], n, TIMEOUT, d_cols, None, cap, d_codes) == 0
    assert (host(d_codes, n) == TIMEOUT).all()


def test_decode_overflowing_rank():
    """first / cap leave plan 1 three elements and plan 2 none: the calls past
    them are the table's first row and nothing outside the columns is written
    (run_unpack's guards), plan 0 starts at a later element."""
    R = ref("kinds")
    T = R.rep.tile
    n = 3 * T + 5
    method = pattern("uniform", n, R.K, T)
    rank = cumcount(method)
    codes = np.random.default_rng(5).integers(0, 3, n)
    n0 = int(np.sum(method == 0))
    first, cap = [7, 10, 40], [7 + n0, 13, 30]
    good = first_ok = np.array([first[k] + r < cap[k] for k, r in zip(method, rank)])
    assert (~good).sum() > 10 and first_ok[method == 0].all()
    elem = np.array([first[k] + r for k, r in zip(method, rank)])
    buf, offs = reply_stream(R, method, np.minimum(elem, NMAX - 1), codes)
    want, full, wflags, wbad = model(buf, len(buf), offs, n, method, first, cap, R)
    assert np.array_equal(full, good) and wflags == BOUNDS and wbad == int(np.flatnonzero(~good)[0])
    rc, got, cols, flags, bad = run_unpack(R, method, buf, len(buf), offs, n, first=first, cap=cap)
    assert rc == 0 and (flags, bad) == (BOUNDS, wbad) and np.array_equal(got, want)
    check_cols(R, method, cols, np.zeros(n, bool), first=first, cap=cap)


def test_index_pack_decode_captured_and_replayed():
    R = ref("calc")
    n = NMAX
    method = pattern("uniform", n, R.K, R.req.tile)
    rank = cumcount(method)
    codes = np.random.default_rng(6).integers(0, 3, n)
    buf, offs = reply_stream(R, method, rank, codes)
    want, woffs = interleave(R.req_rows, method, rank, np.ones(n, bool))
    nb = MixedFrames.index_bytes(n, R.K)
    d_method, d_index, d_counts = dev(method), torch.zeros(nb, dtype=torch.uint8, device="cuda"), empty(8 * (R.K + 1))
    d_out, d_offs = torch.zeros(n * max(R.Fq), dtype=torch.uint8, device="cuda"), empty(4 * (n + 1))
    d_buf, d_roffs = dev(np.frombuffer(buf, np.uint8)), dev(offs)
    cap = [int(np.sum(method == k)) for k in range(R.K)]
    d_cols = [[torch.zeros(4 * cap[k] + 16, dtype=torch.uint8, device="cuda")] for k in range(R.K)]
    d_codes = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st, st2 = status_buf(), status_buf()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        cur = torch.cuda.current_stream()
        assert MixedFrames.index(d_method, n, R.K, d_index, nb, d_counts, st, stream=cur) == 0
        assert R.req.pack(R.d_req_cols, None, [NMAX] * R.K, d_method, d_index, n, d_out, n * max(R.Fq), d_offs, st,
                          stream=cur) == 0
        assert R.rep.unpack(d_buf, len(buf), d_roffs, n, d_method, d_index, n, TIMEOUT, d_cols, None, cap, d_codes,
                            st2, stream=cur) == 0
    torch.cuda.synchronize()
    assert not d_out.any() and not d_codes.any()  # capturing ran nothing
    st.fill_(0xA5)
    g.replay()
    torch.cuda.synchronize()
    assert read_status(st) == (0, NONE) and read_status(st2) == (0, NONE)
    assert np.array_equal(host(d_out, len(want)), want)
    assert np.array_equal(host(d_offs, 4 * (n + 1), np.uint32), woffs.astype(np.uint32))
    assert np.array_equal(host(d_codes, n), codes.astype(np.uint8))
    for k in range(R.K):
        assert np.array_equal(host(d_cols[k][0], 4 * cap[k], np.int32), R.rep_cols[k][0][:cap[k]])
    # the eager run gives the same bytes
    assert np.array_equal(run_pack(R, method)[1], want)


def test_refusals_with_real_plans():
    L = _lib.lib()
    R = ref("calc")
    n = 64
    method = pattern("uniform", n, R.K, 256)
    d_method, d_index = build_index(method, R.K)[:2]
    d_out, d_offs, d_codes = empty(n * 67 + 32), empty(4 * (n + 1) + 16), empty(n + 16)
    cap = [NMAX] * R.K
    ok = dict(cols=R.d_req_cols, first=None, cap=cap, method=d_method, index=d_index, ncalls=n, out=d_out,
              out_cap=n * 67, offs=d_offs)
    assert R.req.pack(**ok) == 0
    assert R.req.pack(**dict(ok, out_cap=n * 67 - 1)) == _lib.SRPC_E_CAPACITY
    assert R.req.pack(**dict(ok, out=d_out.data_ptr() + 8)) == _lib.SRPC_E_ALIGN
    assert R.req.pack(**dict(ok, offs=d_offs.data_ptr() + 2)) == _lib.SRPC_E_ALIGN
    assert R.req.pack(**dict(ok, index=d_index.data_ptr() + 4)) == _lib.SRPC_E_ALIGN
    cols = [list(c) for c in R.d_req_cols]
    cols[1][0] = cols[1][0].data_ptr() + 4
    assert R.req.pack(**dict(ok, cols=cols)) == _lib.SRPC_E_ALIGN
    sp = GpuPacker(Schema("S", (("s", srpc_amd.STRING),)), framed_response_prefix(srpc_amd.NUMBER))
    tiny = GpuPacker(srpc_amd.NUMBER, b"\0\0\0\5")  # room for the BE32, none for a reply's code byte
    bare = GpuPacker(srpc_amd.NUMBER)
    one = [[R.d_req_cols[0][0]]]
    for p, want_req, want_rep in ((sp, _lib.SRPC_E_UNSUPPORTED, _lib.SRPC_E_UNSUPPORTED),
                                  (tiny, 0, _lib.SRPC_E_UNSUPPORTED),
                                  (bare, _lib.SRPC_E_UNSUPPORTED, _lib.SRPC_E_UNSUPPORTED)):
        mf = MixedFrames([p])
        z = dev(np.zeros(n, np.uint8))
        idx = build_index(np.zeros(n, np.uint8), 1)[1]
        big = empty(n * 64 + 16)
        assert mf.pack(one, None, [NMAX], z, idx, n, big, n * 64) == want_req
        cols = [[empty(4 * n + 16)]]
        assert mf.unpack(empty(64), 23, empty(64), 1, z, idx, n, TIMEOUT, cols, None, [n], d_codes) == want_rep
        torch.cuda.synchronize()
        assert (host(d_codes, n + 16) == 0xA5).all() and (host(cols[0][0], 4 * n) == 0xA5).all()
    many = MixedFrames([GpuPacker(BIG, framed_request_prefix(BIG, "m"))] * 7)  # 224 leaf fields in all
    assert many.pack([[R.d_req_cols[0][0]] * 32] * 7, None, [1] * 7, d_method, d_index, n, empty(n * 400), n * 400) \
        == _lib.SRPC_E_UNSUPPORTED
    # the decode's own argument checks
    rc = [[empty(4 * n + 16)] for _ in range(R.K)]
    assert R.rep.unpack(empty(64), 23, empty(64), n + 1, d_method, d_index, n, TIMEOUT, rc, None, cap,
                        d_codes) == _lib.SRPC_E_INVALID
    assert R.rep.unpack(empty(64), 1 << 32, empty(64), 1, d_method, d_index, n, TIMEOUT, rc, None, cap,
                        d_codes) == _lib.SRPC_E_INVALID
    assert R.rep.unpack(empty(64).data_ptr() + 8, 23, empty(64), 1, d_method, d_index, n, TIMEOUT, rc, None, cap,
                        d_codes) == _lib.SRPC_E_ALIGN
    assert R.rep.unpack(empty(64), 23, None, 1, d_method, d_index, n, TIMEOUT, rc, None, cap,
                        d_codes) == _lib.SRPC_E_INVALID
    torch.cuda.synchronize()
    assert (host(d_codes, n + 16) == 0xA5).all()  # nothing was launched
    assert L.srpc_frames_mixed_index(d_method.data_ptr(), n, R.K, d_index.data_ptr(), 0, empty(64).data_ptr(), None,
                                     None) == _lib.SRPC_E_CAPACITY
