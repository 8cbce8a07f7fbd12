"""A batch of request frames of several methods decoded in arrival order on the
device (srpc_frames_unpack_requests_mixed, include/srpc_gpu.h), and the ordered
reply pack (srpc_frames_pack_requests_mixed over response plans with d_method =
d_class).

Nothing expected comes from the kernels under test:
- every frame is the CPU oracle's pack of one element of a method's request
  columns behind its framed prefix (tests/test_gpu_mixed.Ref), the frames
  interleaved in numpy; foreign frames are the oracle's pack behind the prefix of
  a method nobody registered (method 0's name with its last char changed: the
  same length as method 0's frames);
- classes come from `model`, the header's rule written out on the host, and are
  checked against the class each frame was built to have;
- ranks are numpy's (`cumcount`), fields the columns the frames were packed from.
Outputs are 0xA5-filled with 16 guard bytes behind each; the guards must
survive.  Every input's d_class is also compared with srpc_frames_classify's."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import FrameClassifier, GpuPacker, MixedFrames, Schema, _lib, framed_request_prefix, framed_response_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_mixed import BIG, NMAX, cumcount, interleave, ref  # noqa: E402
from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402

UNKNOWN = _lib.SRPC_FRAME_UNKNOWN
BOUNDS = _lib.SRPC_STATUS_BOUNDS
NONE = 2**64 - 1
GUARD = 16
SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 50_001]
# set -> (set of tests/test_gpu_mixed.SETS, its methods in registration order)
PLAN_SETS = {"calc": ("calc", None), "kinds": ("kinds", None), "big": ("big", None), "one": ("one", None),
             "sixteen": ("sixteen", None),
             "twice": ("calc", [0, 1, 0, 3])}  # square registered twice: the first wins, the second counts 0


class Srv:
    """A server's view of one plan set: the request plans it registered, the
    oracle's request frames and the columns they were packed from, a foreign
    method's frames, the response plans (RPC_SUCCESS) and the oracle's replies."""

    def __init__(self, name):
        base, pick = PLAN_SETS[name]
        R = ref(base)
        pick = list(range(R.K)) if pick is None else pick
        self.K = len(pick)
        self.methods = [R.methods[i] for i in pick]
        self.req_cols = [R.req_cols[i] for i in pick]
        self.req_rows = [R.req_rows[i] for i in pick]
        self.rep_cols = [R.rep_cols[i] for i in pick]
        self.rep_rows = [R.rep_rows[0][i] for i in pick]
        self.Fq = [r.shape[1] for r in self.req_rows]
        self.Fr = [r.shape[1] for r in self.rep_rows]
        self.req_prefix = []
        for m, rq, _ in self.methods:
            pre = oracle.request_prefix(m, rq.name)
            self.req_prefix.append(np.frombuffer(struct.pack(">I", len(pre) + rq.body_bytes) + pre, np.uint8))
        self.req_plans = [GpuPacker(rq, framed_request_prefix(rq, m)) for m, rq, _ in self.methods]
        self.rep_plans = [GpuPacker(rs, framed_response_prefix(rs, 0)) for _, _, rs in self.methods]
        self.req = MixedFrames(self.req_plans)
        self.rep = MixedFrames(self.rep_plans)
        self.classifier = FrameClassifier(list(zip(self.req_plans, self.Fr)))
        m0, rq0, _ = self.methods[0]
        pre = oracle.request_prefix(m0[:-1] + ("#" if m0[-1] != "#" else "$"), rq0.name)
        pre = struct.pack(">I", len(pre) + rq0.body_bytes) + pre
        w = oracle.pack(rq0.kinds, [np.array(c) for c in self.req_cols[0]], NMAX, pre)
        self.foreign_rows = np.frombuffer(w, np.uint8).reshape(NMAX, len(pre) + rq0.body_bytes)
        assert self.foreign_rows.shape[1] == self.Fq[0]

    @functools.cached_property
    def d_rep_cols(self):
        return [[dev(c) for c in cols] for cols in self.rep_cols]

    @functools.cached_property
    def d_req_cols(self):
        return [[dev(c) for c in cols] for cols in self.req_cols]


@functools.lru_cache(maxsize=None)
def srv(name):
    return Srv(name)


def model(S, buf, buf_len, offs):
    """d_class by the header's rule: frame i is bytes [offs[i], end_i), end_i the
    next offset or buf_len; it is plan k's when its length is F_k and it starts
    with plan k's prefix, the first such plan winning; UNKNOWN otherwise."""
    n = len(offs)
    cls = np.full(n, UNKNOWN, np.uint8)
    if n == 0:
        return cls
    o = offs.astype(np.int64)
    e = np.append(o[1:], buf_len)
    inside = (o <= e) & (e <= buf_len)
    for k in reversed(range(S.K)):  # reversed: a lower k overwrites, the first match wins
        cand = np.flatnonzero(inside & (e - o == S.Fq[k]))
        if not len(cand):
            continue
        pre = S.req_prefix[k]
        eq = (buf[o[cand][:, None] + np.arange(len(pre))[None, :]] == pre[None, :]).all(axis=1)
        cls[cand[eq]] = k
    return cls


def run(S, buf, buf_len, offs, first=None, cap=None, alloc=None, status=True):
    """-> dict of everything the call wrote (guards included)."""
    n = len(offs)
    K = S.K
    d_buf = dev(buf) if len(buf) else empty(16)
    d_offs = dev(offs.astype(np.uint32)) if n else empty(16)
    sizes = [[np.dtype(c.dtype).itemsize for c in cols] for cols in S.req_cols]
    d_cols = [[empty(alloc[k] * s + GUARD) for s in sizes[k]] for k in range(K)]
    nb = MixedFrames.index_bytes(n, K)
    d_cls, d_index, d_counts = empty(n + GUARD), empty(nb + GUARD), empty(8 * (K + 1) + GUARD)
    st = status_buf()
    st[:] = 0x5A  # the call resets it
    rc = S.req.unpack_requests(d_buf, buf_len, d_offs, n, d_cols, first, cap, d_cls, d_index, nb, d_counts,
                               st if status else None)
    assert rc == 0
    flags, bad = read_status(st) if status else (None, None)
    raw_cls = host(d_cls, n + GUARD)
    assert (raw_cls[n:] == 0xA5).all() and (host(d_index, nb + GUARD)[nb:] == 0xA5).all()
    raw_counts = host(d_counts, 8 * (K + 1) + GUARD)
    assert (raw_counts[-GUARD:] == 0xA5).all()
    cols = [[host(c, alloc[k] * s + GUARD).copy() for c, s in zip(d_cols[k], sizes[k])] for k in range(K)]
    return dict(cls=raw_cls[:n].copy(), counts=raw_counts[:8 * (K + 1)].view(np.uint64).copy(), cols=cols, flags=flags,
                bad=bad, d_cls=d_cls, d_index=d_index, d_buf=d_buf, d_offs=d_offs)


def classify_cls(S, d_buf, buf_len, d_offs, n):
    """d_class as srpc_frames_classify writes it for the same buffer."""
    K = S.K
    d_cls, d_idx = empty(n + GUARD), empty(4 * K * n + GUARD)
    d_counts, d_out_off = empty(8 * (K + 2)), empty(8 * (n + 1))
    sb = S.classifier.scratch_bytes(n)
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda:0")
    S.classifier.classify(d_buf, buf_len, d_offs, n, d_cls, d_idx, d_counts, d_out_off, scratch, sb)
    return host(d_cls, n).copy()


def check(S, buf, buf_len, offs, intent, elem, first=None, cap=None, alloc=None):
    """Run the call and compare everything it wrote with the host's expectation.
    intent[i]: the class frame i was built to have; elem[i]: the element of its
    method's columns it was packed from.  cap / alloc default to exactly the
    elements the frames need.  -> the run."""
    n, K = len(offs), S.K
    want = model(S, buf, buf_len, offs)
    assert np.array_equal(want, intent), "the stream is not what the test meant to build"
    rank = cumcount(want)
    counts = [int((want == k).sum()) for k in range(K)]
    f0 = [0] * K if first is None else list(first)
    cap = [f0[k] + counts[k] for k in range(K)] if cap is None else list(cap)
    alloc = [max(cap[k], f0[k] + counts[k]) for k in range(K)] if alloc is None else list(alloc)
    got = run(S, buf, buf_len, offs, first, cap, alloc)
    assert np.array_equal(got["cls"], want)
    assert np.array_equal(classify_cls(S, got["d_buf"], buf_len, got["d_offs"], n), want)
    assert got["counts"].tolist() == counts + [int((want == UNKNOWN).sum())]
    bad = NONE
    for k in range(K):
        idx = np.flatnonzero(want == k)
        e = f0[k] + rank[idx]
        ok = e < cap[k]
        if not ok.all():
            bad = min(bad, int(idx[~ok][0]))
        for f, c in enumerate(S.req_cols[k]):
            exp = np.full(alloc[k] * c.dtype.itemsize + GUARD, 0xA5, np.uint8)
            view = exp[:alloc[k] * c.dtype.itemsize].view(c.dtype)
            view[e[ok]] = c[elem[idx[ok]]]
            assert np.array_equal(got["cols"][k][f], exp), (k, f)
    assert (got["flags"], got["bad"]) == ((BOUNDS, bad) if bad != NONE else (0, NONE))
    return got


def method_vector(K, n, order, foreign, seed=0, used=None):
    """-> intent: the class of every frame (UNKNOWN for a foreign method's)."""
    rng = np.random.default_rng(1000 * n + 10 * K + seed)
    used = np.arange(K) if used is None else np.asarray(used)
    if order == "uniform":
        m = used[rng.integers(0, len(used), n)]
    elif order == "alternating":
        m = used[np.arange(n) % len(used)]
    else:  # all of method 0, then all of method 1, ...
        m = used[np.arange(n) * len(used) // max(n, 1)]
    m = m.astype(np.uint8)
    if foreign >= 1.0:
        m[:] = UNKNOWN
    elif foreign > 0:
        m[rng.random(n) < foreign] = UNKNOWN
    return m


def stream(S, intent):
    """The frames of `intent` in order -> (buf, offs[n], buf_len, elem)."""
    n = len(intent)
    elem = (np.arange(n) * 31 + 7) % NMAX
    mm = np.where(intent == UNKNOWN, S.K, intent)
    buf, offs = interleave(S.req_rows + [S.foreign_rows], mm, elem, np.ones(n, bool))
    return buf, offs[:n].astype(np.uint32), int(offs[n]), elem


def used_methods(name):
    return [0, 1, 3] if name == "twice" else None  # the second registration's frames are the first's


@pytest.mark.parametrize("order", ["uniform", "alternating", "blocks"])
@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_sizes_and_orders(name, order):
    S = srv(name)
    for n in SIZES:
        intent = method_vector(S.K, n, order, 0.01, used=used_methods(name))
        buf, offs, buf_len, elem = stream(S, intent)
        got = check(S, buf, buf_len, offs, intent, elem)
        if name == "twice":
            assert got["counts"][2] == 0


@pytest.mark.parametrize("foreign", [0.0, 0.01, 0.5, 1.0])
@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_foreign_share(name, foreign):
    S = srv(name)
    for n in (257, 4097):
        intent = method_vector(S.K, n, "uniform", foreign, seed=1, used=used_methods(name))
        buf, offs, buf_len, elem = stream(S, intent)
        check(S, buf, buf_len, offs, intent, elem)


# ---- hostile frames among good neighbours -----------------------------------------------------

HN = 700
SPOTS = [0, 130, 256, 389, 511, HN - 1]  # tile edges and middles, each between good frames


def frame_list(S, n, seed):
    intent = method_vector(S.K, n, "uniform", 0.0, seed=seed)
    elem = (np.arange(n) * 31 + 7) % NMAX
    frames = [S.req_rows[int(intent[i])][elem[i]].copy() for i in range(n)]
    return intent, elem, frames


def assemble(frames):
    lens = np.array([len(f) for f in frames], np.int64)
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    buf = np.concatenate(frames) if len(frames) else np.zeros(0, np.uint8)
    return buf, offs[:-1].astype(np.uint32), int(offs[-1])


def flip(at):
    """One wrong byte at offset `at` (negative: from the prefix's end) of a right-length frame."""
    def edit(S, k, f):
        g = f.copy()
        g[at if at >= 0 else len(S.req_prefix[k]) + at] ^= 0x01
        return g
    return edit


EDITS = {
    "be32": flip(3),             # the frame's BE32 length
    "method_length": flip(4),    # the u64 length of the method string
    "method_char": flip(12 + 5),
    "last_prefix_byte": flip(-1),
    "one_longer": lambda S, k, f: np.append(f, np.uint8(0)),
    "one_shorter": lambda S, k, f: f[:-1].copy(),
    "three_bytes": lambda S, k, f: f[:3].copy(),
    "empty": lambda S, k, f: f[:0].copy(),
}


@pytest.mark.parametrize("what", sorted(EDITS))
@pytest.mark.parametrize("name", ["calc", "big"])
def test_hostile_frame(name, what):
    S = srv(name)
    intent, elem, frames = frame_list(S, HN, seed=len(what))
    for p in SPOTS:
        frames[p] = EDITS[what](S, int(intent[p]), frames[p])
        intent[p] = UNKNOWN
    buf, offs, buf_len = assemble(frames)
    check(S, buf, buf_len, offs, intent, elem)


@pytest.mark.parametrize("name", ["calc", "big"])
def test_junk_longer_than_the_image(name):
    """A 40 KiB frame: longer than the 32 KiB image, so the frames behind it in
    its tile are read from global memory."""
    S = srv(name)
    intent, elem, frames = frame_list(S, HN, seed=40)
    rng = np.random.default_rng(40)
    for p in (0, 300):
        frames[p] = rng.integers(0, 256, 40 * 1024, dtype=np.uint8)
        frames[p][:4] = np.frombuffer(struct.pack(">I", 40 * 1024 - 4), np.uint8)  # a well-formed frame of nobody's
        intent[p] = UNKNOWN
    buf, offs, buf_len = assemble(frames)
    check(S, buf, buf_len, offs, intent, elem)


@pytest.mark.parametrize("name", ["calc", "big"])
def test_offsets_out_of_order(name):
    S = srv(name)
    intent, elem, frames = frame_list(S, HN, seed=7)
    buf, offs, buf_len = assemble(frames)
    for p in (200, 256, 511):
        # frame p - 1 now spans three frames, frame p runs backwards, frame p + 1 is whole
        offs[p] = offs[p + 2]
        intent[p - 1] = intent[p] = UNKNOWN
    check(S, buf, buf_len, offs, intent, elem)


@pytest.mark.parametrize("name", ["calc", "big"])
def test_frames_past_buf_len(name):
    S = srv(name)
    intent, elem, frames = frame_list(S, HN, seed=9)
    buf, offs, total = assemble(frames)
    # the last frame cut by one byte
    cut = intent.copy()
    cut[-1] = UNKNOWN
    check(S, buf, total - 1, offs, cut, elem)
    # the last frame starts past buf_len
    far = offs.copy()
    far[-1] = total + 8
    cut = intent.copy()
    cut[-2:] = UNKNOWN  # the one before it now ends past buf_len
    check(S, buf, total, far, cut, elem)
    # buf_len inside frame 650 (the allocation holds the whole stream): it and every later frame are nobody's
    cut = intent.copy()
    cut[650:] = UNKNOWN
    check(S, buf, int(offs[650]) + S.Fq[int(intent[650])] - 2, offs, cut, elem)


# ---- h_first / h_cap --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["calc", "kinds", "big"])
def test_second_chunk(name):
    """Non-zero h_first: the elements before it stay untouched."""
    S = srv(name)
    n = 1000
    intent = method_vector(S.K, n, "uniform", 0.05, seed=2)
    buf, offs, buf_len, elem = stream(S, intent)
    check(S, buf, buf_len, offs, intent, elem, first=[5 + 11 * k for k in range(S.K)])


@pytest.mark.parametrize("name", ["calc", "kinds", "big"])
def test_short_column(name):
    """h_cap[k] one short of the count: BOUNDS with the smallest such frame, its
    element (allocated, past the cap) untouched, everything else exact."""
    S = srv(name)
    n = 1000
    intent = method_vector(S.K, n, "uniform", 0.05, seed=3)
    buf, offs, buf_len, elem = stream(S, intent)
    counts = [int((intent == k).sum()) for k in range(S.K)]
    k = S.K - 1
    cap = list(counts)
    cap[k] -= 1
    got = check(S, buf, buf_len, offs, intent, elem, cap=cap, alloc=counts)
    assert got["bad"] == int(np.flatnonzero(intent == k)[-1]) and got["cls"][got["bad"]] == k
    # with a non-zero first as well
    first = [3] * S.K
    check(S, buf, buf_len, offs, intent, elem, first=first, cap=[3 + c for c in cap], alloc=[3 + c for c in counts])


def test_null_status():
    S = srv("calc")
    intent = method_vector(S.K, 300, "uniform", 0.1, seed=4)
    buf, offs, buf_len, _ = stream(S, intent)
    counts = [int((intent == k).sum()) for k in range(S.K)]
    got = run(S, buf, buf_len, offs, None, counts, counts, status=False)
    assert np.array_equal(got["cls"], intent)


# ---- the reply side: srpc_frames_pack_requests_mixed over response plans ----------------------

@pytest.mark.parametrize("foreign", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("name", ["calc", "kinds", "big", "sixteen"])
def test_ordered_reply_pack(name, foreign):
    """d_method = d_class, the index the decode wrote: the reply frames in
    arrival order, zero bytes at unknown frames, nothing at or past the total."""
    S = srv(name)
    for n in (1, 257, 4097):
        intent = method_vector(S.K, n, "uniform", foreign, seed=5)
        buf, offs, buf_len, elem = stream(S, intent)
        got = check(S, buf, buf_len, offs, intent, elem)
        out_cap = n * max(S.Fr)
        d_out, d_offs = empty(out_cap + GUARD), empty(4 * (n + 1) + GUARD)
        st = status_buf()
        st[8:] = 0xFF  # the pack does not reset the status: flags 0, no bad record
        rc = S.rep.pack(S.d_rep_cols, None, [NMAX] * S.K, got["d_cls"], got["d_index"], n, d_out, out_cap, d_offs, st)
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
        # a NULL status is accepted
        assert S.rep.pack(S.d_rep_cols, None, [NMAX] * S.K, got["d_cls"], got["d_index"], n, d_out, out_cap, None,
                          None) == 0
        assert np.array_equal(host(d_out, out_cap + GUARD), raw)


@pytest.mark.parametrize("name", ["calc", "kinds", "big", "sixteen"])
def test_round_trip(name):
    """Request frames from pack_requests_mixed, decoded by the server's call,
    give back the columns."""
    S = srv(name)
    for n in (257, 4097):
        method = method_vector(S.K, n, "uniform", 0.0, seed=6)
        nb = MixedFrames.index_bytes(n, S.K)
        d_method, d_index, d_counts = dev(method), empty(nb), empty(8 * (S.K + 1))
        assert MixedFrames.index(d_method, n, S.K, d_index, nb, d_counts) == 0
        out_cap = n * max(S.Fq)
        d_out, d_offs = empty(out_cap + GUARD), empty(4 * (n + 1))
        assert S.req.pack(S.d_req_cols, None, [NMAX] * S.K, d_method, d_index, n, d_out, out_cap, d_offs) == 0
        offs = host(d_offs, 4 * (n + 1), np.uint32)
        buf = host(d_out, int(offs[n])).copy()
        check(S, buf, int(offs[n]), offs[:n].copy(), method, cumcount(method))


# ---- refusals that need real plans -------------------------------------------------------------

def test_refusals_in_order():
    S = srv("calc")
    L = _lib.lib()
    INVALID, UNSUPPORTED, ALIGN, CAPACITY = (_lib.SRPC_E_INVALID, _lib.SRPC_E_UNSUPPORTED, _lib.SRPC_E_ALIGN,
                                             _lib.SRPC_E_CAPACITY)
    n = 300
    nb = MixedFrames.index_bytes(n, S.K)
    buf, offs, cls, idx, cnt = empty(64 * n), empty(4 * n + 16), empty(n), empty(nb + 16), empty(8 * (S.K + 1) + 16)
    cols = [[empty(8 * n + 16) for _ in p.schema.kinds] for p in S.req_plans]

    def call(mf=S.req, buf=buf.data_ptr(), offs=offs.data_ptr(), idx=idx.data_ptr(), nb=nb, cnt=cnt.data_ptr(),
             cols=cols, k=None):
        arr, h_first, h_cap = mf._args(cols, None, [n] * mf.k)
        return L.srpc_frames_unpack_requests_mixed(mf._plans, mf.k if k is None else k, buf, 64 * n, offs, n, arr,
                                                   h_first, h_cap, cls.data_ptr(), idx, nb, cnt, None, None)

    string = MixedFrames([GpuPacker(Schema("S", (("s", srpc_amd.STRING),)), b"\0\0\0\x08abcd")])
    short = MixedFrames([GpuPacker(srpc_amd.NUMBER, b"abc")])
    many = MixedFrames([GpuPacker(BIG, framed_request_prefix(BIG, f"B_servicer::m{j}")) for j in range(7)])
    one_col = [[empty(8 * n + 16)]]
    many_cols = [[empty(8 * n + 16) for _ in range(32)] for _ in range(7)]
    # an argument ahead of the plans, the plans ahead of alignment, alignment ahead of capacity
    assert call(mf=string, cols=one_col, k=17, buf=buf.data_ptr() + 1, nb=0) == INVALID
    assert call(mf=string, cols=one_col, buf=buf.data_ptr() + 1, nb=0) == UNSUPPORTED
    assert call(mf=short, cols=one_col, buf=buf.data_ptr() + 1, nb=0) == UNSUPPORTED
    assert call(mf=many, cols=many_cols, buf=buf.data_ptr() + 1, nb=0) == UNSUPPORTED  # 224 leaves
    assert call(buf=buf.data_ptr() + 8, nb=0) == ALIGN
    assert call(offs=offs.data_ptr() + 2, nb=0) == ALIGN
    assert call(idx=idx.data_ptr() + 4, nb=0) == ALIGN
    assert call(cnt=cnt.data_ptr() + 4, nb=0) == ALIGN
    skew = [list(c) for c in cols]
    skew[2][1] = skew[2][1][8:]
    assert call(cols=skew, nb=0) == ALIGN
    assert call(nb=nb - 1) == CAPACITY
    torch.cuda.synchronize()
    for t in [cls, idx, cnt] + [c for cc in cols for c in cc]:
        assert (t.cpu().numpy() == 0xA5).all()  # refused: nothing launched
