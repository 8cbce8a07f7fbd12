"""Every scratch-taking call on the scratch another call left behind.

In production no scratch is clean: batch_server runs srpc_gpu_unpack_var of one
schema and srpc_gpu_pack_var of another through one d_var_scratch, batch after
batch; one buffer serves classify, offsets and gather_var; batch_client shares
one d_vscratch between its mixed-var, mixed-AoS, legs and replies-var calls.
include/srpc_gpu.h promises that the contents on entry are arbitrary.  Here
each call under test (B) runs on a scratch that a different call (A) has just
used, or that holds 0x00, 0xFF or 0x5A (a u64 of 0x5A reads as a look-back
word with a published aggregate; 0xA5 and 0xFF as a published inclusive).

The protocol of a pair (tests/scratch_cases.py, proven on the CPU by
tests/test_scratch_cases_cpu.py):
1. one scratch S of max(need_A, need_B) + 16 bytes, 0xA5;
2. A runs on it;
3. S[:need_B] is read back: A must have changed it, else the pair is vacuous;
4. B runs on S, untouched, into fresh guarded 0xA5 outputs.
B's wire or columns, rec_offs, every str_offs, the chars up to str_offs[n],
the status, the guards and every byte of S behind need_B are compared with
oracle.pack / oracle.unpack (an inexact index: the documented model of
tests/test_gpu_parity.py); the frame calls with the host models of their own
test modules.  No expected value comes from a GPU call.  Sensitivity is not
shown by removing a reset (a stale look-back word is a wrong output base: an
out-of-bounds store), but by step 3 and by what each group's docstring says
the path reads before it writes.

Pair -> host branch (scratch_cases names every pair `<call>-after-<A>`; the
branch is the pair's `branch` field, checked against the batch's average
record bytes and string count on the CPU):

  pack-*-vkNone, band lt20 / 20-40 / 40-200     rt rpl=2 / rt rpl=1 / rt loop
  pack-*1s*-vk0, pack-long1s*                    k_pack_short_records<true> + k_pack_var<true>
    pack-all-short-after-long-flags              ... no wave long after an A that set long flags
    pack-some-long-after-all-short               ... the reverse
  pack-*{2,3}s*-vk0, pack-wide*-vk0, pack-long*  launch_scan + k_pack_var<false> (no short-records pass)
  unpack1-exact-*                                k_reset_walk1 + k_unpack_var_rt<true>, gated pass idle
  unpack1-inexact-*                              ... + gated k_unpack_var_rt<false> (bad set)
  unpackN-lookback-*                             k_zero_u64 + k_unpack_var_rt<false>; n = 16 641: 65 tiles + 1,
                                                 the per-64-tile second-level words
  tiled-right-* / tiled-<wrong>-*                k_unpack_var_rt<false> with a table / + gated look-back pass
  walk1-*lt20* / walk1-*20-40*                   k_unpack_var_walk<true, 2 / 1> + k_unpack_str1_tail
  walk1-*40-200*-vk0 / walk1-long*               walk + k_scan1 + k_unpack_var_chars
  walkN-*                                        walk + launch_scan + k_unpack_var_chars_multi
  test_server_sequence                           unpack(request): walk + scans; pack(response):
                                                 k_pack_short_records<true> + k_pack_var<true>; unpack again
  test_stalled_retry_on_the_same_scratch         STALLED, then the retry on that scratch
  test_server_frames_on_used_scratch             srpc_frames_classify -> _gather_var -> _offsets (k_zero_counts)
  test_client_frames_on_used_scratch             _unpack_replies_var, _mixed_var / _mixed_legs pack and decode,
                                                 _mixed_aos decode, _unpack_requests_mixed_var / _aos

The several-string scan WITH the short-records pass has no pair: the host
takes it when fixed_bytes + 32 * nstrings <= 64, and two strings' length
words alone make 16 + 64 = 80, so no schema reaches it in this build.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from srpc_amd import FrameClassifier, GpuPacker, Schema, SRPC_STATUS_BOUNDS, framed_request_prefix

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests import scratch_cases as sc  # noqa: E402
from tests import test_gpu_mixed as gm  # noqa: E402
from tests import test_gpu_replies as rp  # noqa: E402
from tests import test_gpu_replies_aos as rpa  # noqa: E402
from tests import test_gpu_requests_mixed as rq  # noqa: E402
from tests import test_gpu_requests_mixed_legs as rql  # noqa: E402
from tests import var_cases as vc  # noqa: E402
from tests.test_gpu_geometry import _assert_packed, _assert_unpacked, _pack_guarded, _unpack_guarded  # noqa: E402
from tests.test_gpu_parity import _model_single_string, dev, empty, host, read_status, status_buf  # noqa: E402

FRESH = 0xA5
STALLED = 4  # SRPC_STATUS_STALLED (include/srpc_gpu.h)


# ---- batches on the host and on the device, made once -------------------------------------

@functools.lru_cache(maxsize=None)
def H(b, prefix=b""):
    kinds, cols, offs = sc.make(b)
    wire = oracle.pack(kinds, cols, b.n, prefix, list(offs))
    rec = vc.rec_offsets(kinds, offs, b.n, len(prefix))
    assert int(rec[b.n]) == len(wire)
    rc, ocols, ooffs, consumed, _ = oracle.unpack(kinds, wire, b.n, prefix)
    assert rc == oracle.ORC_OK and consumed == len(wire)
    for a in list(cols) + [o for o in offs if o is not None] + [rec]:
        a.setflags(write=False)
    return SimpleNamespace(kinds=kinds, cols=cols, offs=offs, n=b.n, wire=wire, rec=rec, ocols=ocols, ooffs=ooffs,
                           prefix=prefix)


@functools.lru_cache(maxsize=None)
def D(b, prefix=b""):
    h = H(b, prefix)
    return SimpleNamespace(cols=[dev(c) for c in h.cols],
                           offs=[None if o is None else dev(np.ascontiguousarray(o, np.uint64)) for o in h.offs],
                           wire=dev(np.frombuffer(h.wire, np.uint8)), rec=dev(h.rec))


@functools.lru_cache(maxsize=None)
def packer(kinds, vk):
    p = GpuPacker(Schema("S", tuple((f"f{i}", k) for i, k in enumerate(kinds))))
    if vk is not None:
        p.tune(var_kernel=vk)
    return p


def plan_of(x):
    return packer(tuple(H(x.batch).kinds), x.vk)


def host_table(h):
    """The tile table from the batch's offsets, on the host: the chars of each
    string field before every 256-record tile."""
    at = np.minimum(np.arange(-(-h.n // 256) + 1) * 256, h.n)
    return np.stack([o[at] - o[0] for o in h.offs if o is not None], axis=1).reshape(-1).astype(np.uint64)


def table_for(h, how):
    t = host_table(h)
    return dev(t if how == "right" else sc.wrong_table(t, how, len(sc.str_fields(h.kinds))))


def need_of(x):
    """Scratch bytes of a predecessor or a call (a fill needs none)."""
    kind = getattr(x, "kind", None) or x.op
    if kind == "fill":
        return 0
    h = H(x.batch)
    cap = sc.bounds_cap(len(h.wire)) if kind == "pack_bounds" else len(h.wire)
    return plan_of(x).var_scratch_bytes(h.n, cap)


# ---- the protocol ------------------------------------------------------------------------

def run_pred(S, a):
    """Step 2: the predecessor, on S.  Its outputs go to throwaway buffers of
    the sizes the API asks for; only what it leaves in S matters."""
    if a.kind == "fill":
        S.fill_(a.arg)
        return
    h, d, p = H(a.batch), D(a.batch), plan_of(a)
    sb = need_of(a)
    st = status_buf()
    if a.kind in ("pack", "pack_bounds"):
        cap = sc.bounds_cap(len(h.wire)) if a.kind == "pack_bounds" else len(h.wire)
        p.pack_var(d.cols, d.offs, h.n, empty(len(h.wire) + 16), cap, empty(8 * (h.n + 1)), S, sb, st)
        assert (read_status(st)[0] == SRPC_STATUS_BOUNDS) == (a.kind == "pack_bounds")
        return
    L = len(h.wire)
    outs = [empty(L + 16) if k == oracle.STRING else empty(h.n * oracle.KIND_SIZE[k] + 16) for k in h.kinds]
    so = [empty(8 * (h.n + 1)) if k == oracle.STRING else None for k in h.kinds]
    wire, rec = d.wire, d.rec
    if a.kind == "unpack_inexact":
        rec = dev(sc.inexact_index(h.rec, h.n))
    elif a.kind == "unpack_bounds":
        wire = dev(np.frombuffer(sc.bounds_wire(h.kinds, h.wire, h.rec, h.n)[0], np.uint8))
    if a.kind == "tiled":
        p.unpack_var_tiled(wire, L, h.n, rec, table_for(h, a.arg), outs, so, S, sb, st)
    else:
        p.unpack_var(wire, L, h.n, rec, outs, so, S, sb, st)
    flags = read_status(st)[0]
    assert (flags & SRPC_STATUS_BOUNDS != 0) == (a.kind in ("unpack_inexact", "unpack_bounds")), (a, flags)


def run_call(S, b, what):
    """Step 4: the call under test on S, checked against the oracle."""
    h, d, p = H(b.batch), D(b.batch), plan_of(b)
    if b.op == "pack":
        g, st = _pack_guarded(p, d.cols, d.offs, h.n, len(h.wire), len(h.wire), scratch=S)
        _assert_packed(g, st, h.wire, h.rec, h.n, len(h.wire), what)
        return
    if b.op == "unpack_inexact":
        idx = sc.inexact_index(h.rec, h.n)
        cols, offs, st = _unpack_guarded(p, h.kinds, d.wire, len(h.wire), h.n, dev(idx), scratch=S)
        f = sc.str_fields(h.kinds)[0]
        want_offs, want_chars = _model_single_string(h.kinds, h.wire, h.n, idx, b"")
        assert st == (SRPC_STATUS_BOUNDS, h.n // 3 - 1), what
        assert np.array_equal(offs[f], want_offs) and cols[f].tobytes() == want_chars, what
        keep = np.ones(h.n, bool)
        keep[h.n // 3 - 1:h.n // 3 + 1] = False  # the two records the moved boundary touches
        for g, k in enumerate(h.kinds):
            if k != oracle.STRING:
                assert np.array_equal(cols[g].view(oracle.KIND_DTYPE[k])[keep], h.ocols[g][keep]), (what, g)
        return
    table = table_for(h, b.arg) if b.op == "tiled" else None
    got = _unpack_guarded(p, h.kinds, d.wire, len(h.wire), h.n, d.rec, table, scratch=S)
    _assert_unpacked(h.kinds, got, (h.ocols, h.ooffs), what)


def dirtied(S, need_b, before):
    """Step 3: the predecessor changed at least one byte of S[:need_b]."""
    torch.cuda.synchronize()
    return bool((S[:need_b] != before).any())


def run_pair(pair):
    need_b = need_of(pair.b)
    S = empty(max(need_of(pair.a), need_b) + 16)
    run_pred(S, pair.a)
    assert dirtied(S, need_b, FRESH), f"{pair.name}: the predecessor left the call's scratch untouched"
    behind = S[need_b:].clone()
    run_call(S, pair.b, pair.name)
    assert torch.equal(S[need_b:], behind), f"{pair.name}: wrote behind the scratch it asked for"


# ---- srpc_gpu_pack_var ---------------------------------------------------------------------

@pytest.mark.parametrize("pair", sc.pack_pairs(), ids=lambda p: p.name)
def test_pack_var_on_used_scratch(pair):
    """The record tiles (var_kernel default, records under ~240 bytes) take no
    scratch at all.  The walk reads before it writes: the kLongFlags
    some_long words (k_pack_var<true> skips the batch when none is set: a
    stale flag costs a second pass, a missing one the whole wire), the tile
    starts tile_first[t] of every 4 KiB wire tile, and the scan partials."""
    run_pair(pair)


# ---- srpc_gpu_unpack_var / _unpack_var_tiled -------------------------------------------------

@pytest.mark.parametrize("pair", sc.unpack_pairs(), ids=lambda p: p.name)
def test_unpack_var_on_used_scratch(pair):
    """Read before written, per path.  Record tiles: the tile ticket, the
    look-back words of every tile and 64-tile block (top two bits: aggregate /
    inclusive published -- a stale published word is a wrong chars base), the
    `bad` word that gates the second pass.  Single-string walk: `bad` and its
    255 long-wave flags, tile_long[t] of every chars tile, tile_first, the
    look-back words of k_scan1 / k_unpack_str1_tail.  Several strings, walk:
    lens / spos of every record, the scan partials, tile_first per field."""
    run_pair(pair)


def test_server_sequence():
    """batch_server's order on its one d_var_scratch, sized as it sizes it
    (the larger need of the request and the response plan at the largest
    batch and capacity): unpack_var(request, batch 1), pack_var(response,
    batch 1), unpack_var(request, batch 2); every step checked, every call
    on the one buffer, larger than the call asks for.  Requests and
    responses are long records (over 255 bytes before their envelopes): the
    unpack walks (lengths, positions and partials from the first byte on)
    and the pack is the one that uses the scratch, so each step lands on the
    words the next one reads.  The record tiles of a 40-200 byte request
    batch keep their few words behind the lens / spos regions, past the end
    of what the pack uses: such a sequence would not test the pack."""
    r1, r2 = sc.SERVER["request"]
    rs = sc.SERVER["response"]
    max_n = sc.SERVER["max_n"]
    req = GpuPacker.for_request(Schema("Req", tuple((f"f{i}", k) for i, k in enumerate(H(r1).kinds))), "Svc_servicer::m")
    resp = GpuPacker.for_response(Schema("Resp", tuple((f"f{i}", k) for i, k in enumerate(H(rs).kinds))))
    h1, h2, hr = H(r1, req.prefix), H(r2, req.prefix), H(rs, resp.prefix)
    d1, d2, dr = D(r1, req.prefix), D(r2, req.prefix), D(rs, resp.prefix)
    cap_in = max(len(h1.wire), len(h2.wire))
    cap_out = len(hr.wire) + 16
    sb = max(req.var_scratch_bytes(max_n, cap_in), resp.var_scratch_bytes(max_n, cap_out))
    S = empty(sb + 16)

    def unpack(h, d, step):
        got = _unpack_guarded(req, h.kinds, d.wire, len(h.wire), h.n, d.rec, scratch=S)
        _assert_unpacked(h.kinds, got, (h.ocols, h.ooffs), step)

    unpack(h1, d1, "request batch 1")
    assert dirtied(S, resp.var_scratch_bytes(hr.n, cap_out), FRESH)
    snap = S.clone()
    g, st = _pack_guarded(resp, dr.cols, dr.offs, hr.n, cap_out, cap_out, scratch=S)
    _assert_packed(g, st, hr.wire, hr.rec, hr.n, cap_out, "response batch 1")
    need2 = req.var_scratch_bytes(h2.n, len(h2.wire))
    assert dirtied(S, need2, snap[:need2]), "the response pack left the next unpack's scratch untouched"
    unpack(h2, d2, "request batch 2")
    assert bool((S[sb:] == FRESH).all()), "wrote behind the scratch"


def test_stalled_retry_on_the_same_scratch():
    """A several-string look-back under a spin budget of one poll (tiles give
    up and report STALLED, as tests/test_gpu_tiled.py provokes it), then the
    caller's retry on the scratch it has -- the stalled call's half-published
    look-back words, tickets and all.  The retry must be exact.  Before
    both, another batch's look-back dirties the scratch."""
    from srpc_amd import _lib
    hook = _lib.lib().srpc_debug_var_spin_limit
    hook.argtypes, hook.restype = [ctypes.c_uint32], ctypes.c_int
    b = sc.STALLED
    h, d = H(b), D(b)
    p = packer(tuple(h.kinds), None)
    a = sc.Pred("unpack", sc.near(b), None, None)
    sb = p.var_scratch_bytes(h.n, len(h.wire))
    S = empty(max(sb, need_of(a)) + 16)
    run_pred(S, a)
    assert dirtied(S, sb, FRESH)
    before = S[:sb].clone()
    assert hook(1) == 0
    try:
        cols, offs, st = _unpack_guarded(p, h.kinds, d.wire, len(h.wire), h.n, d.rec, scratch=S)
    finally:
        assert hook(0) == 0
    assert st[0] & ~STALLED == 0, st
    if not st[0] & STALLED:  # no tile had to wait: the outputs are exact
        _assert_unpacked(h.kinds, (cols, offs, st), (h.ocols, h.ooffs), "under the budget")
    assert dirtied(S, sb, before), "the stalled call left the scratch as it found it"
    behind = S[sb:].clone()
    got = _unpack_guarded(p, h.kinds, d.wire, len(h.wire), h.n, d.rec, scratch=S)  # the retry, once
    _assert_unpacked(h.kinds, got, (h.ocols, h.ooffs), "the retry")
    assert torch.equal(S[sb:], behind)


# ---- frames, server side: classify -> gather_var -> offsets on one scratch -------------------

from tests.test_gpu_frames import METHODS, UNKNOWN, VAR_METHODS, _mixed_var_frames  # noqa: E402

# (frames, foreign share, string share, longest string): A mostly string frames, B another mix
FRAMES_A = (50_001, 0.02, 0.85, 40)
FRAMES_B = (777, 0.2, 0.3, 90)


@functools.lru_cache(maxsize=None)
def frame_batch(spec):
    n, foreign, var_frac, maxlen = spec
    buf, offs, want, _ = _mixed_var_frames(n, np.random.default_rng([n, maxlen]), foreign, maxlen, var_frac)
    return SimpleNamespace(n=n, buf=buf, offs=offs, want=want, d_buf=dev(np.frombuffer(buf, np.uint8)), d_offs=dev(offs))


@functools.lru_cache(maxsize=None)
def frame_classifier():
    fixed = [(GpuPacker(s, framed_request_prefix(s, m)), rb) for s, m, rb in METHODS]
    var = [(GpuPacker.for_request(s, m), 0) for s, m in VAR_METHODS]
    return FrameClassifier(fixed + var)


def guard_ok(t, nbytes):
    return bool((t[nbytes:nbytes + 16] == FRESH).all())


def serve_frames(fc, F, S, check):
    """The server's three scratch-taking calls on S in its order.  With
    `check`, every output against the host model of the dispatch
    (tests/test_gpu_frames.py): a frame's class is what its bytes say, a
    bucket holds its frames, a gathered record is its frame's payload, a
    frame's reply starts where the replies of the frames before it end."""
    n, K, KT = F.n, len(METHODS), len(METHODS) + len(VAR_METHODS)
    sb = fc.scratch_bytes(n)
    d_cls, d_idx = empty(n + 16), empty(4 * KT * n + 16)
    d_counts, d_out_off = empty(8 * (KT + 2) + 16), empty(8 * (n + 1) + 16)
    fc.classify(F.d_buf, len(F.buf), F.d_offs, n, d_cls, d_idx, d_counts, d_out_off, S, sb)
    counts = host(d_counts, 8 * (KT + 2), np.uint64)
    idx = host(d_idx, 4 * KT * n, np.uint32).reshape(KT, n)
    if check:
        assert np.array_equal(host(d_cls, n), F.want), "d_cls"
        assert [int(c) for c in counts[:KT]] == [int((F.want == k).sum()) for k in range(KT)], "counts"
        assert int(counts[KT + 1]) == int((F.want == UNKNOWN).sum()), "unknown count"
        for k in range(KT):
            nk = int((F.want == k).sum())
            assert np.array_equal(np.sort(idx[k, :nk]), np.flatnonzero(F.want == k).astype(np.uint32)), ("bucket", k)
        assert guard_ok(d_cls, n) and guard_ok(d_idx, 4 * KT * n) and guard_ok(d_counts, 8 * (KT + 2))
    bnp = np.frombuffer(F.buf, np.uint8)
    ends = np.append(F.offs[1:], len(F.buf)).astype(np.int64)
    per = np.zeros(n, np.uint64)  # reply bytes per frame, in arrival order
    for k in range(K):
        per[F.want == k] = METHODS[k][2]
    var_rec = [None] * KT
    rng = np.random.default_rng(n)
    for j in range(len(VAR_METHODS)):
        k = K + j
        nk = int((F.want == k).sum())
        if check:
            assert nk == int(counts[k]) and nk > 0
        frames = idx[k, :nk].astype(np.int64)
        payloads = [bytes(bnp[F.offs[f] + 4:ends[f]]) for f in frames]
        total = sum(len(p) for p in payloads)
        g, rec = empty(total + 16), empty(8 * (nk + 1) + 16)
        FrameClassifier.gather_var(F.d_buf, F.d_offs, d_idx[4 * k * n:], nk, g, rec, S, fc.scratch_bytes(nk))
        if check:
            want_rec = np.zeros(nk + 1, np.uint64)
            want_rec[1:] = np.cumsum([len(p) for p in payloads])
            assert np.array_equal(host(rec, 8 * (nk + 1), np.uint64), want_rec), ("record index", k)
            assert host(g, total).tobytes() == b"".join(payloads), ("gathered payloads", k)
            assert guard_ok(g, total) and guard_ok(rec, 8 * (nk + 1))
        # the replies of this bucket: any sizes will do for the offsets (a host-made response index)
        size = rng.integers(17, 300, nk).astype(np.uint64)
        rr = np.zeros(nk + 1, np.uint64)
        rr[1:] = np.cumsum(size)
        var_rec[k] = dev(rr)
        per[frames] = size + np.uint64(4)  # BE32 + the reply record
    total_d = empty(32)
    fc.offsets(d_cls, n, d_idx, d_counts, var_rec, d_out_off, total_d, S, sb)
    if check:
        want_off = np.zeros(n + 1, np.uint64)
        want_off[1:] = np.cumsum(per)
        assert np.array_equal(host(d_out_off, 8 * (n + 1), np.uint64), want_off), "out_off"
        assert int(host(total_d, 8, np.uint64)[0]) == int(want_off[n]), "total"
        assert guard_ok(d_out_off, 8 * (n + 1)) and guard_ok(total_d, 8)
    return sb


@pytest.mark.parametrize("pred", ["larger-batch", "fill00", "fillff", "fill5a"])
def test_server_frames_on_used_scratch(pred):
    """srpc_frames_classify, _gather_var and _offsets keep a u32 per frame in
    the scratch (its reply bytes, its payload length) and behind them the
    block totals of their scan; nothing there is zeroed (k_zero_counts clears
    d_counts), so every frame's word -- an UNKNOWN frame's 0 too -- and every
    block total must be written before the scan reads it.  777 frames of one
    mix after 50 001 mostly-string frames through the same three calls, and
    after each fill."""
    fc = frame_classifier()
    B = frame_batch(FRAMES_B)
    sb_b = fc.scratch_bytes(B.n)
    if pred == "larger-batch":
        A = frame_batch(FRAMES_A)
        strings = lambda F: float(np.mean((F.want >= len(METHODS)) & (F.want != UNKNOWN)))  # noqa: E731
        assert strings(A) > 0.8 and strings(B) < 0.4 and A.n > B.n  # mostly string frames, then another mix
        S = empty(max(fc.scratch_bytes(A.n), sb_b) + 16)
        serve_frames(fc, A, S, check=False)
    else:
        S = empty(sb_b + 16)
        S.fill_(int(pred[4:], 16))
    assert dirtied(S, sb_b, FRESH)
    behind = S[sb_b:].clone()
    serve_frames(fc, B, S, check=True)
    assert torch.equal(S[sb_b:], behind), "wrote behind the scratch it asked for"


# ---- frames, client side: one d_vscratch for every call family ---------------------------------

from tests import test_gpu_mixed_aos as ma  # noqa: E402
from tests import test_gpu_mixed_legs as lg  # noqa: E402
from tests import test_gpu_mixed_var as mv  # noqa: E402
from tests import test_gpu_replies_var as rv  # noqa: E402
from tests import test_gpu_requests_mixed_aos as rqa  # noqa: E402
from tests import test_gpu_requests_mixed_var as rqv  # noqa: E402
from tests.test_gpu_mixed import NMAX, cumcount, reply_stream  # noqa: E402

# the two batches of every family: the predecessor's (more calls, another method
# mix, another length regime or layout) and the call's own
SHAPES = {
    "A": dict(n=4099, which="runs", order="runs", regime="short", rv="mix", aos=("kinds", "odd")),
    "B": dict(n=513, which="uniform", order="uniform", regime="mid", rv="multiple", aos=("calc", "natural")),
}
LEGS = ("calc_text", "natural", "mixed")


def _mv_batch(sh):
    return mv.batch("calc_echo", sh["n"], sh["which"], sh["regime"])


def _codes(sh):
    return np.random.default_rng(sh["n"]).integers(0, 3, sh["n"])


def _aos_reply(sh):
    side = ma.side(*sh["aos"], True)
    return side, ma.order(sh["order"], sh["n"], side.R.K, side.mf.tile)


def _aos_request(sh):
    return rqa.lay_for(*sh["aos"])


def client_need(kind, sh):
    n = sh["n"]
    if kind == "mixed_var_pack":
        return _mv_batch(sh).P.req.scratch_bytes(n)
    if kind in ("mixed_var_decode", ):
        return _mv_batch(sh).P.rep.scratch_bytes(n)
    if kind == "requests_mixed_var":
        return _mv_batch(sh).P.req.scratch_bytes(n)
    if kind == "legs_pack":
        return lg.legs(*LEGS).req.scratch_bytes(n)
    if kind == "legs_decode":
        return lg.legs(*LEGS).rep.scratch_bytes(n)
    if kind == "replies_var":
        return rv.packer(sh["rv"], 2).replies_var_scratch_bytes(n)
    if kind == "mixed_aos_decode":
        return _aos_reply(sh)[0].mf.scratch_bytes
    if kind == "requests_mixed_aos":
        return _aos_request(sh).mf.scratch_bytes
    raise KeyError(kind)


def client_call(kind, sh, S):
    """One call of a family on S, checked in full by its own module's helpers
    (the oracle's frames, the header's per-frame tables restated on the host)."""
    n = sh["n"]
    if kind == "mixed_var_pack":
        B = _mv_batch(sh)
        mv.check_pack(B, mv.run_pack(B, scratch=S))
    elif kind == "mixed_var_decode":
        B = _mv_batch(sh)
        mv.decode_and_check(B, B.rep_frames(_codes(sh)), scratch=S)
    elif kind == "requests_mixed_var":
        B = _mv_batch(sh)
        frames, intent, src = rqv.stream(B, 0.1)
        rqv.check(B.P, B.req, frames, intent, src, scratch=S)
    elif kind == "legs_pack":
        B = _mv_batch(sh)
        lg.check_pack(B, lg.run_pack_legs(lg.legs(*LEGS), B, scratch=S))
    elif kind == "legs_decode":
        B = _mv_batch(sh)
        lg.decode_and_check(lg.legs(*LEGS), B, B.rep_frames(_codes(sh)), scratch=S)
    elif kind == "replies_var":
        rv.decode_and_check(sh["rv"], n, rv.make_lens(sh["rv"], n, "0-40"), _codes(sh), scratch=S)
    elif kind == "mixed_aos_decode":
        side, method = _aos_reply(sh)
        first = [3 * k + 1 for k in range(side.R.K)]
        elem = np.minimum(np.array(first)[method] + cumcount(method), NMAX - 1)
        buf, offs = reply_stream(side.R, method, elem, _codes(sh))
        ma.check(side, method, buf, len(buf), offs, n, first=first, columns=False, scratch=S)
    elif kind == "requests_mixed_aos":
        L = _aos_request(sh)
        intent = rqa.intent_of(sh["aos"][0], sh["order"], n, L.T, foreign=0.1)
        buf, offs, buf_len, elem = rqa.stream(L.S, intent)
        first = [3 * k + 1 for k in range(L.S.K)]
        rqa.check(L, buf, buf_len, offs, intent, elem, first=first, others=False, scratch=S)
    else:
        raise KeyError(kind)


CLIENT_KINDS = ["replies_var", "mixed_var_pack", "mixed_var_decode", "legs_pack", "legs_decode", "mixed_aos_decode",
                "requests_mixed_var", "requests_mixed_aos"]
# the call of another family that ran on the scratch before
OTHER_FAMILY = {"replies_var": "mixed_var_pack", "mixed_var_pack": "mixed_aos_decode", "mixed_var_decode": "legs_pack",
                "legs_pack": "replies_var", "legs_decode": "replies_var", "mixed_aos_decode": "mixed_var_decode",
                "requests_mixed_var": "requests_mixed_aos", "requests_mixed_aos": "requests_mixed_var"}


@pytest.mark.parametrize("after", ["same-call-larger", "other-family"])
@pytest.mark.parametrize("kind", CLIENT_KINDS)
def test_client_frames_on_used_scratch(kind, after):
    """The calls that share batch_client's d_vscratch, on one scratch sized
    for the largest need of all of them at the larger batch (as
    ensure_vscratch sizes it).  What they keep there and read back: the
    uploaded description of the plans (columns, offsets arrays, struct
    layouts: every later kernel reads it from the scratch), the granule
    totals of the pack's size scan, per string and frame the length and the
    chars' stream offset the parse leaves for the slot scan and the copy, the
    slot scan's partials; the reply decode of one string plan its lens / srcs
    per frame and its scan's words.  Each call runs after the same call on
    4 099 calls of another method mix and length regime, and after a call of
    another family."""
    need_b = client_need(kind, SHAPES["B"])
    pred = kind if after == "same-call-larger" else OTHER_FAMILY[kind]
    S = empty(max(client_need(k, sh) for k in CLIENT_KINDS for sh in SHAPES.values()) + 16)
    client_call(pred, SHAPES["A"], S)
    assert dirtied(S, need_b, FRESH), f"{pred} left the scratch of {kind} untouched"
    client_call(kind, SHAPES["B"], S)
    assert bool((S[-16:] == FRESH).all())


# ---- one d_status for every decode: the reset all of them share ------------------------------------

NONE = 2**64 - 1


def _status_site(site):
    """-> (module whose runner makes the status, run(cut) -> (flags, first bad)):
    one decode of a small all-full batch.  With `cut` a reply decode's buffer is
    that many bytes short (the last frame ends past it) and a request decode's
    last plan has one element too few (its last frame has none): BOUNDS."""
    n = 300
    codes = np.zeros(n, np.int64)

    def status_of(got):
        return got["flags"], got["bad"]
    if site in ("requests_mixed", "requests_mixed_aos"):
        L = rqa.lay_for("calc", "natural")
        intent = rqa.intent_of("calc", "uniform", n, L.T)
        buf, offs, buf_len, elem = rqa.stream(L.S, intent)
        counts = [int((intent == k).sum()) for k in range(L.S.K)]
        assert counts[-1] > 1
        cap = lambda cut: counts[:-1] + [counts[-1] - bool(cut)]  # noqa: E731
        if site == "requests_mixed":
            return rq, lambda cut: status_of(rq.check(L.S, buf, buf_len, offs, intent, elem, cap=cap(cut), alloc=counts))
        return rqa, lambda cut: status_of(rqa.check(L, buf, buf_len, offs, intent, elem, cap=cap(cut), others=False))
    if site in ("requests_mixed_var", "requests_mixed_legs"):
        B = mv.batch("calc_echo", n, "uniform", "short")
        if site == "requests_mixed_var":
            frames, intent, src = rqv.stream(B)
            cap = lambda cut: B.counts[:-1] + [B.counts[-1] - bool(cut)]  # noqa: E731
            return rqv, lambda cut: status_of(rqv.check(B.P, B.req, frames, intent, src, cap=cap(cut), alloc=B.counts))
        S = rql.side("calc_echo", "natural", "mixed")
        frames, intent, src = rql.stream_of(S, B, B.method)
        full = [(rql.FRONT if S.rec[k] else 0) + B.counts[k] for k in range(S.K)]
        assert not S.rec[-1]
        return rql, lambda cut: status_of(rql.check(S, B.req, frames, intent, src, cap=full[:-1] + [full[-1] - bool(cut)]))
    if site == "mixed_index":
        return gm, lambda cut: gm.build_index(np.array([0, 1, 9 if cut else 2, 3], np.uint8), 4)[3:]
    if site in ("replies_mixed", "replies_mixed_aos"):
        side, method = _aos_reply(dict(SHAPES["B"], n=n))
        buf, offs = reply_stream(side.R, method, cumcount(method), codes)
        index = gm.build_index(method, side.R.K)[:2]  # ahead of the decode: the index resets a status of its own
        if site == "replies_mixed":
            return gm, lambda cut: gm.run_unpack(side.R, method, buf, len(buf) - cut, offs, n, index=index)[3:]
        return ma, lambda cut: ma.run_unpack_aos(side, method, buf, len(buf) - cut, offs, n, index=index)[3:5]
    if site in ("replies_mixed_var", "replies_mixed_legs"):
        B = mv.batch("calc_echo", n, "uniform", "short")
        buf, offs = mv.joined(B.rep_frames(codes))
        if site == "replies_mixed_var":
            return mv, lambda cut: mv.run_unpack(B, mv.Outs(B), buf, len(buf) - cut, offs[:n], n)[3:]
        L = lg.legs(*LEGS)
        return lg, lambda cut: lg.run_unpack_legs(L, B, lg.LegOuts(L, B), buf, len(buf) - cut, offs[:n], n)[3:]
    if site in ("replies", "replies_aos"):
        buf, offs = rp.stream("number", n, codes)
        p = rp.packer("number")
        if site == "replies":
            return rp, lambda cut: rp.run(p, buf, len(buf) - cut, offs, n)[3:]
        return rpa, lambda cut: rpa.run_aos(p, "number", "natural", buf, len(buf) - cut, offs, n)[3:]
    assert site == "replies_var"
    lens = rv.make_lens("mix", n, "0-40")
    buf, offs = rv.stream("mix", n, lens, codes)
    p = rv.packer("mix", 2)

    def run(cut):
        args = rv.run(p, buf, len(buf) - cut, offs, n, call=False)
        p.unpack_replies_var(*args)
        return read_status(args[-1])
    return rv, run


STATUS_SITES = ["mixed_index", "replies_mixed", "replies_mixed_aos", "replies_mixed_var", "replies_mixed_legs", "replies",
                "replies_var", "replies_aos", "requests_mixed", "requests_mixed_aos", "requests_mixed_var",
                "requests_mixed_legs"]


@pytest.mark.parametrize("site", STATUS_SITES)
def test_decode_resets_the_status_a_flagged_decode_left(site, monkeypatch):
    """Every decode begins by resetting *d_status, all through one launch
    (status_reset_launch).  A decode that flags a bad frame, then a clean one
    on the same d_status: flags 0, no bad record.  (The request decodes'
    runners also fill the status with 0x5A before every call.)"""
    module, run = _status_site(site)
    shared = status_buf()
    monkeypatch.setattr(module, "status_buf", lambda: shared)
    flags, first = run(2)
    print(f"{site}: flagged run left flags={flags} first={first}")
    assert flags == SRPC_STATUS_BOUNDS and first != NONE and read_status(shared) == (flags, first)
    assert run(0) == (0, NONE) and read_status(shared) == (0, NONE)
