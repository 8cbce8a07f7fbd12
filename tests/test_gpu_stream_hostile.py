"""The index-free stream decode (srpc_gpu_unpack_var_stream, sdx.hip) on the
inputs a peer would choose: hostile streams, far entries, overflowing exit
slots, odd pointers and stale scratch.  tests/test_gpu_stream.py covers clean
streams; here every call goes through a guarded runner (`run`):
- the wire, rec_offs, every column, every str_offs and the scratch are slices
  of sentinel-filled tensors, a chars column is as long as the oracle's char
  count rounded up to 16 and the scratch is exactly var_stream_scratch_bytes,
  and after each call every byte outside the slices still holds the sentinel;
- the error contract is checked in full (`verify`): the status, everything
  before the first bad record byte-exact, rec_offs[err] the bad record's
  start (where the oracle's cursor was when it began that record; on a prefix
  mismatch that is the oracle's consumed offset itself), rec_offs[err+1..n] ==
  wire_len and str_offs[f][err+1..n] == str_offs[f][err];
- bad records sit where the decoder changes gear (tests/streams.py
  hostile_places: first and last record, first and last block of scan group
  1, blocks 4095-4097 around the in-order scan's 64-group reload, length
  fields across a block edge and across the end of a staged margin); every
  cut is run with the valid continuation and with 0xA5 behind wire_len, and
  the two calls' outputs must be the same bytes;
- nested_stream: blocks entered by records that started two or more blocks
  back, every block of which speculates a chain that parses and is wrong;
  fan_stream: ~1000 live exits into a block with 255 exit slots;
- the wire at 1, 3, 4, 8 and 15 bytes past a 256-byte boundary (the API asks
  no wire alignment), a chars column 16 bytes past one; misaligned chars and
  rec_offs pointers refused; scratch pre-filled with 0x00, 0xFF and another
  call's leftovers.
What each generator guarantees is checked on the CPU (tests/test_streams_cpu.py).
Every test of the decode runs in the four table modes of tests/test_gpu_stream.py.
"""
import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, Schema, SrpcError

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests import streams  # noqa: E402
from tests.test_gpu_geometry import Checked  # noqa: E402
from tests.test_gpu_parity import dev, status_buf  # noqa: E402
from tests.test_gpu_stream import RES_MISS, RES_OVER, RES_REPAIR, path  # noqa: E402,F401
from tests.test_gpu_sweep import SENTINEL  # noqa: E402

STATUS_OF = {"bounds": srpc_amd.SRPC_STATUS_BOUNDS, "prefix": srpc_amd.SRPC_STATUS_PREFIX}
NO_BAD = 2**64 - 1


def r16(x):
    return (x + 15) // 16 * 16


class Base:
    """One clean stream on the device (guarded), its packer, and the oracle's
    decode of it on the device: what every record before a bad one must equal."""

    def __init__(self, kinds, prefix, wire, n, front=0):
        self.kinds, self.prefix, self.n = list(kinds), prefix, n
        self.wire = np.asarray(wire, np.uint8)
        self.W = self.wire.size
        rc, ocols, ooffs, consumed, _ = oracle.unpack(self.kinds, self.wire.tobytes(), n, prefix)
        assert rc == oracle.ORC_OK and consumed == self.W
        self.ooffs = ooffs
        self.rec = streams.record_starts(self.kinds, ooffs, n, len(prefix))
        self.p = GpuPacker(Schema("S", tuple((f"f{i}", k) for i, k in enumerate(self.kinds))), prefix)
        assert self.p.prefix == prefix
        self.front = front                       # the wire starts this far past a 256-byte boundary
        self.gw = Checked([front + self.W])
        self.dwire = self.gw.slices[0][front:]
        self.clean = dev(self.wire)
        self.dwire.copy_(self.clean[:self.W])
        self.xrec = dev(self.rec)
        self.xcols = [dev(c) for c in ocols]
        self.xoffs = [None if o is None else dev(o) for o in ooffs]

    def chars(self, same, partial=None):
        """The oracle's char count per field after `same` clean records (and
        what it read of the next, bad, one)."""
        return [0 if o is None else int(o[same]) + (partial[f] if partial else 0) for f, o in enumerate(self.ooffs)]


class Out:
    pass


def pads_clean(g, what):
    """Every byte outside g's slices still holds the sentinel; else say where."""
    if g.pads_clean():
        return
    h = g.t.cpu().numpy()
    outside = np.ones(h.size, bool)
    for a, s in g.spans:
        outside[a:a + s] = False
    bad = np.flatnonzero(outside & (h != SENTINEL))
    ends = [a + s for a, s in g.spans]
    after = int(np.searchsorted(ends, bad[0], side="right")) - 1   # the slice the first dirty byte follows
    raise AssertionError(f"{bad.size} bytes written outside {what}: the first {int(bad[0]) - ends[after]} bytes past "
                         f"slice {after} (of {len(ends)}, {g.spans[after][1]} bytes), the last at +{int(bad[-1]) - ends[after]}")


def run(b, wire_len, n, chars, scratch_fill=None, chars_shift=0, dwire=None):
    """One guarded call.  chars: bytes per chars column (rounded up to 16
    here: the decode stores 16 aligned bytes at a time)."""
    sizes, at = [8 * (n + 1)], {}
    for f, k in enumerate(b.kinds):
        at[f] = len(sizes)
        sizes += [chars_shift + r16(chars[f]), 8 * (n + 1)] if k == oracle.STRING else [n * oracle.KIND_SIZE[k]]
    o = Out()
    o.g = Checked(sizes)
    o.cols = [o.g.slices[at[f]][chars_shift:] if k == oracle.STRING else o.g.slices[at[f]]
              for f, k in enumerate(b.kinds)]
    o.offs = [o.g.slices[at[f] + 1] if k == oracle.STRING else None for f, k in enumerate(b.kinds)]
    o.rec = o.g.slices[0]
    sb = b.p.var_stream_scratch_bytes(n, wire_len)
    o.gs = Checked([sb])
    if scratch_fill is not None:
        if isinstance(scratch_fill, int):
            o.gs.slices[0].fill_(scratch_fill)
        else:
            k = min(sb, scratch_fill.numel())
            o.gs.slices[0][:k].copy_(scratch_fill[:k])
    st = status_buf()
    b.p.unpack_var_stream(b.dwire if dwire is None else dwire, wire_len, n, o.rec, o.cols, o.offs,
                          o.gs.slices[0], sb, st)
    torch.cuda.synchronize()
    o.st = st.cpu().numpy()
    o.flags, o.reserved = (int(x) for x in o.st[:8].view(np.uint32))
    o.first = int(o.st[8:16].view(np.uint64)[0])
    o.n = n
    pads_clean(o.g, "the outputs (rec_offs, then each field's column and str_offs)")
    pads_clean(o.gs, "the scratch")
    pads_clean(b.gw, "the wire")
    if chars_shift:
        for f, k in enumerate(b.kinds):
            if k == oracle.STRING:
                assert bool((o.g.slices[at[f]][:chars_shift] == SENTINEL).all()), "bytes written before a chars column"
    return o


def u64s(t, lo, hi):
    return t[8 * lo:8 * hi].view(torch.int64)


def verify(b, o, wire_len, want, last=None):
    """The contract, on the device: `same` leading records are the clean
    stream's; then the error tail, or (last: the oracle's columns and offsets
    from record r0 on) one more good record that differs from the clean one."""
    rcname, err, consumed = want
    n = o.n
    if rcname == "ok":
        assert (o.flags, o.first) == (0, NO_BAD), (o.flags, o.first)
        same = n if last is None else n - 1
    else:
        assert o.flags & STATUS_OF[rcname] and o.first == err, (o.flags, o.first, want)
        same = err
        if rcname == "prefix":
            assert int(b.rec[err]) == consumed
    assert torch.equal(o.rec[:8 * (same + 1)], b.xrec[:8 * (same + 1)]), "rec_offs before the bad record"
    if rcname != "ok":
        assert bool((u64s(o.rec, err + 1, n + 1) == wire_len).all()), "rec_offs[err+1..n] != wire_len"
    else:
        assert int(u64s(o.rec, n, n + 1)[0]) == consumed
    for f, k in enumerate(b.kinds):
        if k != oracle.STRING:
            nb = same * oracle.KIND_SIZE[k]
            assert torch.equal(o.cols[f][:nb], b.xcols[f][:nb]), f
            continue
        assert torch.equal(o.offs[f][:8 * (same + 1)], b.xoffs[f][:8 * (same + 1)]), f
        nc = int(b.ooffs[f][same])
        assert torch.equal(o.cols[f][:nc], b.xcols[f][:nc]), f
        if rcname != "ok":
            assert bool((u64s(o.offs[f], err + 1, n + 1) == nc).all()), f"str_offs[{f}][err+1..n] != str_offs[{f}][err]"
    if last is not None:
        ocols, ooffs, r0 = last
        e = same - r0
        for f, k in enumerate(b.kinds):
            if k != oracle.STRING:
                sz = oracle.KIND_SIZE[k]
                assert o.cols[f][same * sz:(same + 1) * sz].cpu().numpy().tobytes() == ocols[f][e:e + 1].tobytes(), f
            else:
                lo, hi = int(ooffs[f][e]), int(ooffs[f][e + 1])
                nc = int(b.ooffs[f][same])
                assert int(u64s(o.offs[f], n, n + 1)[0]) == nc + hi - lo, f
                assert torch.equal(o.cols[f][nc:nc + hi - lo], dev(ocols[f][lo:hi])[:hi - lo]), f


def run_case(b, case, fills=(None,)):
    """A hostile case: the oracle's verdict on it, then the guarded call --
    once per fill of the bytes behind wire_len (None: the clean stream's
    continuation) -- and the contract."""
    want, partial, ocols, ooffs, r0 = streams.oracle_on_case(b.kinds, b.prefix, b.wire, b.rec, case)
    assert want == case.want, (case.name, want)
    same = want[1] if want[0] != "ok" else case.n - 1
    last = (ocols, ooffs, r0) if want[0] == "ok" else None
    if last:
        partial = [0 if o is None else int(o[same - r0 + 1]) - int(o[same - r0]) for o in ooffs]
    outs = []
    try:
        for at, bts in case.patch:
            b.dwire[at:at + bts.size].copy_(torch.from_numpy(np.array(bts)))
        for fill in fills:
            if fill is not None:
                b.dwire[case.wire_len:].fill_(fill)
            o = run(b, case.wire_len, case.n, b.chars(same, partial))
            verify(b, o, case.wire_len, want, last)
            outs.append(o)
    finally:
        lo = min([at for at, _ in case.patch] + [case.wire_len])
        b.dwire[lo:].copy_(b.clean[lo:b.W])
    for o in outs[1:]:
        assert torch.equal(o.g.t, outs[0].g.t) and o.st.tobytes() == outs[0].st.tobytes(), \
            f"{case.name}: the outputs depend on the bytes behind wire_len"
    return outs[0]


def run_clean(b, **kw):
    o = run(b, b.W, b.n, b.chars(b.n), **kw)
    verify(b, o, b.W, ("ok", b.n, b.W))
    return o


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def hostile_base(name):
    def make():
        s = streams.hostile_base(name)
        return Base(s["kinds"], s["prefix"], s["wire"], s["n"]), s
    return cached(("hostile", name), make)


# ---- 3. the hostile sweep --------------------------------------------------

SWEEP = [(base, place) for base in streams.HOSTILE_BASES for place in
         (["first", "last"] + (list(streams.EDGE_SPLITS) if base != "bare_32m" else [])
          + (["group1_first_block", "group1_last_block"] if base != "enveloped_mixed" else [])
          + (["block_4095", "block_4096", "block_4097"] if base == "bare_32m" else []))]


@pytest.mark.parametrize("base,place", SWEEP)
def test_hostile_sweep(base, place, path):
    b, s = hostile_base(base)
    cases = streams.hostile_cases(b.kinds, b.prefix, b.wire, b.rec, b.n, {place: s["places"][place]})
    assert len(cases) >= 9
    for case in cases:
        run_case(b, case, fills=(None, SENTINEL) if case.wire_len < b.W else (None,))


def test_clean_bases_in_guards(path):
    for name in streams.HOSTILE_BASES:
        run_clean(hostile_base(name)[0])


def test_empty_wire(path):
    b, _ = hostile_base("enveloped_mixed")
    for n in (5, 1):
        o = run(b, 0, n, b.chars(0))
        verify(b, o, 0, ("bounds", 0, 0))
    b, _ = hostile_base("five_str")
    verify(b, run(b, 0, 5, b.chars(0)), 0, ("bounds", 0, 0))


# ---- 4. far entries ---------------------------------------------------------

NESTED = {"zh4": ([oracle.INT8, oracle.STRING, oracle.INT16, oracle.STRING], b""),
          "bare": ([oracle.STRING], b""),
          "enveloped": ([oracle.INT32, oracle.STRING, oracle.INT8], oracle.request_prefix("Svc::nested", "N"))}


def nested_base(schema, n=600):
    def make():
        kinds, prefix = NESTED[schema]
        cols, offs = streams.nested_stream(kinds, n, np.random.default_rng(17), prefix=prefix)
        wire = np.frombuffer(oracle.pack(kinds, cols, n, prefix, offs), np.uint8)
        return Base(kinds, prefix, wire, n)
    return cached(("nested", schema, n), make)


@pytest.mark.parametrize("schema", list(NESTED))
def test_far_entries(schema, path):
    b = nested_base(schema)
    o = run_clean(b)
    blocks = (b.W + streams.BLOCK - 1) // streams.BLOCK
    far = streams.far_entries(b.rec, b.W)
    assert far.size >= 0.3 * blocks
    walked = o.reserved >> 8
    print(f"{schema} {path}: reserved bits {o.reserved & 0xff:#x}, walked {walked}, blocks {blocks}, far {far.size}")
    if path == "walk_norepair":
        assert o.reserved & RES_MISS and not o.reserved & RES_REPAIR, o.reserved
    else:
        # the end of a record longer than a block is not among
        # the exits of the block before, so the first scan misses it, the
        # repair runs, and pass 1 walks such blocks -- at most every block
        assert o.reserved & RES_REPAIR, o.reserved
    assert 1 <= walked <= blocks, (walked, blocks)
    # a bad length in a block that a far record enters: the first record that starts there
    c = next(int(c) for c in far[far.size // 2:] if np.searchsorted(b.rec, c * streams.BLOCK) < b.n
             and b.rec[np.searchsorted(b.rec, c * streams.BLOCK)] < (c + 1) * streams.BLOCK)
    r = int(np.searchsorted(b.rec, c * streams.BLOCK))
    a = int(b.rec[r]) + streams.first_len_at(b.kinds, len(b.prefix))
    for v in (2**63, b.W - (a + 8) + 1):
        run_case(b, streams.Case(f"far_block_{c}", [(a, streams._u64(v))], b.W, b.n, ("bounds", r, a + 8)))


# ---- 5. more live exits than exit slots ------------------------------------

FAN_PAIRS = 12   # tests/test_streams_cpu.py: the last fan block is block 64, a scan group's first


def fan_base(T):
    def make():
        wire, n, fans = streams.fan_stream(FAN_PAIRS, np.random.default_rng(3), T=T)
        return Base([oracle.STRING], b"", wire, n), fans
    return cached(("fan", T), make)


@pytest.mark.parametrize("T", [701, 9])
def test_exit_slot_overflow(T, path):
    """T = 701: the cursor's entry into every fan block is none of the 255 kept
    exit slots (a walk); T = 9: it is one of them."""
    b, fans = fan_base(T)
    o = run_clean(b)
    print(f"fan T={T} {path}: reserved bits {o.reserved & 0xff:#x}, walked {o.reserved >> 8}")
    if path != "walk_norepair" and T == 701:
        assert o.reserved & RES_OVER, o.reserved   # more possible entries than exit slots
    # a bad length in the block right after a fan block
    for c in (fans[3], fans[-1]):
        r = int(np.searchsorted(b.rec, (c + 1) * streams.BLOCK))
        assert b.rec[r] < (c + 2) * streams.BLOCK
        a = int(b.rec[r])
        run_case(b, streams.Case(f"after_fan_{c}", [(a, streams._u64(2**63))], b.W, b.n, ("bounds", r, a + 8)))


# ---- 6. placement ------------------------------------------------------------

def random_base():
    b, _ = hostile_base("enveloped_mixed")
    return b


PLACED = {"random": random_base, "nested": lambda: nested_base("zh4", 60), "fan": lambda: fan_base(701)[0]}


@pytest.mark.parametrize("stream", list(PLACED))
def test_wire_and_chars_placement(stream, path):
    """The wire at odd offsets past a 256-byte boundary, a chars column 16
    bytes past one: the same bytes out as from the aligned call."""
    b = PLACED[stream]()
    ref = run_clean(b)
    for front in (1, 3, 4, 8, 15):
        moved = Base(b.kinds, b.prefix, b.wire, b.n, front=front)
        assert moved.dwire.data_ptr() % 256 == front
        o = run_clean(moved)
        assert torch.equal(o.g.t, ref.g.t) and (o.flags, o.first) == (ref.flags, ref.first), front
    o = run_clean(b, chars_shift=16)
    for f in range(len(b.kinds)):
        assert torch.equal(o.cols[f][:ref.cols[f].numel()], ref.cols[f]), f
        assert b.kinds[f] != oracle.STRING or torch.equal(o.offs[f], ref.offs[f]), f
    assert torch.equal(o.rec, ref.rec)


@pytest.mark.parametrize("base", ["enveloped_mixed", "five_str"])
def test_misaligned_outputs_are_refused(base, path):
    """... before any launch: nothing is written, also where the schema goes on
    to the indexed decode (five string fields), which would refuse it only
    after the index kernels had run."""
    b = hostile_base(base)[0]
    n, sb = b.n, b.p.var_stream_scratch_bytes(b.n, b.W)
    f0 = b.kinds.index(oracle.STRING)
    for what in ("chars", "rec_offs", "str_offs"):
        sizes = [8 * (n + 2)] + [x for k in b.kinds for x in
                                 ([b.W + 16, 8 * (n + 2)] if k == oracle.STRING else [n * oracle.KIND_SIZE[k] + 16])]
        g, gs = Checked(sizes), Checked([sb])
        it = iter(g.slices[1:])
        cols, offs = [], []
        for k in b.kinds:
            cols.append(next(it))
            offs.append(next(it) if k == oracle.STRING else None)
        rec = g.slices[0]
        if what == "chars":
            cols[f0] = cols[f0][8:]
        elif what == "rec_offs":
            rec = rec[4:]
        else:
            offs[f0] = offs[f0][4:]
        st = status_buf()
        with pytest.raises(SrpcError) as e:
            b.p.unpack_var_stream(b.dwire, b.W, n, rec, cols, offs, gs.slices[0], sb, st)
        assert e.value.code == srpc_amd._lib.SRPC_E_ALIGN, what
        torch.cuda.synchronize()
        assert bool((g.t == SENTINEL).all()) and bool((gs.t == SENTINEL).all()), what


# ---- 7. the scratch's contents ------------------------------------------------

@pytest.mark.parametrize("stream", ["random", "nested", "error"])
def test_result_is_independent_of_stale_scratch(stream, path):
    b = nested_base("zh4", 60) if stream == "nested" else random_base()
    other = hostile_base("bare_two_str")[0]          # a larger, different stream
    assert other.W > b.W
    left = run_clean(other).gs.slices[0].clone()
    case = None
    if stream == "error":
        r = b.n // 2
        a = int(b.rec[r]) + streams.first_len_at(b.kinds, len(b.prefix))
        case = streams.Case("mid", [(a, streams._u64(2**64 - 1))], b.W, b.n, ("bounds", r, a + 8))
    outs = []
    for fill in (0x00, 0xFF, left):
        if case is None:
            outs.append(run_clean(b, scratch_fill=fill))
            continue
        want, partial, _, _, _ = streams.oracle_on_case(b.kinds, b.prefix, b.wire, b.rec, case)
        try:
            for at, bts in case.patch:
                b.dwire[at:at + bts.size].copy_(torch.from_numpy(np.array(bts)))
            o = run(b, b.W, b.n, b.chars(want[1], partial), scratch_fill=fill)
            verify(b, o, b.W, want)
            outs.append(o)
        finally:
            b.dwire.copy_(b.clean[:b.W])
    for o in outs[1:]:
        assert torch.equal(o.g.t, outs[0].g.t), "the outputs depend on what the scratch held"
        assert o.st.tobytes() == outs[0].st.tobytes(), (o.st, outs[0].st)   # status and reserved


# ---- the checks themselves ------------------------------------------------------

def test_the_checks_notice_a_wrong_byte():
    """verify and the guards fail on one wrong byte in each place they cover
    (outputs of a correct call, damaged here)."""
    b = random_base()
    r = b.n // 3
    a = int(b.rec[r]) + streams.first_len_at(b.kinds, len(b.prefix))
    case = streams.Case("third", [(a, streams._u64(2**63))], b.W, b.n, ("bounds", r, a + 8))
    f0 = b.kinds.index(oracle.STRING)
    damage = {
        "rec_offs before": lambda o: o.rec[8 * (r - 1)].add_(1),
        "rec_offs tail": lambda o: o.rec[8 * (b.n - 2)].add_(1),
        "str_offs before": lambda o: o.offs[f0][8 * (r - 1)].add_(1),
        "str_offs tail": lambda o: o.offs[f0][8 * (r + 5)].add_(1),
        "chars": lambda o: o.cols[f0][int(b.ooffs[f0][r]) - 1].add_(1),
        "fixed": lambda o: o.cols[0][r - 1].add_(1),
    }
    for what, hit in damage.items():
        o = run_case(b, case)
        verify(b, o, b.W, case.want)
        hit(o)
        with pytest.raises(AssertionError):
            verify(b, o, b.W, case.want)
    o = run_case(b, case)
    for g, at in ((o.g, o.g.spans[1][0] + o.g.spans[1][1]), (o.g, o.g.t.numel() - 1), (o.gs, 0)):
        pads_clean(g, "")
        g.t[at] = 0
        with pytest.raises(AssertionError):
            pads_clean(g, "")
        g.t[at] = SENTINEL
