"""A batch whose wire passes a byte boundary (2^32 by default), every byte of
it from the CPU oracle (helper of tests/test_gpu_past_4gib.py, proven to be
what it says by tests/test_giant_cpu.py; no test in here).

The wire format appends: the wire of a concatenation of batches is the
concatenation of their wires.  So a handful of small *segments* -- seeded numpy
inputs, packed by oracle.pack on the CPU -- are uploaded once and then
concatenated with torch.cat in a seeded, non-periodic order: the segment wires
into the reference wire, the segment inputs (fixed columns, chars, string
offsets and record offsets with their running bases added) into the inputs of
the same batch.  No kernel of the library takes part.

build(kinds, prefix, straddle) arranges the order so that the boundary byte
lies where `straddle` says:
  "short": strictly inside a short record whose index is no multiple of 16
           (for a fixed record whose size divides the boundary neither is
           possible: the boundary is then a record boundary by arithmetic, and
           Giant.inside says so);
  "long":  (string schemas) inside the one long string of a one-record segment
           that begins before the boundary and ends after it; a second such
           record lies wholly past the boundary.
The premises are asserted when the batch is built: a test that did not meet
its own premise fails.

Offsets are held as int64 tensors: every value is below 2^63, so the bytes are
those of the uint64 the ABI reads.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

import oracle

STR = oracle.STRING
MIB = 1 << 20
SEG_TARGETS = (9 * MIB + 4111, 10 * MIB + 70001, 12 * MIB + 333, 13 * MIB + 500009, 15 * MIB + 17)
SEG_RANGE = (8 * MIB, 16 * MIB)


def fixed_bytes(kinds, prefix_len=0):
    return prefix_len + sum(8 if k == STR else oracle.KIND_SIZE[k] for k in kinds)


@dataclass
class Segment:
    """A small batch: numpy inputs and the oracle's wire of them."""
    n: int
    cols: list            # numpy column (fixed field) or uint8 chars (string field), exact length
    offs: list            # n + 1 u64 string offsets from 0, or None
    rec: np.ndarray       # n + 1 u64 record starts from 0
    wire: np.ndarray      # uint8

    @property
    def nbytes(self):
        return int(self.wire.size)


def _bytes(n, rng, zero_heavy):
    """n random bytes; zero_heavy: 19 in 20 of them zero (where the stream decode's
    speculated record starts are often wrong, tests/streams.py)."""
    c = rng.integers(0, 256, n, dtype=np.uint8)
    if zero_heavy:
        c[rng.random(n) >= 0.05] = 0
    return c


def _fixed_col(k, n, rng, zero_heavy=False):
    dt = np.dtype(oracle.KIND_DTYPE[k])
    c = _bytes(n * dt.itemsize, rng, zero_heavy).view(dt)
    return (c & 1).astype(np.uint8) if k == oracle.BOOL else c


def _segment(kinds, prefix, n, lens, rng, zero_heavy=False):
    """lens: per string field, the n lengths."""
    cols, offs, si = [], [], 0
    sizes = np.full(n, fixed_bytes(kinds, len(prefix)), np.uint64)
    for k in kinds:
        if k == STR:
            o = np.zeros(n + 1, np.uint64)
            o[1:] = np.cumsum(lens[si].astype(np.uint64))
            sizes += lens[si].astype(np.uint64)
            si += 1
            cols.append(_bytes(int(o[-1]), rng, zero_heavy))
            offs.append(o)
        else:
            cols.append(_fixed_col(k, n, rng, zero_heavy))
            offs.append(None)
    rec = np.zeros(n + 1, np.uint64)
    rec[1:] = np.cumsum(sizes)
    # oracle.pack wants a non-empty chars array to point at
    pcols = [c if c.size else np.zeros(1, np.uint8) for c in cols]
    wire = np.frombuffer(oracle.pack(kinds, pcols, n, prefix, list(offs)), np.uint8).copy()
    assert wire.size == int(rec[n])
    return Segment(n, cols, offs, rec, wire)


def make_segment(kinds, prefix, target_bytes, seed, maxlen, parity, zero_heavy=False):
    """About target_bytes of wire; n has the given parity (0 / 1).  Strings as
    tests/test_gpu_parity._random_string_batch draws them: uniform in
    [0, maxlen], a fifth of them emptied."""
    rng = np.random.default_rng([0x61A7, seed])
    ns = sum(k == STR for k in kinds)
    avg = fixed_bytes(kinds, len(prefix)) + ns * 0.4 * maxlen
    n = max(3, int(target_bytes / avg))
    n += (n & 1) != parity
    lens = []
    for _ in range(ns):
        ln = rng.integers(0, maxlen + 1, n).astype(np.uint64)
        ln[rng.random(n) < 0.2] = 0
        lens.append(ln)
    return _segment(kinds, prefix, n, lens, rng, zero_heavy)


def make_long_segment(kinds, prefix, long_len, seed, maxlen, zero_heavy=False):
    """One record whose first string has long_len chars."""
    rng = np.random.default_rng([0x10E6, seed])
    ns = sum(k == STR for k in kinds)
    assert ns, "the long arrangement is for string schemas"
    lens = [np.array([long_len if s == 0 else int(rng.integers(0, maxlen + 1))], np.uint64) for s in range(ns)]
    return _segment(kinds, prefix, 1, lens, rng, zero_heavy)


def _periodic(order):
    """True when the order repeats itself with a period of at most half its length."""
    o = np.asarray(order)
    return any(np.array_equal(o[p:], o[:-p]) for p in range(1, len(o) // 2 + 1))


def locate(segs, order, boundary):
    """(position in the order, record within that segment, global record
    index, bytes of that record before the boundary) of the boundary byte."""
    lens = np.array([segs[i].nbytes for i in order], np.int64)
    cs = np.cumsum(lens)
    j = int(np.searchsorted(cs, boundary, side="right"))
    assert j < len(order), "the wire does not reach the boundary"
    local = boundary - int(cs[j] - lens[j])
    s = segs[order[j]]
    r = int(np.searchsorted(s.rec, local, side="right")) - 1
    g = sum(segs[i].n for i in order[:j]) + r
    return j, r, g, local - int(s.rec[r])


def arrange(segs, longs, straddle, boundary, tail, seed=0, tries=20000):
    """A seeded order of segment indices (indices >= len(segs) name longs[])
    that meets the arrangement; the premises are asserted by assemble()."""
    K = len(segs)
    L = np.array([s.nbytes for s in segs], np.int64)
    N = np.array([s.n for s in segs], np.int64)
    rb_fixed = None
    if all(o is None for o in segs[0].offs):
        rb_fixed = int(L[0]) // int(N[0])
    count = int((boundary + tail) // int(L.min())) + 2
    for t in range(tries):
        rng = np.random.default_rng([0x0DE4, seed, t])
        order = rng.integers(0, K, count)
        if straddle == "long":
            la, lb = longs[0].nbytes, longs[1].nbytes
            cs = np.cumsum(L[order])
            d = boundary - cs
            ok = np.nonzero((d > la // 4) & (d < 3 * (la // 4)))[0]
            if not len(ok):
                continue
            k = int(ok[0]) + 1                      # longs[0] goes after k ordinary segments
            gap = 1 + int(rng.integers(0, 3))       # ordinary segments between the two long ones
            order = list(order[:k]) + [K] + list(order[k:k + gap]) + [K + 1] + list(order[k + gap:])
            allsegs = list(segs) + list(longs)
        else:
            order = list(order)
            allsegs = list(segs)
        cs = np.cumsum([allsegs[i].nbytes for i in order])
        cut = int(np.searchsorted(cs, boundary + tail, side="left"))
        if cut >= len(order):
            continue
        order = [int(i) for i in order[:cut + 1]]
        if straddle == "long" and (K + 1) not in order:
            continue
        if sum(allsegs[i].n for i in order) % 2 == 0:
            continue
        if _periodic(order):
            continue
        if straddle == "short" and not (rb_fixed and boundary % rb_fixed == 0):
            _, _, g, into = locate(allsegs, order, boundary)
            if into == 0 or g % 16 == 0:
                continue
        return order
    raise AssertionError(f"no {straddle!r} arrangement found in {tries} orders")


@dataclass
class Giant:
    kinds: list
    prefix: bytes
    straddle: str
    boundary: int
    segs: list                 # every segment the order names, the long ones last
    order: list
    n: int = 0
    W: int = 0
    rec_index: int = 0         # the record that holds the boundary byte
    into: int = 0              # bytes of that record before the boundary byte (0: it begins there)
    inside: bool = False       # the boundary byte lies strictly inside a record
    long_records: list = field(default_factory=list)  # global indices of the long records
    ref: "torch.Tensor" = None      # uint8[W]
    cols: list = None               # per field: the column / the chars
    offs: list = None               # per field: int64[n + 1] or None
    rec_offs: "torch.Tensor" = None  # int64[n + 1]
    device: object = "cpu"

    # ---- the oracle's bytes of a window, from the CPU segments alone --------
    def _window(self, sizes, get, lo, hi):
        """Elements [lo, hi) of the concatenation whose part p has sizes[p]
        elements, get(p) giving part p."""
        out, at = [], 0
        for p, sz in enumerate(sizes):
            a, b = max(lo, at), min(hi, at + sz)
            if a < b:
                out.append(get(p)[a - at:b - at])
            at += sz
            if at >= hi:
                break
        return np.concatenate(out) if out else np.zeros(0, np.uint8)

    def wire_window(self, lo, hi):
        return self._window([self.segs[i].nbytes for i in self.order], lambda p: self.segs[self.order[p]].wire, lo, hi)

    def col_window(self, f, lo, hi):
        """Elements [lo, hi) of input column f (chars for a string field)."""
        return self._window([self.segs[i].cols[f].size for i in self.order],
                            lambda p: self.segs[self.order[p]].cols[f], lo, hi)

    def _based_window(self, per_seg, lo, hi):
        """Entries [lo, hi) of an offsets array (n + 1 entries, running bases added)."""
        sizes = [self.segs[i].n for i in self.order]
        bases = np.concatenate([[0], np.cumsum([int(per_seg(self.segs[i])[-1]) for i in self.order])])
        parts = lambda p: per_seg(self.segs[self.order[p]])[:-1] + np.uint64(bases[p])
        body = self._window(sizes, parts, lo, min(hi, self.n)).astype(np.uint64)
        if hi > self.n:
            body = np.concatenate([body, np.array([bases[-1]], np.uint64)])
        return body

    def off_window(self, f, lo, hi):
        return self._based_window(lambda s: s.offs[f], lo, hi)

    def rec_window(self, lo, hi):
        return self._based_window(lambda s: s.rec, lo, hi)

    def col_len(self, f):
        return sum(self.segs[i].cols[f].size for i in self.order)

    # ---- the device arrays, from the segments with torch.cat ---------------------
    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def upload_wire(self):
        d = {i: self._up(self.segs[i].wire) for i in set(self.order)}
        self.ref = torch.cat([d[i] for i in self.order])

    def upload_inputs(self):
        """cols, offs and rec_offs (again, after drop_inputs: a test that cannot hold them next to
        its outputs and scratch drops them for the call and makes them anew to compare)."""
        idx = set(self.order)
        self.cols, self.offs = [], []
        for f, k in enumerate(self.kinds):
            d = {i: self._up(self.segs[i].cols[f]) for i in idx}
            self.cols.append(torch.cat([d[i] for i in self.order]))
            if k == STR:
                d = {i: self._up(self.segs[i].offs[f].astype(np.int64)) for i in idx}
                self.offs.append(_cat_based(d, self.order, self.device))
            else:
                self.offs.append(None)
        d = {i: self._up(self.segs[i].rec.astype(np.int64)) for i in idx}
        self.rec_offs = _cat_based(d, self.order, self.device)

    def drop_inputs(self):
        self.cols = self.offs = self.rec_offs = None

    def free(self):
        self.ref = None
        self.drop_inputs()


def wrap_visible(t, boundary, win=4096, what="array"):
    """Premise: an index into t (a 1-D tensor) that lost its bits from
    `boundary` bytes up would be seen.  The win elements from the element that
    holds byte `boundary` of t, if it has one, differ from t's first win."""
    b = boundary // t.element_size()
    if t.numel() <= b:
        return False
    m = min(win, t.numel() - b)
    assert not torch.equal(t[b:b + m], t[:m]), f"{what}: a wrapped index would not be seen at byte {boundary}"
    return True


def assemble(kinds, prefix, straddle, segs, order, boundary, device, win=4096, margin=MIB, nlong=0):
    """The batch of `order` over `segs` (the last nlong of them long records),
    its premises asserted."""
    kinds = list(kinds)
    g = Giant(kinds, bytes(prefix), straddle, boundary, list(segs), [int(i) for i in order])
    used = [segs[i] for i in g.order]
    g.n = sum(s.n for s in used)
    g.W = sum(s.nbytes for s in used)
    rb = fixed_bytes(kinds, len(prefix)) if STR not in kinds else 0

    # -- the segments
    K = len(segs) - nlong
    lens = [s.nbytes for s in segs[:K]]
    assert len(set(lens)) == len(lens), "segment lengths are not pairwise different"
    assert all(boundary % ln for ln in lens), "a segment length divides the boundary"

    # -- where the boundary byte is
    assert g.W >= boundary + margin and boundary >= margin, "ordinary records on both sides of the boundary"
    j, r, g.rec_index, g.into = locate(segs, g.order, boundary)
    g.inside = g.into != 0
    starts = np.concatenate([[0], np.cumsum([s.n for s in used])])
    g.long_records = [int(starts[p]) for p, i in enumerate(g.order) if i >= K]
    if straddle == "short":
        assert not g.long_records
        if rb and boundary % rb == 0:
            assert not g.inside  # arithmetic: every record of this size begins at a multiple of it
        else:
            assert g.inside, "short: the boundary byte lies on a record boundary"
            assert g.rec_index % 16, "short: the boundary record's index is a multiple of 16"
    elif straddle == "long":
        assert nlong == 2 and len(g.long_records) == 2, "long: two long records"
        a, b = g.long_records
        assert g.rec_index == a, "long: the boundary byte lies outside the first long record"
        s = segs[g.order[j]]
        f0 = kinds.index(STR)
        head = len(prefix) + sum(8 if k == STR else oracle.KIND_SIZE[k] for k in kinds[:f0]) + 8
        assert head < g.into < head + int(s.offs[f0][1]), "long: the boundary byte lies outside the long string"
        pb = g.order.index(K + 1)
        assert sum(x.nbytes for x in used[:pb]) > boundary, "long: the second long record begins before the boundary"
    else:
        raise ValueError(straddle)
    assert g.n % 2 == 1, "n is even"
    assert not _periodic(g.order), "the order is periodic"

    # -- build with torch alone
    g.device = device
    g.upload_wire()
    g.upload_inputs()
    assert g.ref.numel() == g.W and g.rec_offs.numel() == g.n + 1

    # -- a wrapped index would be seen
    assert wrap_visible(g.ref, boundary, win, "wire"), "the wire does not pass the boundary"
    for f, c in enumerate(g.cols):
        wrap_visible(c, boundary, win, f"column {f}")
        if g.offs[f] is not None:
            wrap_visible(g.offs[f], boundary, win, f"offsets {f}")
    wrap_visible(g.rec_offs, boundary, win, "rec_offs")
    return g


def _cat_based(d, order, device):
    """cat of the per-segment offsets (each n + 1 entries from 0) with running bases added."""
    parts, base = [], 0
    ends = {i: int(t[-1]) for i, t in d.items()}
    for i in order:
        parts.append(d[i][:-1] + base)
        base += ends[i]
    parts.append(torch.tensor([base], dtype=torch.int64, device=device))
    return torch.cat(parts)


def build(kinds, prefix, straddle, device="cuda:0", boundary=2**32, seg_targets=SEG_TARGETS, seg_range=SEG_RANGE,
          tail=64 * MIB, long_len=MIB + 4321, maxlen=40, win=4096, margin=MIB, seed=0, zero_heavy=False):
    """The batch of `kinds` under `prefix` whose wire passes `boundary` by about `tail` bytes
    (zero_heavy: 19 in 20 bytes of every field and string are zero)."""
    kinds = list(kinds)
    segs = [make_segment(kinds, prefix, t, 16 * seed + i, maxlen, i & 1, zero_heavy) for i, t in enumerate(seg_targets)]
    for s in segs:
        assert seg_range[0] <= s.nbytes <= seg_range[1], f"a segment of {s.nbytes} bytes"
    longs = []
    if straddle == "long":
        longs = [make_long_segment(kinds, prefix, long_len + 1237 * i, 16 * seed + i, maxlen, zero_heavy) for i in range(2)]
    order = arrange(segs, longs, straddle, boundary, tail, seed)
    return assemble(kinds, prefix, straddle, segs + longs, order, boundary, device, win, margin, len(longs))
