"""Adversarial string-record streams for the index-free decode (pure numpy:
used by tests/test_gpu_stream.py, tests/test_gpu_stream_hostile.py and
tools/stream_bench.py; their properties are checked on the CPU by
tests/test_streams_cpu.py)."""
from collections import namedtuple

import numpy as np

import oracle

BLOCK = 8192    # wire bytes per decode block (sdx.hip kSB)
MARGIN = 1536   # bytes past a block that its workgroup stages (kMargin)
WINDOW = 64     # entry window of a block's table (kWin)
SLOTS = 255     # exit slots per block (kE)


def straddler_stream(n, rng, lead, over, fill="zero", maxlen=24, p_empty=0.5, p_nonzero=0.05):
    """zero-heavy int8/string/int16/string records,
    and across EVERY 8 KiB block boundary one record (its first string
    `fill`: all zero bytes, or zero-heavy like the rest) that starts `lead`
    bytes before the boundary and ends `over` bytes after it -- past the
    table's 64-byte window, inside chars where the speculation has no clue.
    Returns the columns and string offsets for oracle.pack."""
    l0 = rng.integers(0, maxlen, n)
    l0[rng.random(n) < p_empty] = 0
    l1 = rng.integers(0, maxlen, n)
    l1[rng.random(n) < p_empty] = 0
    size = 19 + l0 + l1
    pos, i, B = 0, 0, 8192
    L0, L1, FIL = [], [], []
    while i < n:
        ld, ov = int(rng.integers(*lead)), int(rng.integers(*over))
        cs = pos + np.cumsum(size[i:i + 2 * 8192 // 19 + 4])
        k = min(int(np.searchsorted(cs, B - ld, side="right")), n - i)
        L0.append(l0[i:i + k])
        L1.append(l1[i:i + k])
        FIL.append(np.zeros(k, bool))
        if k:
            pos = int(cs[k - 1])
        i += k
        if i >= n:
            break
        L0.append(np.array([B + ov - pos - 19]))  # from pos (at most `lead` before B) to B + over
        L1.append(np.array([0]))
        FIL.append(np.ones(1, bool))
        pos, i = B + ov, i + 1
        while B <= pos:
            B += 8192
    l0, l1, fil = np.concatenate(L0)[:n], np.concatenate(L1)[:n], np.concatenate(FIL)[:n]
    cols, offs = [np.zeros(n, np.int8), None, np.zeros(n, np.int16), None], [None, None, None, None]
    for f, ls in ((1, l0), (3, l1)):
        o = np.zeros(n + 1, np.uint64)
        o[1:] = np.cumsum(ls)
        c = np.zeros(max(1, int(o[-1])), np.uint8)
        nz = rng.random(c.size) < p_nonzero
        if fill == "zero":  # the straddling records' chars stay all zero
            for r in np.flatnonzero(fil & (ls > 0)):
                nz[int(o[r]):int(o[r + 1])] = False
        c[nz] = 7
        cols[f], offs[f] = c, o
    return cols, offs


def random_batch(kinds, n, rng, maxlen):
    """Random columns and string offsets for oracle.pack: string lengths
    0..maxlen, a fifth of them empty, random chars and fixed fields."""
    cols, offs = [], []
    for k in kinds:
        if k == oracle.STRING:
            lens = rng.integers(0, maxlen + 1, n).astype(np.uint64)
            lens[rng.random(n) < 0.2] = 0
            o = np.zeros(n + 1, np.uint64)
            o[1:] = np.cumsum(lens)
            cols.append(rng.integers(0, 256, max(1, int(o[-1])), dtype=np.uint8))
            offs.append(o)
        else:
            dt = np.dtype(oracle.KIND_DTYPE[k])
            c = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
            cols.append((c & 1).astype(np.uint8) if k == oracle.BOOL else c)
            offs.append(None)
    return cols, offs


def record_starts(kinds, offs, n, prefix_len=0):
    """Record starts 0..n of the packed stream, from the string offsets."""
    fixed = prefix_len + sum(8 if k == oracle.STRING else oracle.KIND_SIZE[k] for k in kinds)
    sizes = np.full(n, fixed, np.uint64)
    for k, o in zip(kinds, offs):
        if k == oracle.STRING:
            sizes += np.diff(np.asarray(o[:n + 1], np.uint64))
    r = np.zeros(n + 1, np.uint64)
    r[1:] = np.cumsum(sizes)
    return r


def nested_stream(kinds, n, rng, lo=9 * 1024, hi=20 * 1024, inner_max=24, prefix=b""):
    """Ordinary random records (strings up to inner_max), except that each
    record's first string is lo..hi bytes cut at a random offset out of a
    packed stream of the SAME schema and prefix: inside such a string almost
    every block speculates a chain of records that parses and is wrong, and
    about half the blocks are entered by a record that started two or more
    blocks back (far_entries).  Returns the columns and string offsets
    for oracle.pack."""
    f0 = list(kinds).index(oracle.STRING)
    m = 4096
    icols, ioffs = random_batch(kinds, m, rng, inner_max)
    inner = np.frombuffer(oracle.pack(kinds, icols, m, prefix, list(ioffs)), np.uint8)
    assert inner.size > hi
    cols, offs = random_batch(kinds, n, rng, inner_max)
    lens = rng.integers(lo, hi + 1, n)
    at = rng.integers(0, inner.size - hi, n)
    o = np.zeros(n + 1, np.uint64)
    o[1:] = np.cumsum(lens)
    cols[f0] = np.concatenate([inner[a:a + l] for a, l in zip(at, lens)])
    offs[f0] = o
    return cols, offs


def far_entries(rec, W):
    """Blocks c >= 1 of a W-byte wire entered by a record that started two or
    more blocks back (before block c - 1), given the record starts."""
    rec = np.asarray(rec).astype(np.int64)
    edges = np.arange(1, (W + BLOCK - 1) // BLOCK, dtype=np.int64) * BLOCK
    holder = np.searchsorted(rec, edges, side="right") - 1  # the record that holds byte c * BLOCK
    return edges[rec[holder] < edges - BLOCK] // BLOCK


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype="<u8")).view(np.uint8)


def fan_stream(pairs, rng, delta=40, T=701, gap_blocks=3, first=9):
    """Bare one-string records with `pairs` fan blocks c = first, first +
    gap_blocks + 2, ...: ordinary records (strings of 0..40 random bytes) run
    to `delta` bytes into block c - 1; then ONE record that ends 8 T bytes
    into block c, whose chars inside block c - 1 are u64 values, one per 8
    bytes, each a length that ends at a DIFFERENT 8-aligned position of block
    c (never 8 T); block c is 16-byte records (length 8, chars = u64 8), so
    every 8-aligned position of it parses, on two chains that never merge.
    Every fan block then has ~1000 distinct live exits (live_exits), more
    than its exit slots, and only the one at 8 T is where the cursor enters.
    Returns (wire as uint8 array, n records, the fan blocks)."""
    assert delta % 8 == 0 and 0 < T < BLOCK // 8 and first >= 2
    out, fans = [], []
    pos = n = 0

    def put(length, chars):
        nonlocal pos, n
        out.append(_u64(length))
        out.append(chars)
        pos += 8 + int(length)
        n += 1

    def ordinary(target):
        while target - pos > 64:
            k = int(rng.integers(0, 41))
            put(k, rng.integers(0, 256, k, dtype=np.uint8))
        k = target - pos - 8
        put(k, rng.integers(0, 256, k, dtype=np.uint8))

    for i in range(pairs):
        c = first + i * (gap_blocks + 2)
        fans.append(c)
        cB = c * BLOCK
        ordinary(cB - BLOCK + delta)
        p = np.arange(pos + 8, cB, 8, dtype=np.int64)       # the fan record's chars inside block c - 1
        j = rng.permutation(np.delete(np.arange(BLOCK // 8), T))[:p.size]
        fan = (cB + 8 * j - p - 8).astype("<u8").view(np.uint8)
        put(cB + 8 * T - pos - 8, np.concatenate([fan, _u64(np.full(T, 8))]))
        while pos < cB + BLOCK:
            put(8, _u64(8))
    ordinary((fans[-1] + 1 + gap_blocks) * BLOCK - 100)
    return np.concatenate(out), n, fans


def live_exits(wire, c):
    """The brute-force model of the repair pass for bare one-string records:
    the ends, inside block c, of records that parse at a position of block
    c - 1, at which a record parses too (ascending, distinct)."""
    w = np.asarray(wire, np.uint8)
    W = w.size
    words = np.lib.stride_tricks.sliding_window_view(np.concatenate([w, np.zeros(8, np.uint8)]), 8)

    def parse(pos):
        pos = pos[pos + 8 <= W]
        v = np.ascontiguousarray(words[pos]).view("<u8").ravel()
        ok = v <= (W - pos - 8).astype(np.uint64)
        return pos[ok] + 8 + v[ok].astype(np.int64)

    ends = np.unique(parse(np.arange((c - 1) * BLOCK, min(c * BLOCK, W), dtype=np.int64)))
    ends = ends[(ends >= c * BLOCK) & (ends < (c + 1) * BLOCK)]
    live = ends[ends + 8 <= W]
    v = np.ascontiguousarray(words[live]).view("<u8").ravel()
    return live[v <= (W - live - 8).astype(np.uint64)]


# ---- hostile variants of one clean stream ---------------------------------

# name: what is done to which record; patch: [(wire offset, bytes)] over the
# clean stream (kept as patches: the 32 MiB stream is not copied per case);
# the call's wire_len and n; want: the verdict the name promises, (oracle
# return code, first bad record, consumed), worked out from the record layout
# alone (tests/test_streams_cpu.py holds the oracle to it).
Case = namedtuple("Case", "name patch wire_len n want")

EDGE_SPLITS = {"edge_1_7": BLOCK - 1, "edge_4_4": BLOCK - 4, "edge_7_1": BLOCK - 7,
               "margin_1_7": MARGIN - 1, "margin_4_4": MARGIN - 4, "margin_7_1": MARGIN - 7}


def _layout(kinds, prefix_len, wire, q):
    """The clean record at q: [(length field position, length)] of its string
    fields, [(position, size, follows a string)] of its fixed fields."""
    at = q + prefix_len
    strs, fixed = [], []
    for k in kinds:
        if k == oracle.STRING:
            length = int(np.ascontiguousarray(wire[at:at + 8]).view("<u8")[0])
            strs.append((at, length))
            at += 8 + length
        else:
            fixed.append((at, oracle.KIND_SIZE[k], bool(strs)))
            at += oracle.KIND_SIZE[k]
    return strs, fixed


def first_len_at(kinds, prefix_len):
    d = prefix_len
    for k in kinds:
        if k == oracle.STRING:
            return d
        d += oracle.KIND_SIZE[k]


def _lengthen(cols, offs, f, r, d, rng):
    """d more random chars at the end of string field f of record r."""
    cols[f] = np.insert(cols[f], int(offs[f][r + 1]), rng.integers(0, 256, d, dtype=np.uint8))
    offs[f][r + 1:] += np.uint64(d)


def with_straddles(kinds, cols, offs, n, prefix_len, rng, residues=tuple(EDGE_SPLITS.values())):
    """Lengthen one string before each of len(residues) evenly spread records
    so that the 8 bytes of that record's first length field start at the
    given offsets modulo the block: split 1/7, 4/4 and 7/1 over a block edge
    and over the end of a block's staged margin.  Those records, the first
    and the last get a first string of at least 2 chars (to be cut inside)."""
    f0 = list(kinds).index(oracle.STRING)
    cols, offs = list(cols), [None if o is None else o.copy() for o in offs]
    d0 = first_len_at(kinds, prefix_len)
    targets = [(i + 1) * n // (len(residues) + 1) for i in range(len(residues))]
    for r in [0, n - 1] + targets:
        if offs[f0][r + 1] - offs[f0][r] < 2:
            _lengthen(cols, offs, f0, r, 4, rng)
    for t, res in zip(targets, residues):
        a = int(record_starts(kinds, offs, n, prefix_len)[t]) + d0
        d = (res - a) % BLOCK
        if d:
            _lengthen(cols, offs, f0, t - 1, d, rng)
    return cols, offs


def hostile_places(kinds, prefix_len, wire, rec, n, straddles=True):
    """Records to go bad: the first and the last; one starting in the first
    and one in the last block of scan group 1 (blocks 64 and 127, or the
    wire's last); in blocks 4095-4097 where the wire has them (the in-order
    scan reloads its registers every 64 groups); and records whose first
    length field straddles a block edge or the end of a staged margin."""
    rec = np.asarray(rec).astype(np.int64)
    nb = (wire.size + BLOCK - 1) // BLOCK
    places = {"first": 0, "last": n - 1}
    blocks = {}
    if nb > 64:
        blocks["group1_first_block"] = 64
        blocks["group1_last_block"] = min(127, nb - 1)
    if nb > 4097:
        blocks.update(block_4095=4095, block_4096=4096, block_4097=4097)
    for name, b in blocks.items():
        lo, hi = np.searchsorted(rec[:n], [b * BLOCK, (b + 1) * BLOCK])
        # one whose strings can be cut inside their chars, if the block starts one
        rs = [r for r in range(lo, hi) if any(ln >= 2 for _, ln in _layout(kinds, prefix_len, wire, int(rec[r]))[0])]
        assert lo < hi, (name, b)
        places[name] = rs[0] if rs else int(lo)
    a = rec[:n] + first_len_at(kinds, prefix_len)
    for name, res in EDGE_SPLITS.items() if straddles else ():
        hit = np.flatnonzero((a % BLOCK == res) & (a > BLOCK))
        hit = [r for r in hit if _layout(kinds, prefix_len, wire, int(rec[r]))[0][0][1] >= 2]
        if hit:
            places[name] = int(hit[len(hit) // 2])
    return places


def hostile_cases(kinds, prefix, wire, rec, n, places=None):
    """Hostile variants of one clean stream (wire: uint8 array; rec: its n + 1
    record starts): at each place a flipped prefix byte, string lengths that
    run past the wire or wrap, a string ending exactly at the wire's end, and
    the wire cut inside a prefix, a length field, chars, a fixed field and at
    the record's start.  A list of Case."""
    wire = np.asarray(wire, np.uint8)
    W, plen = wire.size, len(prefix)
    if places is None:
        places = hostile_places(kinds, plen, wire, rec, n)
    cases = []
    for place, r in places.items():
        q = int(rec[r])
        strs, fixed = _layout(kinds, plen, wire, q)

        def add(kind, patch, wire_len, ncall, want):
            cases.append(Case(f"{place}/{kind}->{want[0]}@{want[1]}", patch, wire_len, ncall, want))

        if plen:
            at = q + min(10, plen - 1)
            add("flip_prefix", [(at, np.array([wire[at] ^ 0x04], np.uint8))], W, n, ("prefix", r, q))
        which = [("first_str", strs[0])] + ([("last_str", strs[-1])] if len(strs) > 1 else [])
        for wname, (a, _) in which:
            for lname, v in (("past_by_1", W - (a + 8) + 1), ("2^32", 2**32), ("2^63", 2**63),
                             ("2^64-1", 2**64 - 1), ("wraps", 2**64 - a - 7)):
                add(f"{wname}_len_{lname}", [(a, _u64(v))], W, n, ("bounds", r, a + 8))
        a = strs[-1][0]
        if kinds[-1] == oracle.STRING:   # the record becomes the stream's last and consumes it
            add("string_ends_at_wire_len", [(a, _u64(W - (a + 8)))], W, r + 1, ("ok", r + 1, W))
        else:                            # ... and its trailing fixed field is missing
            add("string_ends_at_wire_len", [(a, _u64(W - (a + 8)))], W, n, ("bounds", r, W))
        if plen >= 2:
            add("cut_prefix", [], q + plen // 2, n, ("bounds", r, q))
        add("cut_length", [], strs[0][0] + 3, n, ("bounds", r, strs[0][0]))
        for a, ln in strs:
            if ln >= 2:
                add("cut_chars", [], a + 8 + ln // 2, n, ("bounds", r, a + 8))
                break
        wide = [f for f in fixed if f[1] >= 2]
        if wide:
            at = ([f for f in wide if f[2]] or wide)[0][0]   # a fixed field after a string, if there is one
            add("cut_fixed", [], at + 1, n, ("bounds", r, at))
        add("cut_at_record_start", [], q, r + 1, ("bounds", r, q))
    return cases


def patched(wire, case, lo=0):
    """wire[lo:case.wire_len] with the case's patch applied (a copy)."""
    sub = np.array(wire[lo:case.wire_len])
    for at, b in case.patch:
        assert lo <= at and at + b.size <= case.wire_len
        sub[at - lo:at - lo + b.size] = b
    return sub


ORC_NAME = {oracle.ORC_OK: "ok", oracle.ORC_ERR_BOUNDS: "bounds", oracle.ORC_ERR_PREFIX: "prefix"}


def oracle_on_case(kinds, prefix, wire, rec, case):
    """The oracle's decode of a case: (verdict as Case.want, chars per string
    field that it wrote for the bad record's fields before the failing one,
    the columns and string offsets of records r0.., r0).  The cursor has no
    state but its position, and a case changes no byte before its record, so
    the oracle starts at record r0, one before the first byte that differs
    from the clean stream."""
    x = min([at for at, _ in case.patch] + [case.wire_len])
    r0 = max(int(np.searchsorted(np.asarray(rec).astype(np.int64), x, side="right")) - 2, 0)
    r0 = min(r0, case.n - 1)
    base = int(rec[r0])
    m = case.n - r0
    rc, cols, offs, consumed, err = oracle.unpack(kinds, patched(wire, case, base).tobytes(), m, prefix)
    partial = [0 if o is None or rc == oracle.ORC_OK or not int(o[err + 1]) else int(o[err + 1]) - int(o[err])
               for o in offs]
    return (ORC_NAME[rc], err + r0, consumed + base), partial, cols, offs, r0


def _truncate(kinds, cols, offs, n):
    out = []
    for k, c, o in zip(kinds, cols, offs):
        out.append(c[:max(1, int(o[n]))] if k == oracle.STRING else c[:n])
    return out, [None if o is None else o[:n + 1] for o in offs]


HOSTILE_BASES = {
    # name: (kinds, enveloped, records, longest string, straddling length fields)
    "enveloped_mixed": ([oracle.INT8, oracle.STRING, oracle.INT64, oracle.BOOL, oracle.STRING, oracle.INT16],
                        True, 3900, 60, True),                       # ~0.45 MB: within scan group 0
    "bare_two_str": ([oracle.STRING, oracle.INT32, oracle.STRING], False, 11_500, 100, True),   # ~1.2 MB: group 1 whole
    "five_str": ([oracle.STRING, oracle.INT8, oracle.STRING, oracle.INT16, oracle.STRING, oracle.INT64,
                  oracle.STRING, oracle.INT8, oracle.STRING, oracle.INT16], True, 8000, 30, True),
    # just over 32 MiB in ~20k records: blocks 4095-4097, past the scan's 64-group reload
    "bare_32m": ([oracle.INT32, oracle.STRING, oracle.INT8], False, 22_000, 4096, False),
}
_bases = {}


def hostile_base(name):
    """One clean stream per HOSTILE_BASES entry (built once per process):
    kinds, prefix, n, wire (uint8 array), rec (record starts), places."""
    if name not in _bases:
        kinds, enveloped, n, maxlen, straddle = HOSTILE_BASES[name]
        rng = np.random.default_rng(len(name) * 1000 + n)
        prefix = oracle.request_prefix("Svc::stream", "S") if enveloped else b""
        cols, offs = random_batch(kinds, n, rng, maxlen)
        if not straddle:   # cut a little past block 4097's end
            n = int(np.searchsorted(record_starts(kinds, offs, n, len(prefix)), 4098 * BLOCK + BLOCK // 2)) + 1
            cols, offs = _truncate(kinds, cols, offs, n)
        cols, offs = with_straddles(kinds, cols, offs, n, len(prefix), rng, EDGE_SPLITS.values() if straddle else ())
        wire = np.frombuffer(oracle.pack(kinds, cols, n, prefix, list(offs)), np.uint8)
        rec = record_starts(kinds, offs, n, len(prefix))
        _bases[name] = dict(kinds=kinds, prefix=prefix, n=n, wire=wire, rec=rec,
                            places=hostile_places(kinds, len(prefix), wire, rec, n, straddle))
    return _bases[name]
