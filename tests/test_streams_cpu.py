"""The adversarial straddler streams (tests/streams.py) are what DESIGN §4.4.1
says they are: across every 8 KiB block edge one record that starts within
`lead` bytes before the edge and ends `over` bytes past it (past the decode
table's 64-byte window), its chars zero-filled or zero-heavy.  CPU only: the
records are located with the oracle's own unpack (the reference cursor)."""
import numpy as np
import pytest

import oracle
from tests.streams import straddler_stream

KINDS = [oracle.INT8, oracle.STRING, oracle.INT16, oracle.STRING]


@pytest.mark.parametrize("lead,over,fill", [((1, 960), (65, 1000), "zero"), ((1, 900), (65, 100), "heavy"),
                                            ((1, 6000), (65, 6000), "zero")])
def test_every_block_edge_is_straddled(lead, over, fill):
    n = 30_000
    cols, offs = straddler_stream(n, np.random.default_rng(5), lead, over, fill)
    wire = bytes(oracle.pack(KINDS, cols, n, b"", offs))
    rc, ocols, ooffs, consumed, _ = oracle.unpack(KINDS, wire, n, b"")
    assert rc == oracle.ORC_OK and consumed == len(wire)
    # record starts from the field sizes: 1 + 8 + len0 + 2 + 8 + len1
    l0 = np.diff(ooffs[1].astype(np.int64))
    l1 = np.diff(ooffs[3].astype(np.int64))
    ends = np.cumsum(19 + l0 + l1)
    starts = ends - (19 + l0 + l1)
    assert ends[-1] == len(wire)
    B = 8192
    seen = 0
    while B < ends[-1] - 8192:
        r = int(np.searchsorted(ends, B, side="right"))  # the record that holds byte B
        if starts[r] == B:  # a record starting exactly at the edge is no straddler
            B += 8192
            continue
        # (the last ordinary record ends at most `lead` before the edge, so
        # the straddler starts up to one ordinary record, <= 65 bytes, earlier)
        assert B - starts[r] <= lead[1] + 65, (B, starts[r])
        # it ends past the table window (or, for the long leads, the record
        # spans more than one edge: the next edge is inside it)
        assert ends[r] - B >= over[0] or ends[r] > B + 8192, (B, ends[r])
        if fill == "zero":
            s0 = int(ooffs[1][r])
            assert not ocols[1][s0:s0 + int(l0[r])].any()  # zero-filled chars
        seen += 1
        B += 8192
    assert seen >= (ends[-1] // 8192) // 2


# ---- the generators behind tests/test_gpu_stream_hostile.py ----------------
# Each condition below is one the GPU tests rely on to reach the code they are
# about; the oracle alone decides them.

from tests import streams  # noqa: E402

NESTED = {"zh4": (KINDS, b""), "bare": ([oracle.STRING], b""),
          "enveloped": ([oracle.INT32, oracle.STRING, oracle.INT8], oracle.request_prefix("Svc::nested", "N"))}


@pytest.mark.parametrize("schema", list(NESTED))
def test_nested_stream_has_far_entries_and_wrong_chains(schema):
    kinds, prefix = NESTED[schema]
    n = 600
    cols, offs = streams.nested_stream(kinds, n, np.random.default_rng(17), prefix=prefix)
    wire = oracle.pack(kinds, cols, n, prefix, offs)
    rc, _, ooffs, consumed, _ = oracle.unpack(kinds, wire, n, prefix)
    assert rc == oracle.ORC_OK and consumed == len(wire)
    rec = streams.record_starts(kinds, ooffs, n, len(prefix))
    assert rec[n] == len(wire)
    blocks = (len(wire) + streams.BLOCK - 1) // streams.BLOCK
    share = streams.far_entries(rec, len(wire)).size / blocks
    print(f"{schema}: {len(wire)} bytes, {blocks} blocks, far-entry share {share:.3f}")
    assert share >= 0.30
    # inside every long string some position parses as two records in a row
    f0 = kinds.index(oracle.STRING)
    at = rec[:n].astype(np.int64) + streams.first_len_at(kinds, len(prefix)) + 8   # the long strings' chars
    lens = np.diff(ooffs[f0].astype(np.int64))
    for r in range(n):
        lo, hi = int(at[r]), int(at[r] + lens[r])
        for p in range(lo, lo + 2048):
            rc, _, _, used, _ = oracle.unpack(kinds, wire[p:p + 1024], 2, prefix)
            if rc == oracle.ORC_OK and p + used <= hi:
                break
        else:
            raise AssertionError(f"record {r}: no wrong chain in its string")


FAN_PAIRS = 12   # fan blocks 9, 14, ..., 64: the last is a scan group's first block


@pytest.mark.parametrize("T", [701, 9])
def test_fan_stream_overflows_the_exit_slots(T):
    wire, n, fans = streams.fan_stream(FAN_PAIRS, np.random.default_rng(3), T=T)
    rc, _, ooffs, consumed, _ = oracle.unpack([oracle.STRING], wire.tobytes(), n, b"")
    assert rc == oracle.ORC_OK and consumed == wire.size
    rec = streams.record_starts([oracle.STRING], ooffs, n)
    assert any(c % 64 == 0 for c in fans), fans
    for c in fans:
        live = streams.live_exits(wire, c)
        past = live[live >= c * streams.BLOCK + streams.WINDOW]
        entry = int(rec[np.searchsorted(rec, c * streams.BLOCK)])   # the first record start in block c
        assert entry == c * streams.BLOCK + 8 * T and entry in past
        assert past.size >= 256, (c, past.size)
        if T == 701:
            assert entry not in past[:streams.SLOTS], c   # the true entry is not a kept slot
        else:
            assert entry in past[:streams.SLOTS], c
    print(f"T={T}: {wire.size} bytes, {n} records, fan blocks {fans}, live exits past the window "
          f"{[int((streams.live_exits(wire, c) >= c * streams.BLOCK + 64).sum()) for c in fans]}")


@pytest.mark.parametrize("base", list(streams.HOSTILE_BASES))
def test_hostile_cases_are_what_their_names_say(base):
    b = streams.hostile_base(base)
    kinds, prefix, wire, rec, n = b["kinds"], b["prefix"], b["wire"], b["rec"], b["n"]
    rc, _, ooffs, consumed, _ = oracle.unpack(kinds, wire.tobytes(), n, prefix)
    assert rc == oracle.ORC_OK and consumed == wire.size
    assert np.array_equal(rec, streams.record_starts(kinds, ooffs, n, len(prefix)))
    blocks = (wire.size + streams.BLOCK - 1) // streams.BLOCK
    want_places = {"first", "last"}
    if base != "bare_32m":
        want_places |= set(streams.EDGE_SPLITS)
    if base in ("bare_two_str", "five_str"):
        assert blocks > 128
        want_places |= {"group1_first_block", "group1_last_block"}
    if base == "bare_32m":
        assert 4098 < blocks <= 4100 and 15_000 < n < 25_000
        want_places |= {"group1_first_block", "group1_last_block", "block_4095", "block_4096", "block_4097"}
    assert set(b["places"]) == want_places
    at = rec[:n].astype(np.int64) + streams.first_len_at(kinds, len(prefix))
    for name, res in streams.EDGE_SPLITS.items():
        if name in b["places"]:   # the 8 bytes of that length field lie across the edge
            a = int(at[b["places"][name]])
            edge = (a + 7) // streams.BLOCK * streams.BLOCK + (streams.MARGIN if "margin" in name else 0)
            assert a < edge < a + 8 and edge - a == int(name.split("_")[1]), (name, a)
    for name, blk in (("group1_first_block", 64), ("block_4095", 4095), ("block_4096", 4096), ("block_4097", 4097)):
        if name in b["places"]:
            assert int(rec[b["places"][name]]) // streams.BLOCK == blk
    cases = streams.hostile_cases(kinds, prefix, wire, rec, n, b["places"])
    kinds_seen = {}
    for c in cases:
        verdict = streams.oracle_on_case(kinds, prefix, wire, rec, c)[0]
        assert verdict == c.want, (c.name, verdict)
        # and, on the small streams, without the shortcut of starting the oracle late
        if wire.size < 1 << 21:
            rc, _, _, consumed, err = oracle.unpack(kinds, streams.patched(wire, c).tobytes(), c.n, prefix)
            assert (streams.ORC_NAME[rc], err, consumed) == c.want, c.name
        place, kind = c.name.split("->")[0].split("/")
        kinds_seen.setdefault(place, set()).add(kind)
    strs = kinds.count(oracle.STRING)
    expect = {"string_ends_at_wire_len", "cut_length", "cut_chars", "cut_at_record_start"}
    expect |= {f"{w}_len_{v}" for w in (["first_str", "last_str"] if strs > 1 else ["first_str"])
               for v in ("past_by_1", "2^32", "2^63", "2^64-1", "wraps")}
    expect |= {"cut_fixed"} | ({"flip_prefix", "cut_prefix"} if prefix else set())
    for place in want_places:
        assert kinds_seen[place] == expect, (place, expect ^ kinds_seen[place])
