"""The pairs of tests/scratch_cases.py are what their names say, proven from
the generated data and the oracle alone (no GPU): every batch lies in the band
it names -- the input property that selects the host branch of
srpc_gpu_pack_var / _unpack_var -- predecessor and call differ in everything a
stale scratch word could carry, errored predecessors are errors to the oracle,
and an "inexact index" disagrees with the decoded lengths."""
import functools

import numpy as np
import pytest

import oracle
from tests import scratch_cases as sc
from tests import var_cases as vc

PAIRS = sc.all_pairs()


@functools.lru_cache(maxsize=None)
def facts(b):
    """(kinds, n, wire bytes, chars per string field, longest string, wire, rec_offs)."""
    kinds, cols, offs = sc.make(b)
    wire = oracle.pack(kinds, cols, b.n, b"", list(offs))
    rec = vc.rec_offsets(kinds, offs, b.n)
    assert int(rec[b.n]) == len(wire)
    longest = max(int(np.diff(o.astype(np.int64)).max()) for o in offs if o is not None)
    return kinds, b.n, len(wire), sc.chars_totals(offs), longest, wire, rec


def all_batches():
    seen = {}
    for p in PAIRS:
        for b in sc.batches_of(p):
            seen[b] = None
    for b in list(sc.SERVER["request"]) + [sc.SERVER["response"], sc.STALLED]:
        seen[b] = None
    return list(seen)


def test_names_are_unique_and_sizes_are_the_issues():
    names = [p.name for p in PAIRS]
    assert len(set(names)) == len(names)
    for p in PAIRS:
        assert p.b.batch.n in (257, 513, 4099, 16_641), p.name
        assert p.a.batch is None or p.a.batch.n <= 30_001, p.name
    big = {(p.b.op, p.b.batch) for p in PAIRS if p.b.batch.n == 16_641}  # the one 65-tile case
    assert big == {("unpack", sc.STALLED)} and 16_641 // 256 == 65  # 65 full tiles and a record: two 64-tile blocks
    assert {p.a.arg for p in PAIRS if p.a.kind == "fill"} == {0x00, 0xFF, 0x5A}
    # 0x5A reads as a published aggregate, 0xA5 and 0xFF as a published inclusive, 0x00 as nothing
    assert int.from_bytes(b"\x5a" * 8, "little") >> 62 == 1 and int.from_bytes(b"\xa5" * 8, "little") >> 62 == 2


@pytest.mark.parametrize("b", all_batches(), ids=sc.label)
def test_batch_is_in_its_band(b):
    kinds, n, total, chars, longest, _, _ = facts(b)
    lo, hi = sc.BANDS[b.band]
    assert lo <= total // n < hi, (total // n, b.band)
    assert len(chars) == b.nstr and len(sc.str_fields(kinds)) == b.nstr
    if b.gen == "wide":
        assert kinds == vc.WIDE
    # the record tiles' LDS image: the pack takes them while avg * 256 * 17/16 + 64 fits 15/16 of 64 KiB
    fits = (total // n) * 256 * 17 // 16 + 64 <= 65536 * 15 // 16
    assert fits == (b.band != "gt255")


@pytest.mark.parametrize("p", PAIRS, ids=lambda p: p.name)
def test_pair_is_what_it_says(p):
    kinds_b, n_b, total_b, chars_b, longest_b, _, _ = facts(p.b.batch)
    if "all short" in p.branch:
        assert longest_b <= sc.SHORT_COPY
    if "some long" in p.branch:
        assert longest_b > sc.SHORT_COPY
    if p.b.op == "pack":
        # one string field: the pack that writes rec_offs without a scan; more: the scan
        assert ("short_records<true>" in p.branch) == (p.b.batch.nstr == 1 and (p.b.vk == 0 or p.b.batch.band == "gt255"))
        assert p.branch.startswith("rt ") == (p.b.vk is None and p.b.batch.band != "gt255")
        if "rpl=2" in p.branch:
            assert p.b.batch.band == "lt20"
        if "rpl=1" in p.branch:
            assert p.b.batch.band == "20-40"
        if "rt loop" in p.branch:
            assert p.b.batch.band == "40-200"
    else:
        avg = total_b // n_b
        tiles = p.b.vk == 2 or (p.b.vk is None and 40 <= avg and avg * 256 * 17 // 16 + 64 <= 49152)
        assert ("unpack_var_rt" in p.branch) == tiles, (avg, p.branch)
        if "rt<true>" in p.branch or "str1_tail" in p.branch or "scan1" in p.branch:
            assert p.b.batch.nstr == 1
        if "scans" in p.branch:
            assert p.b.batch.nstr > 1
        if "str1_tail" in p.branch:
            assert avg <= vc.fixed_bytes(kinds_b) + sc.SHORT_COPY
        if "scan1" in p.branch:
            assert avg > vc.fixed_bytes(kinds_b) + sc.SHORT_COPY
        if "walk<true,2>" in p.branch:
            assert avg <= 20
        if "lookback" in p.name or p.b.op == "tiled":
            assert p.b.batch.nstr > 1
    if p.b.op == "unpack_inexact":
        assert_inexact(p.b.batch)
    if p.a.kind == "fill":
        return
    # nothing stale can equal the right value by accident
    kinds_a, n_a, total_a, chars_a, longest_a, wire_a, rec_a = facts(p.a.batch)
    assert n_a != n_b and total_a != total_b
    assert not set(chars_a) & set(chars_b), (chars_a, chars_b)
    if p.name.endswith("after-larger") or p.name.endswith("after-larger-pack") or "-after-near" in p.name:
        assert n_a > n_b
    if "-after-near" in p.name and p.a.batch._replace(n=0) == p.b.batch._replace(n=0):
        assert sc.layout_class(p.a.batch) == sc.layout_class(p.b.batch) and n_a - n_b <= 7
    if p.name.endswith("after-larger") or p.name.endswith("after-larger-pack"):
        assert n_a > n_b and total_a > total_b
        assert p.a.batch.band != p.b.batch.band or p.b.op != "pack"
        assert p.a.batch.nstr != p.b.batch.nstr
    if p.name.endswith("after-unpack"):
        assert kinds_a != kinds_b  # a different plan
    if p.name == "pack-all-short-after-long-flags" or p.name.endswith("long-tiles"):
        assert longest_a > sc.SHORT_COPY and p.a.batch.nstr == 1 and p.a.vk == 0
    if p.name == "pack-some-long-after-all-short":
        assert longest_a <= sc.SHORT_COPY
    # errored predecessors are errors to the oracle
    if p.a.kind == "pack_bounds":
        cap = sc.bounds_cap(total_a)
        assert 0 < cap < total_a  # the oracle's pack (facts) needs total_a bytes: more than the wire_cap given
        r = int(np.searchsorted(rec_a, cap, side="right")) - 1
        assert 0 < r < n_a - 1 and int(rec_a[r]) < cap  # ... and the cut lies inside the batch
    if p.a.kind == "unpack_bounds":
        bad, r = sc.bounds_wire(kinds_a, wire_a, rec_a, n_a)
        rc, _, _, _, err = oracle.unpack(kinds_a, bad, n_a, b"")
        assert rc == oracle.ORC_ERR_BOUNDS and err == r
    if p.a.kind == "unpack_inexact":
        assert_inexact(p.a.batch)
    if p.a.kind == "tiled" and p.a.arg != "right" or p.b.op == "tiled" and p.b.arg != "right":
        which, how = (p.a.batch, p.a.arg) if p.a.kind == "tiled" and p.a.arg != "right" else (p.b.batch, p.b.arg)
        _, cols, offs = sc.make(which)
        ns = which.nstr
        at = np.minimum(np.arange(-(-which.n // 256) + 1) * 256, which.n)
        right = np.stack([o[at] - o[0] for o in offs if o is not None], axis=1).reshape(-1).astype(np.uint64)
        wrong = sc.wrong_table(right, how, ns)
        assert wrong.size == right.size and (wrong != right).any()


def assert_inexact(b):
    """At least one record whose index size disagrees with its decoded lengths."""
    kinds, n, total, _, _, wire, rec = facts(b)
    rc, _, ooffs, consumed, _ = oracle.unpack(kinds, wire, n, b"")
    assert rc == oracle.ORC_OK and consumed == total
    idx = sc.inexact_index(rec, n)
    decoded = np.full(n, vc.fixed_bytes(kinds), np.int64)
    for o in ooffs:
        if o is not None:
            decoded += np.diff(o.astype(np.int64))
    sizes = np.diff(idx.astype(np.int64))
    assert (sizes != decoded).sum() >= 1
    assert (np.diff(rec.astype(np.int64)) == decoded).all()  # the right index is exact
    assert (sizes >= 0).all() and int(idx[n]) == total  # still monotonic and inside the wire


def test_server_sequence_and_stalled_batches():
    r1, r2 = sc.SERVER["request"]
    resp = sc.SERVER["response"]
    assert r1.nstr == r2.nstr and r1.band == r2.band and r1.n != r2.n  # one request plan, two batches
    assert resp.nstr != r1.nstr                                        # another plan
    assert max(r1.n, r2.n, resp.n) == sc.SERVER["max_n"]
    f1, f2, fr = facts(r1), facts(r2), facts(resp)
    assert len({f1[2], f2[2], fr[2]}) == 3
    assert not set(f1[3]) & set(f2[3]) and not set(fr[3]) & (set(f1[3]) | set(f2[3]))
    s = sc.STALLED
    assert s.nstr > 1 and -(-s.n // 256) > 64 and 40 <= facts(s)[2] // s.n < 180  # look-back tiles, two levels


def test_every_named_branch_has_a_pair():
    branches = {p.branch for p in PAIRS}
    for want in ("rt rpl=2", "rt rpl=1", "rt loop", "short_records<true> all short + pack_var<true>",
                 "short_records<true> some long + pack_var<true>", "scan + pack_var<false>",
                 "unpack_var_rt<true> stays exact", "unpack_var_rt<true> + gated look-back pass",
                 "zero_u64 + unpack_var_rt<false> look-back", "unpack_var_rt<false> table, no second pass",
                 "unpack_var_rt<false> table + gated look-back pass", "walk<true,2> + str1_tail",
                 "walk<true,1> + str1_tail", "walk<true,1> + scan1 + chars", "walk + scan1 + chars",
                 "walk + scans + chars_multi"):
        assert want in branches, want
    # the all-short / some-long flags both ways round
    names = {p.name for p in PAIRS}
    assert {"pack-all-short-after-long-flags", "pack-some-long-after-all-short"} <= names
    # (the several-string scan WITH the short-records pass cannot be reached: it
    # needs fixed_bytes + 32 * nstrings <= 64, and two length words alone are 16)
    assert min(vc.fixed_bytes(k) + sc.SHORT_COPY * sum(x == oracle.STRING for x in k)
               for k in (vc.SCHEMAS[2], vc.SCHEMAS[3], vc.WIDE, [oracle.STRING, oracle.STRING])) > 64
