"""The string batches of tests/var_cases.py are in the regimes they claim,
proven from the generated data alone (no GPU, no kernel-selection rule
restated), and the oracle packs and unpacks every one of them."""
import numpy as np
import pytest

import oracle
from tests import var_cases as vc


def _spans(kinds, offs, n, prefix_len=0):
    """Wire bytes of every aligned 256-record tile."""
    rec = vc.rec_offsets(kinds, offs, n, prefix_len).astype(np.int64)
    edges = np.append(np.arange(0, n, vc.TILE), n)
    return np.diff(rec[edges])


def _roundtrip(kinds, cols, offs, n, prefix=b""):
    wire = oracle.pack(kinds, cols, n, prefix, list(offs))
    assert len(wire) == int(vc.rec_offsets(kinds, offs, n, len(prefix))[n])
    rc, ocols, ooffs, consumed, _ = oracle.unpack(kinds, wire, n, prefix)
    assert rc == oracle.ORC_OK and consumed == len(wire)
    for f, k in enumerate(kinds):
        if k == oracle.STRING:
            o = np.asarray(offs[f], np.uint64)
            assert np.array_equal(ooffs[f], o - o[0])
            assert ocols[f].tobytes() == cols[f][:int(o[n] - o[0])].tobytes()
        else:
            assert ocols[f].tobytes() == cols[f].tobytes()
    return wire


@pytest.mark.parametrize("n", vc.SLACK_SIZES)
@pytest.mark.parametrize("b", range(3))
def test_uniform_average_in_band(b, n):
    lo, hi = vc.BANDS[b]
    kinds, cols, offs = vc.uniform(vc.BANDS[b], n, (1, 2, 3)[b])
    total = int(vc.record_sizes(kinds, offs, n).sum())
    assert lo * n <= total < hi * n  # the exact average, fixed bytes included
    if n >= 255:
        for k, o in zip(kinds, offs):
            if k == oracle.STRING:
                assert (np.diff(o.astype(np.int64)) == 0).any()  # empty strings occur
    _roundtrip(kinds, cols, offs, n)
    # deterministic
    again = vc.uniform(vc.BANDS[b], n, (1, 2, 3)[b])
    assert all(a.tobytes() == c.tobytes() for a, c in zip(cols, again[1]))


def test_uniform_with_prefix_counts_the_prefix():
    pre = oracle.request_prefix("Svc_servicer::m", "S")
    kinds, cols, offs = vc.uniform((40, 200), 4099, 1, len(pre))
    total = len(_roundtrip(kinds, cols, offs, 4099, pre))
    assert 40 * 4099 <= total < 200 * 4099


@pytest.mark.parametrize("which", sorted(vc.HEAVY))
def test_heavy_tail_regime(which):
    n, nstr, longs = vc.HEAVY[which]
    kinds, cols, offs = vc.heavy_tail(which)
    sidx = [f for f, k in enumerate(kinds) if k == oracle.STRING]
    assert len(sidx) == nstr and nstr == {"low": 2, "mid": 3}[which]
    lens = np.stack([np.diff(offs[f].astype(np.int64)) for f in sidx])
    assert (lens <= 8).mean() >= 0.9
    assert lens.max() > 65536
    total = int(vc.record_sizes(kinds, offs, n).sum())
    avg = total / n
    assert avg < 40 if which == "low" else 40 <= avg < 200
    spans = _spans(kinds, offs, n)
    assert spans.max() > 4 * vc.TILE * avg
    # the long strings sit in different fields of different tiles, and a tile
    # next to a long one is an ordinary short tile
    where = {(int(r) // vc.TILE, int(s)) for s, r in zip(*np.nonzero(lens > 256))}
    assert len({t for t, _ in where}) == len(where) >= 5
    assert len({s for _, s in where}) == nstr
    assert (spans[:-1] < 2 * vc.TILE * vc.fixed_bytes(kinds)).sum() >= len(spans) // 2
    _roundtrip(kinds, cols, offs, n)


@pytest.mark.parametrize("nstr", [2, 3])
@pytest.mark.parametrize("n", [4099, 30_001])
def test_bursts_regime(n, nstr):
    kinds, cols, offs = vc.bursts(n, nstr)
    sizes = vc.record_sizes(kinds, offs, n).astype(np.int64)
    fixed = vc.fixed_bytes(kinds)
    empty = sizes == fixed
    assert ((sizes > 270) & (sizes < 330))[~empty].all()  # the other records are near 300 bytes
    # runs of empty records: 256..600 long (the batch's last run may be cut)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], empty.astype(np.int8), [0]])))
    runs = edges[1::2] - edges[0::2]
    assert len(runs) >= 5
    inner = runs[:-1] if empty[-1] else runs
    assert (inner >= 256).all() and (runs <= 600).all()
    # consecutive aligned tiles switch regimes: a tile of mostly long records
    # beside a tile of mostly empty ones
    spans = _spans(kinds, offs, n)[:-1]
    ratio = np.maximum(spans[1:], spans[:-1]) / np.minimum(spans[1:], spans[:-1])
    assert (ratio > 4).sum() >= 3
    _roundtrip(kinds, cols, offs, n)


def test_bursts_small_sizes_roundtrip():
    for n in vc.SLACK_SIZES:
        kinds, cols, offs = vc.bursts(n)
        _roundtrip(kinds, cols, offs, n)


def test_based_is_the_same_batch_shifted():
    case = vc.heavy_tail("mid")
    kinds, cols, boffs, bases = vc.based(case)
    assert [b for b in bases if b is not None] == [1, 4093, 2**32 + 5]
    n = vc.HEAVY["mid"][0]
    for f, k in enumerate(kinds):
        if k != oracle.STRING:
            assert boffs[f] is None and bases[f] is None
            continue
        assert boffs[f].dtype == np.uint64 and int(boffs[f][0]) == bases[f] != 0
        assert np.array_equal(boffs[f] - np.uint64(bases[f]), case[2][f])
        # addressed from a column pointer moved back by the base, the chars are the same bytes
        assert int(boffs[f][n]) - bases[f] <= cols[f].size
    assert vc.rec_offsets(kinds, boffs, n).tobytes() == vc.rec_offsets(kinds, case[2], n).tobytes()
    # the oracle reads absolute offsets too: chars column moved forward by a small base
    small = vc.based(case, bases=(1, 7, 64))
    moved = [np.concatenate([np.zeros(b, np.uint8), c]) if b else c for c, b in zip(cols, small[3])]
    assert oracle.pack(kinds, moved, n, b"", list(small[2])) == oracle.pack(kinds, cols, n, b"", list(case[2]))


def test_wide_schema_roundtrip():
    kinds, cols, offs = vc.wide(4099)
    assert kinds.count(oracle.INT64) == 16 and kinds.count(oracle.STRING) == 4
    total = len(_roundtrip(kinds, cols, offs, 4099))
    assert total // 4099 < 225


def test_slack_capacities_cross_every_threshold():
    """The slack test's capacities put wire_cap / n on both sides of 20, 40 and
    the record tiles' ~240-byte limit for at least one batch each (from the
    batches' bytes alone), and every batch keeps its exact-capacity run."""
    crossed = {20: 0, 40: 0, 240: 0}
    names = set()
    for name, make in vc.slack_batches():
        kinds, cols, offs = make()
        n = len(cols[0]) if offs[0] is None else len(offs[0]) - 1
        total = int(vc.record_sizes(kinds, offs, n).sum())
        caps = vc.slack_caps(total)
        assert caps[0] == ("exact", total) and len(caps) == 6 and caps[-1][1] == 64 * total, name
        names.add(name)
        q = [cap // n for _, cap in caps]
        for t in crossed:
            # strictly apart from the threshold, so an off-by-one in the rule still crosses
            crossed[t] += min(q) < t - 2 and max(q) > t + 2 and n >= 255
    assert len(names) == 4 * len(vc.SLACK_SIZES) + 2
    assert all(v >= 3 for v in crossed.values()), crossed
