"""tests/giant.py is what it says (CPU only): at a boundary of some 40 000
bytes and segments of a few KiB, the helper's wire is the oracle's pack of the
helper's concatenated inputs in one call, the oracle's unpack of it gives the
inputs back, the host windows are slices of both, and the premise assertions
fire when they are violated on purpose.
"""
import numpy as np
import pytest

import oracle
from tests import giant

torch = pytest.importorskip("torch")

I8, I16, I32, I64, BOOL, CHAR, STR = (oracle.INT8, oracle.INT16, oracle.INT32, oracle.INT64, oracle.BOOL,
                                      oracle.CHAR, oracle.STRING)
SIX = [BOOL, I8, CHAR, I16, I32, I64]
SCHEMAS = {
    "fixed": (SIX, b""),
    "envelope": (SIX, oracle.request_prefix("Svc_servicer::m", "all_kinds")),
    "one_string": ([I8, CHAR, I64, STR], b""),
    "two_strings": ([STR, I32, I8, STR], oracle.response_prefix(0, "S")),
}
SMALL = dict(device="cpu", seg_targets=(2100, 2750, 3301, 3907, 4513), seg_range=(1500, 6000), tail=8192,
             long_len=3000, win=512, margin=4096)
CASES = [(s, st) for s in SCHEMAS for st in ("short", "long") if st == "short" or STR in SCHEMAS[s][0]]


def _np(t, dtype):
    return t.numpy().view(dtype)


@pytest.mark.parametrize("zero_heavy", [False, True], ids=["random", "zero_heavy"])
@pytest.mark.parametrize("boundary", [40_003, 52_345])
@pytest.mark.parametrize("schema,straddle", CASES)
def test_wire_is_the_oracles_pack_of_the_inputs(schema, straddle, boundary, zero_heavy):
    kinds, prefix = SCHEMAS[schema]
    g = giant.build(kinds, prefix, straddle, boundary=boundary, zero_heavy=zero_heavy, **SMALL)
    every = np.concatenate([c.numpy().view(np.uint8).reshape(-1) for c in g.cols])
    zeros = float((every == 0).mean())
    assert zeros > 0.5 if zero_heavy else zeros < 0.5
    assert g.n % 2 == 1 and boundary + 8192 <= g.W < boundary + 8192 + 6000
    cols = [c.numpy() if c.numel() else np.zeros(1, np.uint8) for c in g.cols]
    offs = [None if o is None else _np(o, np.uint64) for o in g.offs]
    want = oracle.pack(kinds, cols, g.n, prefix, list(offs))
    assert g.ref.numpy().tobytes() == want
    rc, ocols, ooffs, consumed, _ = oracle.unpack(kinds, want, g.n, prefix)
    assert rc == 0 and consumed == g.W
    for f, k in enumerate(kinds):
        assert ocols[f].tobytes() == g.cols[f].numpy().tobytes(), f
        if k == STR:
            assert np.array_equal(ooffs[f], offs[f]), f
    # rec_offs: where the oracle's records begin
    fixed = giant.fixed_bytes(kinds, len(prefix))
    sizes = np.full(g.n, fixed, np.uint64)
    for o in offs:
        if o is not None:
            sizes += np.diff(o)
    rec = _np(g.rec_offs, np.uint64)
    assert rec[0] == 0 and np.array_equal(rec[1:], np.cumsum(sizes)) and int(rec[-1]) == g.W

    # the boundary byte is where the arrangement says
    r = g.rec_index
    assert int(rec[r]) + g.into == boundary and int(rec[r]) <= boundary < int(rec[r + 1])
    if straddle == "short":
        assert g.inside and r % 16 and not g.long_records
        assert int(sizes.max()) <= fixed + 2 * 40
    else:
        a, b = g.long_records
        assert r == a and int(rec[a]) < boundary < int(rec[a + 1]) and int(rec[b]) > boundary
        assert min(int(sizes[a]), int(sizes[b])) >= 3000 and np.sort(sizes)[-3] <= fixed + 2 * 40

    # the host windows are the oracle's bytes
    for lo, hi in [(0, 100), (boundary - 300, boundary + 300), (g.W - 500, g.W)]:
        assert g.wire_window(lo, hi).tobytes() == want[lo:hi]
    for f, k in enumerate(kinds):
        m = g.col_len(f)
        assert m == g.cols[f].numel()
        for lo, hi in [(0, min(m, 50)), (max(0, m - 70), m), (m // 2, min(m, m // 2 + 4000))]:
            assert g.col_window(f, lo, hi).tobytes() == g.cols[f][lo:hi].numpy().tobytes()
        if k == STR:
            for lo, hi in [(0, 9), (g.n - 5, g.n + 1), (g.n // 2, g.n // 2 + 700)]:
                assert np.array_equal(g.off_window(f, lo, hi), offs[f][lo:hi])
    for lo, hi in [(0, 9), (g.n - 5, g.n + 1), (r - 3, r + 3)]:
        assert np.array_equal(g.rec_window(lo, hi), rec[lo:hi])


def test_fixed_record_that_divides_the_boundary_is_reported():
    """16-byte records and a boundary of 2^k: the helper says that the boundary is a record boundary."""
    g = giant.build([I32] * 4, b"", "short", boundary=40_000, **SMALL)
    assert not g.inside and g.into == 0 and g.rec_index == 2500 and g.n % 2 == 1


def test_inputs_dropped_and_made_again_are_the_same():
    kinds, prefix = SCHEMAS["two_strings"]
    g = giant.build(kinds, prefix, "long", boundary=40_003, **SMALL)
    cols, offs, rec = g.cols, g.offs, g.rec_offs
    g.drop_inputs()
    assert g.cols is None and g.ref is not None
    g.upload_inputs()
    assert torch.equal(rec, g.rec_offs) and all(torch.equal(a, b) for a, b in zip(cols, g.cols))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(offs, g.offs))


def test_orders_differ_by_seed_and_are_reproducible():
    kinds, prefix = SCHEMAS["one_string"]
    a = giant.build(kinds, prefix, "short", boundary=40_003, **SMALL)
    b = giant.build(kinds, prefix, "short", boundary=40_003, **SMALL)
    c = giant.build(kinds, prefix, "short", boundary=40_003, seed=1, **SMALL)
    assert a.order == b.order and torch.equal(a.ref, b.ref)
    assert a.order != c.order


def _valid(schema="one_string", boundary=40_003):
    kinds, prefix = SCHEMAS[schema]
    return kinds, prefix, giant.build(kinds, prefix, "short", boundary=boundary, **SMALL)


def test_premise_two_equal_segments_only():
    kinds, prefix, g = _valid()
    s = g.segs[0]
    order = [0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1, 0][: 48_000 // s.nbytes + 2]
    with pytest.raises(AssertionError, match="pairwise different"):
        giant.assemble(kinds, prefix, "short", [s, s], order, 40_003, "cpu", 512, 4096)
    # and the wrap that such segments hide is seen by the wrap premise itself
    two = torch.cat([torch.from_numpy(s.wire.copy())] * 2)
    with pytest.raises(AssertionError, match="wrapped index"):
        giant.wrap_visible(two, s.nbytes, 512, "wire")


def test_premise_boundary_on_a_record_boundary():
    kinds, prefix, g = _valid()
    on = int(g.rec_window(g.rec_index + 1, g.rec_index + 2)[0])
    with pytest.raises(AssertionError, match="record boundary"):
        giant.assemble(kinds, prefix, "short", g.segs, g.order, on, "cpu", 512, 4096)


def test_premise_even_n_and_multiple_of_16():
    kinds, prefix, g = _valid("fixed")
    with pytest.raises(AssertionError, match="n is even"):
        giant.assemble(kinds, prefix, "short", g.segs, g.order + [next(i for i, s in enumerate(g.segs) if s.n % 2)],
                       40_003, "cpu", 512, 4096)
    with pytest.raises(AssertionError, match="multiple of 16"):
        giant.assemble(kinds, prefix, "short", g.segs, g.order, 17 * 16 * 150 + 5, "cpu", 512, 4096)


def test_premise_long_record_must_straddle():
    kinds, prefix = SCHEMAS["two_strings"]
    g = giant.build(kinds, prefix, "long", boundary=40_003, **SMALL)
    with pytest.raises(AssertionError, match="outside the first long record"):
        giant.assemble(kinds, prefix, "long", g.segs, g.order, 40_003 - 6000, "cpu", 512, 4096, nlong=2)
