"""Pairs "predecessor A, then call under test B" for the scratch-reuse tests
(pure numpy and plain data: run by tests/test_gpu_scratch_reuse.py, proven to
be what their names say by tests/test_scratch_cases_cpu.py).

Every call that takes d_scratch keeps per-call state there, and in production
the scratch is whatever the call before left: batch_server runs the unpack of
one schema and the pack of another through one buffer, batch after batch.  A
pair names the call that dirties the scratch (A) and the call whose outputs
are checked (B).  A and B differ in n, in their wire bytes and in every string
field's chars, so no stale word can equal the right one by accident.

Batches are the generators of tests/var_cases.py by name (`Batch`), so a pair
is a few strings and numbers; `make` turns a Batch into (kinds, cols, offs).
The bands are the host branches of srpc_gpu_pack_var / _unpack_var, keyed by
the average record bytes wire_bytes // n (prefix and length words included).
"""
import functools
from collections import namedtuple

import numpy as np

import oracle
from tests import var_cases as vc

# average record bytes [lo, hi) per band name
BANDS = {
    "lt20": (0, 20),        # two records per lane
    "20-40": (20, 40),      # tiles without the persistent loop; the walk for unpack
    "40-200": (40, 201),    # record tiles, persistent pack loop
    "gt255": (256, 1 << 62),  # over 240 * 17/16: the span does not fit the LDS image
}
FILLS = (0x00, 0xFF, 0x5A)  # 0x5A: top bits 01, a u64 of it reads as a published aggregate
SHORT_COPY = 32             # strings up to this long are "short" to the walk kernels

# gen: uniform | long | wide; nstr: string fields (var_cases.SCHEMAS; wide has 4)
Batch = namedtuple("Batch", "gen n nstr band")
# kind: fill (arg: the byte) | pack | pack_bounds | unpack | unpack_inexact |
#       unpack_bounds | tiled (arg: "right", or how the table is wrong)
# vk: var_kernel of A's plan (None: the default)
Pred = namedtuple("Pred", "kind batch vk arg")
# op: pack | unpack | unpack_inexact | tiled (arg as in Pred)
Call = namedtuple("Call", "op batch vk arg")
Pair = namedtuple("Pair", "name a b branch")

_UNIFORM_BAND = {("lt20", 1): (12, 20), ("20-40", 1): (20, 40), ("20-40", 2): (20, 40), ("20-40", 3): (36, 40),
                 ("40-200", 1): (40, 200), ("40-200", 2): (40, 200), ("40-200", 3): (40, 200)}


def long_records(n, nstr):
    """Strings uniform in [0, 800 / nstr]: records of about 400 bytes."""
    kinds = list(vc.SCHEMAS[nstr])
    rng = np.random.default_rng([17, n, nstr])
    return vc._batch(kinds, [rng.integers(0, 800 // nstr + 1, n) for _ in range(nstr)], n, rng)


def make(b):
    if b.gen == "uniform":
        return vc.uniform(_UNIFORM_BAND[(b.band, b.nstr)], b.n, b.nstr)
    if b.gen == "long":
        return long_records(b.n, b.nstr)
    if b.gen == "wide":
        return vc.wide(b.n)
    raise KeyError(b.gen)


def label(b):
    return f"{b.gen}{b.nstr}s_{b.band}_n{b.n}"


def str_fields(kinds):
    return [f for f, k in enumerate(kinds) if k == oracle.STRING]


def chars_totals(offs):
    return [int(o[-1] - o[0]) for o in offs if o is not None]


def inexact_index(rec, n):
    """The record index with one inner boundary moved by a byte: records
    n // 3 - 1 and n // 3 then have sizes that disagree with their lengths."""
    out = np.array(rec, np.uint64)
    out[n // 3] += 1
    return out


def bounds_wire(kinds, wire, rec, n, prefix_len=0):
    """The wire with record n // 2's first string length pointing far past
    the record (and the wire).  Returns (bytes, the record)."""
    r = n // 2
    f = str_fields(kinds)[0]
    at = int(rec[r]) + prefix_len + sum(oracle.KIND_SIZE[k] for k in kinds[:f])
    w = bytearray(wire)
    w[at:at + 8] = (1 << 40).to_bytes(8, "little")
    return bytes(w), r


def bounds_cap(total):
    """A wire_cap short of the batch, near two thirds of it."""
    return total * 2 // 3 + 5


def wrong_table(table, how, ns):
    """A tile table (u64, tile-major, ns words per tile) made wrong as
    tests/test_gpu_tiled.py does."""
    t = np.array(table, np.uint64)
    if how == "one_entry_off_by_one":
        t[ns * (t.size // ns // 2) + ns - 1] += 1
    elif how == "zeros":
        t[:] = 0
    else:
        raise KeyError(how)
    return t


def U(band, n, nstr):
    return Batch("uniform", n, nstr, band)


# the large predecessors (30 001 records: at most that many)
A_S1_LT20 = U("lt20", 30_001, 1)       # every string short
A_S1_MID = U("40-200", 30_001, 1)      # strings up to 220 bytes: long flags, long tiles
A_S2_2040 = U("20-40", 30_001, 2)
A_S2_MID = U("40-200", 30_001, 2)
A_S3_MID = U("40-200", 30_001, 3)


def _fills(name, call, branch):
    return [Pair(f"{name}-after-fill{v:02x}", Pred("fill", None, None, v), call, branch) for v in FILLS]


def pack_pairs():
    """srpc_gpu_pack_var.  The record tiles keep nothing in the scratch (they
    do not take it), so a predecessor pack runs with var_kernel 0 -- the walk,
    which writes partials, tile starts and the long flags."""
    out = []
    # (B, the larger A of another band and schema, branch under the default, branch under var_kernel 0)
    rows = [
        (U("lt20", 4099, 1), A_S3_MID, "rt rpl=2", "short_records<true> all short + pack_var<true>"),
        (U("20-40", 257, 1), A_S3_MID, "rt rpl=1", "short_records<true> some long + pack_var<true>"),
        (U("20-40", 513, 2), A_S1_MID, "rt rpl=1", "scan + pack_var<false>"),
        (U("20-40", 4099, 3), A_S1_LT20, "rt rpl=1", "scan + pack_var<false>"),
        (U("40-200", 4099, 1), A_S2_2040, "rt loop", "short_records<true> some long + pack_var<true>"),
        (U("40-200", 513, 2), A_S1_LT20, "rt loop", "scan + pack_var<false>"),
        (U("40-200", 257, 3), A_S1_LT20, "rt loop", "scan + pack_var<false>"),
        (Batch("wide", 513, 4, "40-200"), A_S1_LT20, "rt loop", "scan + pack_var<false>"),
        (Batch("long", 257, 1, "gt255"), A_S3_MID, "short_records<true> some long + pack_var<true>", None),
        (Batch("long", 513, 2, "gt255"), A_S1_LT20, "scan + pack_var<false>", None),
        (Batch("long", 4099, 3, "gt255"), A_S1_MID, "scan + pack_var<false>", None),
    ]
    for b, big, br_default, br_walk in rows:
        for vk, branch in ((None, br_default), (0, br_walk or br_default)):
            call = Call("pack", b, vk, None)
            name = f"pack-{label(b)}-vk{vk}"
            out += _fills(name, call, branch)
            out.append(Pair(f"{name}-after-larger-pack", Pred("pack", big, 0, None), call, branch))
            out.append(Pair(f"{name}-after-bounds-pack", Pred("pack_bounds", big, 0, None), call, branch))
            out.append(Pair(f"{name}-after-unpack", Pred("unpack", big, 0, None), call, branch))
    # the single-string walk's long flags, both ways round
    short_b, long_b = U("lt20", 513, 1), U("40-200", 257, 1)
    out.append(Pair("pack-all-short-after-long-flags", Pred("pack", A_S1_MID, 0, None), Call("pack", short_b, 0, None),
                    "short_records<true> all short + pack_var<true>"))
    out.append(Pair("pack-some-long-after-all-short", Pred("pack", A_S1_LT20, 0, None), Call("pack", long_b, 0, None),
                    "short_records<true> some long + pack_var<true>"))
    return out


def _round256(x):
    return (x + 255) & ~255


@functools.lru_cache(maxsize=None)
def layout_class(b):
    """What places the regions of the unpack scratch (var.hip, scratch_layout):
    the scan blocks of 2048 records, the tile starts of every string field
    (one per 4 KiB of wire, two spare) and the lens / spos arrays, each
    rounded up to 256 bytes."""
    kinds, _, offs = make(b)
    total = int(vc.rec_offsets(kinds, offs, b.n)[b.n])
    return -(-b.n // 2048), _round256(8 * (total // 4096 + 2) * b.nstr), _round256(8 * b.nstr * b.n)


@functools.lru_cache(maxsize=None)
def near(b):
    """The same kind of batch a few records longer, with b's layout_class:
    its scratch puts every region where b's call has it, so the flags, tickets
    and look-back words it leaves lie exactly on the words b's call reads."""
    for d in (5, 4, 3, 6, 2, 7, 1):
        c = b._replace(n=b.n + d)
        if layout_class(c) == layout_class(b):
            return c
    raise ValueError(f"no near batch for {b}")


def unpack_pairs():
    """srpc_gpu_unpack_var and _unpack_var_tiled.  Two predecessors per call:
    "near" -- the same path on a batch a few records longer (`near`), whose flags,
    tickets and look-back words land on the call's own -- and "larger" -- a
    30 001-record batch through the walk (var_kernel 0), whose lengths,
    positions and partials cover the whole of the call's scratch.  (The record
    tiles of a large batch keep their words behind its lens / spos regions,
    past the end of a small call's scratch: they would leave it untouched.)"""
    out = []

    def add(name, a, b, branch, fills=True):
        out.append(Pair(name, a, b, branch))
        if fills:
            out.extend(_fills(name.split("-after-")[0], b, branch))

    # single string, record tiles: the optimistic pass, exact after inexact and the reverse
    for vk in (None, 2):
        bb = U("40-200", 4099, 1)
        b = Call("unpack", bb, vk, None)
        br = "unpack_var_rt<true> stays exact"
        add(f"unpack1-exact-vk{vk}-after-near-inexact", Pred("unpack_inexact", near(bb), vk, None), b, br)
        add(f"unpack1-exact-vk{vk}-after-larger-inexact", Pred("unpack_inexact", A_S1_MID, 0, None), b, br, fills=False)
        bb = U("40-200", 513, 1)
        b = Call("unpack_inexact", bb, vk, None)
        br = "unpack_var_rt<true> + gated look-back pass"
        add(f"unpack1-inexact-vk{vk}-after-near-exact", Pred("unpack", near(bb), vk, None), b, br)
        add(f"unpack1-inexact-vk{vk}-after-larger", Pred("unpack", A_S2_MID, 0, None), b, br, fills=False)
    # ... and for short records, which only var_kernel 2 gives to the record tiles
    bb = U("lt20", 513, 1)
    add("unpack1-exact-short-vk2-after-near-inexact", Pred("unpack_inexact", near(bb), 2, None),
        Call("unpack", bb, 2, None), "unpack_var_rt<true> stays exact")
    # several strings: the look-back, 65 tiles (second-level words) and small batches
    for vk in (None, 2):
        for bb, big in ((U("40-200", 16_641, 2), A_S3_MID), (U("40-200", 513, 2), A_S3_MID),
                        (U("40-200", 257, 3), A_S2_MID), (U("40-200", 4099, 3), A_S2_MID)):
            b = Call("unpack", bb, vk, None)
            br = "zero_u64 + unpack_var_rt<false> look-back"
            add(f"unpackN-lookback-{label(bb)}-vk{vk}-after-near", Pred("unpack", near(bb), vk, None), b, br,
                fills=bb.n != 4099)
            add(f"unpackN-lookback-{label(bb)}-vk{vk}-after-larger", Pred("unpack", big, 0, None), b, br, fills=False)
    add("unpackN-lookback-after-pack-walk", Pred("pack", A_S1_MID, 0, None),
        Call("unpack", U("40-200", 4099, 3), None, None), "zero_u64 + unpack_var_rt<false> look-back", fills=False)
    # tiled: a right table after a wrong one, and the reverse
    for vk in (None, 2):
        for how in ("one_entry_off_by_one", "zeros"):
            bb = U("40-200", 4099, 2)
            add(f"tiled-right-vk{vk}-after-near-{how}", Pred("tiled", near(bb), vk, how),
                Call("tiled", bb, vk, "right"), "unpack_var_rt<false> table, no second pass", fills=how == "zeros")
            bb = U("40-200", 513, 2)
            add(f"tiled-{how}-vk{vk}-after-near-right", Pred("tiled", near(bb), vk, "right"),
                Call("tiled", bb, vk, how), "unpack_var_rt<false> table + gated look-back pass", fills=how == "zeros")
        add(f"tiled-right-vk{vk}-after-larger", Pred("unpack", A_S3_MID, 0, None),
            Call("tiled", U("40-200", 513, 2), vk, "right"), "unpack_var_rt<false> table, no second pass", fills=False)
    # single string, the walk: the short tail and the long one, after long tiles and after BOUNDS
    walk1 = [
        (Call("unpack", U("lt20", 4099, 1), None, None), "walk<true,2> + str1_tail"),
        (Call("unpack", U("20-40", 513, 1), None, None), "walk<true,1> + str1_tail"),
        (Call("unpack", U("20-40", 257, 1), 0, None), "walk<true,1> + str1_tail"),
        (Call("unpack", U("40-200", 4099, 1), 0, None), "walk<true,1> + scan1 + chars"),
        (Call("unpack", Batch("long", 257, 1, "gt255"), None, None), "walk + scan1 + chars"),
    ]
    for b, branch in walk1:
        name = f"walk1-{label(b.batch)}-vk{b.vk}"
        add(f"{name}-after-near-long-tiles", Pred("unpack", U("40-200", b.batch.n + 5, 1), 0, None), b, branch)
        add(f"{name}-after-larger-long-tiles", Pred("unpack", A_S1_MID, 0, None), b, branch, fills=False)
        add(f"{name}-after-near-bounds", Pred("unpack_bounds", near(b.batch), b.vk, None), b, branch, fills=False)
        add(f"{name}-after-larger-bounds", Pred("unpack_bounds", A_S1_LT20, None, None), b, branch, fills=False)
    # several strings, the walk plus scans
    for bb, big in ((U("20-40", 513, 2), A_S3_MID), (U("40-200", 4099, 3), A_S2_MID), (U("20-40", 257, 3), A_S2_2040)):
        b = Call("unpack", bb, 0, None)
        add(f"walkN-{label(bb)}-after-near", Pred("unpack", near(bb), 0, None), b, "walk + scans + chars_multi")
        add(f"walkN-{label(bb)}-after-larger", Pred("unpack", big, 0, None), b, "walk + scans + chars_multi", fills=False)
    bb = U("20-40", 4099, 2)
    add("walkN-default-short-after-larger", Pred("unpack", A_S3_MID, 0, None), Call("unpack", bb, None, None),
        "walk + scans + chars_multi")
    add("walkN-default-short-after-near-bounds", Pred("unpack_bounds", near(bb), None, None),
        Call("unpack", bb, None, None), "walk + scans + chars_multi", fills=False)
    return out


# the server's sequence: unpack(request plan, batch 1), pack(response plan,
# batch 1), unpack(request plan, batch 2) on one scratch sized for the largest
# need of both plans at the largest batch
SERVER = {
    # batch 1, batch 2: records too long for the record tiles' LDS stage even before the envelope, so the
    # unpack walks -- lengths, positions and partials from the scratch's first byte on, where the response
    # pack keeps its own (the record tiles' few words of a shorter-record batch lie behind all that, out
    # of the pack's reach: seen on the GPU)
    "request": (Batch("long", 4099, 2, "gt255"), Batch("long", 513, 2, "gt255")),
    "response": Batch("long", 4099, 1, "gt255"),  # too long for the record tiles: the pack that uses the scratch
    "max_n": 4099,
}
# the STALLED retry: a several-string look-back batch, and what dirtied the scratch before it
STALLED = U("40-200", 16_641, 2)


def all_pairs():
    return pack_pairs() + unpack_pairs()


def batches_of(pair):
    return [x.batch for x in (pair.a, pair.b) if x.batch is not None]
