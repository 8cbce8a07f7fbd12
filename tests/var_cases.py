"""Deterministic string-record batches whose shape, not their bytes, is the
point (pure numpy: used by tests/test_gpu_geometry.py, proven to be what they
say by tests/test_var_cases_cpu.py).

Every generator returns (kinds, cols, offs) as oracle.pack takes them: cols[f]
a numpy column (fixed field) or the uint8 chars (string field), offs[f] the
n + 1 u64 string offsets or None.  "Record bytes" always include the fixed
fields, the 8-byte length words and the envelope prefix (`prefix_len`).
"""
import numpy as np

import oracle

I8, I16, I32, I64, BOOL, STR = oracle.INT8, oracle.INT16, oracle.INT32, oracle.INT64, oracle.BOOL, oracle.STRING

# one, two and three string fields between fixed fields of every width
SCHEMAS = {
    1: [I16, STR],                                  # 10 fixed bytes
    2: [STR, I32, STR],                             # 20
    3: [I8, STR, I64, BOOL, STR, I16, STR],         # 36
}
# 16 int64 fields and 4 strings: with the largest LDS image and chars stage a
# plan can ask for, the record-tile pack's carve passes a workgroup's LDS
WIDE = [I64, STR, I64, I64, I64, I64, STR, I64, I64, I64, I64, STR, I64, I64, I64, I64, STR, I64, I64, I64]

BANDS = [(12, 20), (20, 40), (40, 200)]  # average record bytes [lo, hi) of uniform(band, ...)
TILE = 256                               # records of an aligned tile

# wire capacities of the slack tests as functions of the batch's bytes
CAPS = {
    "exact": lambda t: t,
    "plus1": lambda t: t + 1,
    "x17/16": lambda t: t * 17 // 16,
    "x2": lambda t: 2 * t,
    "x8": lambda t: 8 * t,
    "x64": lambda t: 64 * t,
}
SLACK_SIZES = [1, 255, 256, 257, 511, 512, 513, 4099, 30_001]


def fixed_bytes(kinds, prefix_len=0):
    return prefix_len + sum(8 if k == STR else oracle.KIND_SIZE[k] for k in kinds)


def record_sizes(kinds, offs, n, prefix_len=0):
    sizes = np.full(n, fixed_bytes(kinds, prefix_len), np.uint64)
    for k, o in zip(kinds, offs):
        if k == STR:
            sizes += np.diff(np.asarray(o, np.uint64))
    return sizes


def rec_offsets(kinds, offs, n, prefix_len=0):
    r = np.zeros(n + 1, np.uint64)
    r[1:] = np.cumsum(record_sizes(kinds, offs, n, prefix_len))
    return r


def _batch(kinds, lens, n, rng):
    """Columns of random bytes around the given per-string-field lengths."""
    cols, offs, si = [], [], 0
    for k in kinds:
        if k == STR:
            o = np.zeros(n + 1, np.uint64)
            o[1:] = np.cumsum(lens[si].astype(np.uint64))
            si += 1
            cols.append(rng.integers(0, 256, max(1, int(o[-1])), dtype=np.uint8))
            offs.append(o)
        else:
            dt = np.dtype(oracle.KIND_DTYPE[k])
            c = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
            cols.append((c & 1).astype(np.uint8) if k == BOOL else c)
            offs.append(None)
    return kinds, cols, offs


def uniform(band, n, nstr=1, prefix_len=0, kinds=None):
    """Lengths uniform in [0, maxlen] (empty strings included), maxlen chosen
    so the exact average record lands mid-band; a draw that misses the band
    (tiny n) is drawn again with the next seed."""
    lo, hi = band
    kinds = list(kinds or SCHEMAS[nstr])
    ns = sum(k == STR for k in kinds)
    fixed = fixed_bytes(kinds, prefix_len)
    target = (lo + hi) / 2 if hi <= 40 else 120
    if fixed >= target:
        raise ValueError(f"{fixed} fixed bytes leave no room in band {band}")
    maxlen = int(round(2 * (target - fixed) / ns))
    for seed in range(200):
        rng = np.random.default_rng([lo, n, ns, prefix_len, seed])
        lens = [rng.integers(0, maxlen + 1, n) for _ in range(ns)]
        total = fixed * n + int(sum(l.sum() for l in lens))
        if lo * n <= total < hi * n:
            return _batch(kinds, lens, n, rng)
    raise ValueError(f"no draw of {n} records in band {band}")


# (n, string fields, {(record, string ordinal): length}) of the heavy_tail
# instances: long strings in different fields of different tiles -- at a
# tile's first and last record and inside it -- and one string past 64 KiB
HEAVY = {
    "low": (30_001, 2, {(300, 0): 5_000, (256 * 5 + 255, 1): 9_000, (256 * 9, 0): 3_000, (256 * 40 + 17, 1): 70_001,
                        (256 * 41, 0): 700, (30_000, 1): 4_097}),
    "mid": (4_099, 3, {(300, 0): 5_000, (256 * 5 + 255, 1): 9_000, (256 * 9, 2): 3_000, (256 * 3 + 17, 1): 90_001,
                       (256 * 4, 2): 20_000, (4_098, 0): 4_097}),
}


def heavy_tail(which):
    """Nearly all strings of 0..8 bytes, a handful of long ones: a tile's wire
    span is then many times the batch average's."""
    n, nstr, longs = HEAVY[which]
    kinds = list(SCHEMAS[nstr])
    rng = np.random.default_rng([7, n, nstr])
    lens = [rng.integers(0, 9, n) for _ in range(nstr)]
    for (r, s), ln in longs.items():
        lens[s][r] = ln
    return _batch(kinds, lens, n, rng)


def bursts(n, nstr=2, prefix_len=0):
    """Runs of 256..600 records with every string empty alternate with runs of
    60..300 records near 300 bytes: consecutive tiles switch regimes.  The
    batch starts inside a long-record run."""
    kinds = list(SCHEMAS[nstr])
    rng = np.random.default_rng([11, n, nstr])
    per = (300 - fixed_bytes(kinds, prefix_len)) // nstr
    lens = [np.zeros(n, np.int64) for _ in range(nstr)]
    at, long_run = 0, True
    while at < n:
        run = int(rng.integers(60, 301)) if long_run else int(rng.integers(256, 601))
        end = min(n, at + run)
        if long_run:
            for l in lens:
                l[at:end] = rng.integers(per - 8, per + 9, end - at)
        at, long_run = end, not long_run
    return _batch(kinds, lens, n, rng)


def based(case, bases=(1, 4093, 2**32 + 5)):
    """The same batch with string field s's offsets shifted by bases[s mod
    len]: offsets are absolute, so the chars of that field are addressed from
    a column pointer moved BACK by the base (no allocation grows).  Returns
    (kinds, cols, shifted offs, per-field base or None)."""
    kinds, cols, offs = case
    out, per_field, s = [], [], 0
    for k, o in zip(kinds, offs):
        if k == STR:
            b = int(bases[s % len(bases)])
            s += 1
            out.append(np.asarray(o, np.uint64) + np.uint64(b))
            per_field.append(b)
        else:
            out.append(None)
            per_field.append(None)
    return kinds, cols, out, per_field


def wide(n, maxlen=12):
    """WIDE with short strings (an average record under 240 bytes: the record
    tiles would be chosen)."""
    rng = np.random.default_rng([13, n])
    ns = sum(k == STR for k in WIDE)
    return _batch(list(WIDE), [rng.integers(0, maxlen + 1, n) for _ in range(ns)], n, rng)


def slack_batches():
    """(name, maker) of every batch of the capacity-slack test."""
    out = []
    for b, band in enumerate(BANDS):
        nstr = (1, 2, 3)[b]
        for n in SLACK_SIZES:
            out.append((f"uniform{band[0]}-{band[1]}_n{n}", lambda band=band, n=n, nstr=nstr: uniform(band, n, nstr)))
    for n in SLACK_SIZES:
        out.append((f"bursts_n{n}", lambda n=n: bursts(n)))
    for which in HEAVY:
        out.append((f"heavy_{which}", lambda which=which: heavy_tail(which)))
    return out


def slack_caps(total):
    """(name, wire_cap) of the capacities run for a batch of `total` bytes
    (the largest, 64 times the 3.6 MB batch, is a 230 MB device buffer)."""
    return [(name, f(total)) for name, f in CAPS.items()]
