"""Inputs that choose a kernel or its LDS carve, varied apart from the data.

srpc_gpu_pack_var picks its kernel (record tiles against the scan + chunk
walk, one or two records per lane, per-tile or looping workgroups) and the
size of its LDS image from wire_cap / n -- the caller's capacity -- and the
four geometry knobs (SRPC_TUNE_TILE_BYTES, _PACK_TILE_BYTES, _VAR_IMAGE_BYTES,
_VAR_CHARS_BYTES) move tile edges.  Here: capacities with slack and short of
the batch, every knob at its edges, string lengths that are heavy-tailed or
come in bursts (tests/var_cases.py) so that single tiles overflow the image
and take the in-kernel walk, and string offsets that do not start at 0.

Expected bytes always come from oracle.pack / oracle.unpack.  Every output is
a slice between sentinel pads (Guarded), so each case also asserts that
nothing outside the output was written.
"""
import functools

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, Schema, SrpcError, SRPC_PATH_TILE, SRPC_STATUS_BOUNDS, _lib
from tests import var_cases as vc
from tests.test_gpu_parity import DEV, dev, empty, gpu_pack_var, host, read_status, status_buf, torch
from tests.test_gpu_sweep import PAD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

CLEAN = (0, 2**64 - 1)
KNOB_TILE, KNOB_PACK_TILE, KNOB_VAR_IMAGE, KNOB_VAR_CHARS = 4, 9, 8, 10


class Checked(Guarded):
    """Guarded whose checks run on the device (the capacity tests' buffers
    are tens of MiB): pads, untouched ranges and expected bytes."""

    def pads_clean(self):
        at = 0
        for a, s in self.spans:
            if not bool((self.t[at:a] == SENTINEL).all()):
                return False
            at = a + s
        return bool((self.t[at:] == SENTINEL).all())

    def untouched(self, i, lo):
        """Bytes [lo, size) of slice i still hold the sentinel."""
        a, s = self.spans[i]
        return lo >= s or bool((self.t[a + lo:a + s] == SENTINEL).all())

    def head(self, i, nbytes):
        a, _ = self.spans[i]
        return self.t[a:a + nbytes].cpu().numpy()


def _n_of(cols, offs):
    for c, o in zip(cols, offs):
        return (len(o) - 1) if o is not None else len(c)


@functools.lru_cache(maxsize=None)
def _case(name, prefix=b""):
    """(kinds, cols, offs, n, want wire, want rec_offs): generated and packed
    by the oracle once.  The generators' averages are those of the plain
    batch; an envelope adds its bytes to every record."""
    kind, _, arg = name.partition(":")
    if kind == "slack":
        kinds, cols, offs = dict(vc.slack_batches())[arg]()
    elif kind == "uniform":  # uniform:<band>:<n>:<nstr>
        b, n, nstr = (int(x) for x in arg.split(":"))
        kinds, cols, offs = vc.uniform(vc.BANDS[b], n, nstr)
    elif kind == "heavy":
        kinds, cols, offs = vc.heavy_tail(arg)
    elif kind == "bursts":  # bursts:<n>:<nstr>
        n, nstr = (int(x) for x in arg.split(":"))
        kinds, cols, offs = vc.bursts(n, nstr)
    elif kind == "wide":
        kinds, cols, offs = vc.wide(int(arg))
    else:
        raise KeyError(name)
    n = _n_of(cols, offs)
    want = oracle.pack(kinds, cols, n, prefix, list(offs))
    rec = vc.rec_offsets(kinds, offs, n, len(prefix))
    assert int(rec[n]) == len(want)
    for a in list(cols) + [o for o in offs if o is not None] + [rec]:
        a.setflags(write=False)
    return kinds, cols, offs, n, want, rec


@functools.lru_cache(maxsize=None)
def _unpacked(name, prefix=b""):
    kinds, _, _, n, want, _ = _case(name, prefix)
    rc, ocols, ooffs, consumed, _ = oracle.unpack(kinds, want, n, prefix)
    assert rc == oracle.ORC_OK and consumed == len(want)
    return ocols, ooffs


def _packer(kinds, envelope=None):
    sch = Schema("S", tuple((f"f{i}", k) for i, k in enumerate(kinds)))
    return GpuPacker.for_request(sch, "Svc_servicer::m") if envelope else GpuPacker(sch)


ENVELOPE = oracle.request_prefix("Svc_servicer::m", "S")


def _upload(cols, offs):
    return [dev(c) for c in cols], [dev(np.ascontiguousarray(o, np.uint64)) if o is not None else None for o in offs]


def _pack_guarded(p, dcols, doffs, n, wire_bytes, wire_cap, scratch=None):
    """pack_var into guarded wire / rec_offs slices (scratch: the caller's own,
    at least var_scratch_bytes long, instead of a fresh one).  Returns
    (Checked, status)."""
    g = Checked([wire_bytes, 8 * (n + 1)])
    sb = p.var_scratch_bytes(n, wire_cap)
    if scratch is None:
        scratch = empty(sb + 16)
    assert scratch.numel() >= sb
    st = status_buf()
    p.pack_var(dcols, doffs, n, g.slices[0], wire_cap, g.slices[1], scratch, sb, st)
    return g, read_status(st)


def _assert_packed(g, st, want, rec, n, wire_bytes, what):
    """The wire is the oracle's, the index exact, the status clean, nothing else written."""
    assert st == CLEAN, what
    assert g.head(0, len(want)).tobytes() == want, what
    assert g.untouched(0, len(want)), what  # [total, wire_cap)
    assert g.pads_clean(), what
    assert g.head(1, 8 * (n + 1)).view(np.uint64).tobytes() == rec.tobytes(), what


# ---- a. capacity slack ------------------------------------------------------------

@pytest.mark.parametrize("name", [name for name, _ in vc.slack_batches()])
def test_pack_var_capacity_slack(name):
    """wire_cap from the batch's bytes exactly to 64 times them: the quotient
    wire_cap / n, not the data, picks the kernel and sizes its image."""
    kinds, cols, offs, n, want, rec = _case("slack:" + name)
    dcols, doffs = _upload(cols, offs)
    for vk in (None, 0):
        p = _packer(kinds)
        if vk is not None:
            p.tune(var_kernel=vk)
        for cname, cap in vc.slack_caps(len(want)):
            g, st = _pack_guarded(p, dcols, doffs, n, cap, cap)
            _assert_packed(g, st, want, rec, n, cap, (name, vk, cname, cap // n))


# ---- b. capacity short of the batch, record tiles ------------------------------------

def _cuts(kinds, offs, rec, n):
    """Capacities strictly inside a record past the batch's middle: in a fixed
    field, in a length word, in chars."""
    f_fixed = next(f for f, k in enumerate(kinds) if k != oracle.STRING and oracle.KIND_SIZE[k] >= 2)
    s_last = max(f for f, k in enumerate(kinds) if k == oracle.STRING)
    lens = {f: np.diff(offs[f].astype(np.int64)) for f, k in enumerate(kinds) if k == oracle.STRING}
    r = next(r for r in range(n * 2 // 3, n) if all(l[r] >= 2 for l in lens.values()))

    def field_at(f):  # wire offset of field f inside record r
        at = 0
        for g in range(f):
            at += 8 + int(lens[g][r]) if g in lens else oracle.KIND_SIZE[kinds[g]]
        return int(rec[r]) + at
    return r, {"fixed": field_at(f_fixed) + 1, "length": field_at(s_last) + 3, "chars": field_at(s_last) + 8 + 1}


@pytest.mark.parametrize("vk", [None, 0], ids=["tiles", "walk"])
@pytest.mark.parametrize("name", ["uniform:1:4099:2", "heavy:low", "heavy:mid"])
def test_pack_var_capacity_inside_batch(name, vk):
    """A capacity inside the batch: exactly want[:cap] is written and nothing
    after it, BOUNDS names the first record that does not fit, rec_offs[n] is
    the size needed.  (The short capacity makes wire_cap / n small: record
    tiles, with tiles that straddle and lie past the capacity.)"""
    kinds, cols, offs, n, want, rec = _case(name)
    dcols, doffs = _upload(cols, offs)
    p = _packer(kinds)
    if vk is not None:
        p.tune(var_kernel=vk)
    r, cuts = _cuts(kinds, offs, rec, n)
    for where, cap in cuts.items():
        assert int(rec[r]) < cap < int(rec[r + 1])
        g, st = _pack_guarded(p, dcols, doffs, n, len(want) + 64, cap)
        what = (name, where, cap)
        assert g.head(0, cap).tobytes() == want[:cap], what
        assert g.untouched(0, cap) and g.pads_clean(), what
        assert st == (SRPC_STATUS_BOUNDS, r), what
        got_rec = g.head(1, 8 * (n + 1)).view(np.uint64)
        assert int(got_rec[n]) == len(want) and got_rec.tobytes() == rec.tobytes(), what


# ---- c. VAR_IMAGE_BYTES x VAR_CHARS_BYTES ----------------------------------------------

IMAGE_BYTES = [8192, 8208, 32768, 65536]
CHARS_BYTES = [0, 16, 4096, 65536]


def _unpack_guarded(p, kinds, dwire, wire_len, n, drec, table=None, scratch=None):
    """unpack_var (or _tiled) into guarded columns and offsets (scratch: the
    caller's own instead of a fresh one).  Returns (cols, offs, status) as host
    arrays, string chars cut to their length."""
    sizes = []
    for k in kinds:
        sizes.append(wire_len if k == oracle.STRING else n * oracle.KIND_SIZE[k])
    sidx = [f for f, k in enumerate(kinds) if k == oracle.STRING]
    g = Guarded(sizes + [8 * (n + 1)] * len(sidx))
    outs = g.slices[:len(kinds)]
    so = [None] * len(kinds)
    for j, f in enumerate(sidx):
        so[f] = g.slices[len(kinds) + j]
    sb = p.var_scratch_bytes(n, wire_len)
    if scratch is None:
        scratch = empty(sb + 16)
    assert scratch.numel() >= sb
    st = status_buf()
    if table is None:
        p.unpack_var(dwire, wire_len, n, drec, outs, so, scratch, sb, st)
    else:
        p.unpack_var_tiled(dwire, wire_len, n, drec, table, outs, so, scratch, sb, st)
    status = read_status(st)
    back = g.read()  # asserts the pads
    cols, offs = [], [None] * len(kinds)
    for j, f in enumerate(sidx):
        offs[f] = back[len(kinds) + j].view(np.uint64).copy()
    for f, k in enumerate(kinds):
        cols.append(back[f][:int(offs[f][n])] if k == oracle.STRING else back[f])
    return cols, offs, status


def _assert_unpacked(kinds, got, want, what):
    cols, offs, st = got
    ocols, ooffs = want
    assert st == CLEAN, what
    for f, k in enumerate(kinds):
        if k == oracle.STRING:
            assert np.array_equal(offs[f], ooffs[f]), (what, f)
        assert cols[f].tobytes() == ocols[f].tobytes(), (what, f)


@pytest.mark.parametrize("envelope", [False, True], ids=["plain", "request"])
@pytest.mark.parametrize("name", ["uniform:0:4099:1", "uniform:1:4099:1", "uniform:2:4099:3", "heavy:low", "heavy:mid",
                                  "bursts:4099:1", "bursts:4099:3", "wide:4099"])
def test_var_image_and_chars_knobs(name, envelope):
    """Every image size against every chars stage, 0 bytes included: records
    straddling an image end, tiles whose chars do not fit the stage, and -- for
    the wide schema at the largest sizes -- a carve past a workgroup's LDS,
    which must take the walk.  Pack, then unpack (default and record tiles)."""
    prefix = ENVELOPE if envelope else b""
    kinds, cols, offs, n, want, rec = _case(name, prefix)
    want_back = _unpacked(name, prefix)
    dcols, doffs = _upload(cols, offs)
    dwire, drec = dev(np.frombuffer(want, np.uint8)), dev(rec)
    p = _packer(kinds, envelope)
    assert p.prefix == prefix
    for img in IMAGE_BYTES:
        for ch in CHARS_BYTES:
            p.tune(var_kernel=1, var_image_bytes=img, var_chars_bytes=ch)
            g, st = _pack_guarded(p, dcols, doffs, n, len(want), len(want))
            _assert_packed(g, st, want, rec, n, len(want), (name, img, ch))
            for vk in (1, 2):
                p.tune(var_kernel=vk)
                got = _unpack_guarded(p, kinds, dwire, len(want), n, drec)
                _assert_unpacked(kinds, got, want_back, (name, img, ch, vk))


def test_wide_schema_two_per_lane_carve():
    """The wide schema under a capacity that makes wire_cap / n < 20 (512
    records per tile: twice the column slices) with the largest image."""
    kinds, cols, offs, n, want, rec = _case("wide:4099")
    dcols, doffs = _upload(cols, offs)
    p = _packer(kinds)
    p.tune(var_image_bytes=65536)
    cap = 19 * n + 7
    g, st = _pack_guarded(p, dcols, doffs, n, len(want) + 64, cap)
    assert g.head(0, cap).tobytes() == want[:cap]
    assert g.untouched(0, cap) and g.pads_clean()
    assert st == (SRPC_STATUS_BOUNDS, int(np.searchsorted(rec, cap, side="right")) - 1)
    assert g.head(1, 8 * (n + 1)).tobytes() == rec.tobytes()


# ---- d. unpack of skewed batches ------------------------------------------------------

def _table(p, doffs, n):
    t = empty(8 * p.var_tile_table_words(n) + 16)
    p.var_tile_table(doffs, n, t)
    return t


@pytest.mark.parametrize("name", ["heavy:low", "heavy:mid", "bursts:4099:2", "bursts:30001:3"])
def test_unpack_var_skewed(name):
    kinds, cols, offs, n, want, rec = _case(name)
    want_back = _unpacked(name)
    _, doffs = _upload(cols, offs)
    dwire, drec = dev(np.frombuffer(want, np.uint8)), dev(rec)
    p = _packer(kinds)
    for vk in (None, 0, 2):
        if vk is not None:
            p.tune(var_kernel=vk)
        got = _unpack_guarded(p, kinds, dwire, len(want), n, drec)
        _assert_unpacked(kinds, got, want_back, (name, vk))
    for vk in (1, 2):
        p.tune(var_kernel=vk)
        got = _unpack_guarded(p, kinds, dwire, len(want), n, drec, _table(p, doffs, n))
        _assert_unpacked(kinds, got, want_back, (name, "tiled", vk))


@pytest.mark.parametrize("vk", [None, 0, 2], ids=["default", "walk", "tiles"])
@pytest.mark.parametrize("junk", [1, 4097, 300_000])
def test_unpack_var_trailing_junk(junk, vk):
    """wire_len past rec_offs[n]: bytes after the last record belong to no
    record, and a legal index decodes as with the exact length."""
    name = "heavy:mid"
    kinds, _, _, n, want, rec = _case(name)
    rng = np.random.default_rng(junk)
    longer = np.concatenate([np.frombuffer(want, np.uint8), rng.integers(0, 256, junk, dtype=np.uint8)])
    p = _packer(kinds)
    if vk is not None:
        p.tune(var_kernel=vk)
    got = _unpack_guarded(p, kinds, dev(longer), longer.size, n, dev(rec))
    _assert_unpacked(kinds, got, _unpacked(name), (junk, vk))


# ---- e. string offsets that do not start at 0 -------------------------------------------

def _upload_based(cols, boffs, bases, shift=3):
    """Chars columns `shift` bytes into their allocation, given as a pointer
    moved back by the field's base; offsets absolute."""
    keep, ptrs, doffs = [], [], []
    for c, o, b in zip(cols, boffs, bases):
        if b is None:
            t = dev(c)
            ptrs.append(t)
            doffs.append(None)
        else:
            t = torch.zeros(c.size + 2 * PAD, dtype=torch.uint8, device=DEV)
            t[PAD + shift:PAD + shift + c.size].copy_(torch.from_numpy(np.array(c)))
            ptrs.append(int(t.data_ptr()) + PAD + shift - b)
            doffs.append(dev(o))
        keep.append(t)
    return keep, ptrs, doffs


@pytest.mark.parametrize("name,vk,route", [
    ("uniform:1:4099:2", None, "tiles"),      # under 40 bytes: a workgroup per tile
    ("uniform:0:4099:1", None, "tiles x2"),   # under 20: two records per lane
    ("uniform:2:4099:3", None, "loop"),       # 40 and more: resident workgroups loop over tiles
    ("heavy:mid", None, "loop + in-kernel walk"),
    ("uniform:1:4099:2", 0, "scan + walk"),
    ("uniform:0:4099:1", 0, "short records + walk"),
    ("heavy:mid", 0, "scan + walk, long"),
])
def test_pack_var_nonzero_first_offsets(name, vk, route):
    """offs[0] != 0 (a chunk of a larger batch, as the batched client passes
    it): the wire is the oracle's pack of the zero-based batch."""
    kinds, cols, offs, n, want, rec = _case(name)
    _, _, boffs, bases = vc.based((kinds, cols, offs))
    keep, ptrs, doffs = _upload_based(cols, boffs, bases)
    p = _packer(kinds)
    if vk is not None:
        p.tune(var_kernel=vk)
    g, st = _pack_guarded(p, ptrs, doffs, n, len(want), len(want))
    _assert_packed(g, st, want, rec, n, len(want), (name, route))
    # the tile table of the shifted offsets: chars before each tile, not offsets
    sidx = [f for f, k in enumerate(kinds) if k == oracle.STRING]
    words = p.var_tile_table_words(n)
    assert words == (-(-n // 256) + 1) * len(sidx)
    t = Guarded([8 * words])
    p.var_tile_table(doffs, n, t.slices[0])
    table = t.read()[0].view(np.uint64).reshape(-1, len(sidx))
    for j, f in enumerate(sidx):
        at = np.minimum(np.arange(table.shape[0]) * 256, n)
        assert np.array_equal(table[:, j], offs[f][at] - offs[f][0]), (name, f)
    del keep


# ---- f. TILE_BYTES / PACK_TILE_BYTES on fixed schemas ---------------------------------------

TILE_VALUES = [1024, 1025, 4096, 12_345, 49_151, 49_152]
_ALL6 = [oracle.BOOL, oracle.INT8, oracle.CHAR, oracle.INT16, oracle.INT32, oracle.INT64]
# The widest fixed record a plan accepts is SRPC_MAX_PREFIX + 8 * SRPC_MAX_FIELDS
# = 1280 bytes (tests/cpp/schema_limits_test.cpp), under kMaxTileStride = 2048:
# that stride and one a field narrower stand for "at the limit".
FIXED_SCHEMAS = {
    "3B": ([oracle.INT8, oracle.INT16], b""),
    "17B_all_kinds": (_ALL6, b""),
    "53B_request": ([oracle.INT32], oracle.request_prefix(srpc_amd.SQUARE_METHOD, "Number")),
    "1280B_limit": ([oracle.INT64] * _lib.SRPC_MAX_FIELDS, bytes(range(256)) * 4),
    "1273B_below": ([oracle.INT64] * (_lib.SRPC_MAX_FIELDS - 1) + [oracle.INT8], bytes(range(256)) * 4),
}


@functools.lru_cache(maxsize=None)
def _fixed_case(schema, n):
    kinds, prefix = FIXED_SCHEMAS[schema]
    rng = np.random.default_rng([n, len(kinds)])
    cols = []
    for k in kinds:
        c = rng.integers(0, 256, n * oracle.KIND_SIZE[k], dtype=np.uint8).view(oracle.KIND_DTYPE[k])
        cols.append((c & 1).astype(np.uint8) if k == oracle.BOOL else c)
    return kinds, prefix, cols, oracle.pack(kinds, cols, n, prefix)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 65_537])
@pytest.mark.parametrize("schema", sorted(FIXED_SCHEMAS))
def test_tile_bytes_knobs(schema, n):
    """Tile sizes that no stride divides, at both ends of the knobs' range,
    set together and one at a time, generic and schema-specialised kernels:
    partial last tiles and ragged wire tails.  Compared on the device (the
    widest case is an 84 MB wire)."""
    kinds, prefix, cols, want = _fixed_case(schema, n)
    assert len(want) == n * (len(prefix) + sum(oracle.KIND_SIZE[k] for k in kinds))
    assert len(want) // n == int(schema.split("B")[0])
    dcols = [dev(c) for c in cols]
    dwant = dev(np.frombuffer(want, np.uint8))[:len(want)]
    col_bytes = [c.nbytes for c in cols]
    p = GpuPacker(Schema("X", tuple((f"f{i}", k) for i, k in enumerate(kinds))), prefix)
    p.force_path(SRPC_PATH_TILE)
    p.tune(wave_pack_bytes=0, wave_unpack_bytes=0)  # workgroup tiles: the kernels these knobs size
    for rec_kernel in (0, 2):
        for v in TILE_VALUES:
            for which in ("both", "unpack only", "pack only"):
                if which == "both":
                    p.tune(tile_bytes=v)  # sets the pack tile too
                elif which == "unpack only":
                    p.tune(tile_bytes=v, pack_tile_bytes=24576 if prefix else 16384)
                else:
                    p.tune(tile_bytes=32768, pack_tile_bytes=v)
                p.tune(rec_kernel=rec_kernel)
                what = (schema, n, rec_kernel, v, which)
                w = Checked([len(want)])
                p.pack(dcols, n, w.slices[0])
                assert torch.equal(w.slices[0][:len(want)], dwant), what
                assert w.pads_clean(), what
                out = Checked(col_bytes)
                assert p.unpack(dwant, len(want), n, out.slices) == 0, what
                for c, d, s in zip(dcols, out.slices, col_bytes):
                    assert torch.equal(d[:s], c[:s]), what
                assert out.pads_clean(), what
    # ... and once through the host, so the device-side comparison itself is checked
    assert host(dwant, min(len(want), 4096)).tobytes() == want[:4096]


# ---- g. knob validation ---------------------------------------------------------------------

def test_geometry_knob_validation():
    """Values just outside each knob's documented range, a non-multiple of 16
    for the two string knobs, and the wrong kind of schema: SRPC_E_INVALID,
    the plan unchanged -- a pack afterwards still matches the oracle."""
    L = _lib.lib()

    def tune(p, knob, v):
        return L.srpc_plan_tune(p._h, knob, v)

    # a string plan
    kinds, cols, offs, n, want, rec = _case("uniform:2:4099:3")
    ps = _packer(kinds)
    for knob, bad, good in ((KNOB_VAR_IMAGE, (8191, 8176, 65537, 65552, 8200, 32769, -16, 0), (8192, 65536, 8208)),
                            (KNOB_VAR_CHARS, (-1, -16, 65537, 65552, 8, 4097), (0, 16, 65536))):
        for v in good:
            assert tune(ps, knob, v) == _lib.SRPC_OK, (knob, v)
        for v in bad:
            assert tune(ps, knob, v) == _lib.SRPC_E_INVALID, (knob, v)
    with pytest.raises(SrpcError) as e:
        ps.tune(var_image_bytes=8200)
    assert e.value.code == _lib.SRPC_E_INVALID
    for knob in (KNOB_TILE, KNOB_PACK_TILE):  # tile knobs on a string plan
        for v in (1024, 8192, 49152):
            assert tune(ps, knob, v) == _lib.SRPC_E_INVALID, (knob, v)
    # the rejected calls left the last accepted values (image 8208, stage 65536) in place
    wire, got_rec, st = gpu_pack_var(ps, kinds, cols, offs, n)
    assert st == CLEAN and wire == want and np.array_equal(got_rec, rec)
    wire, got_rec, st = gpu_pack_var(ps, kinds, cols, offs, n, wire_cap=2 * len(want) + 5)
    assert st == CLEAN and wire == want and np.array_equal(got_rec, rec)

    # fixed plans: a small record and the widest one
    for schema in ("17B_all_kinds", "1280B_limit"):
        fk, prefix, fcols, fwant = _fixed_case(schema, 4099)
        pf = GpuPacker(Schema("X", tuple((f"f{i}", k) for i, k in enumerate(fk))), prefix)
        pf.tune(tile_bytes=4096)
        for knob in (KNOB_TILE, KNOB_PACK_TILE):
            for v in (1024, 49152):
                assert tune(pf, knob, v) == _lib.SRPC_OK, (knob, v)
            for v in (1023, 0, -1, 49153, 65536, 2**31 - 1, -2**31):
                assert tune(pf, knob, v) == _lib.SRPC_E_INVALID, (knob, v)
        for knob in (KNOB_VAR_IMAGE, KNOB_VAR_CHARS):  # string knobs on a fixed plan
            for v in (8192, 65536, 16):
                assert tune(pf, knob, v) == _lib.SRPC_E_INVALID, (knob, v)
        g = Checked([len(fwant)])
        pf.pack([dev(c) for c in fcols], 4099, g.slices[0])
        assert g.head(0, len(fwant)).tobytes() == fwant and g.pads_clean()
    # (A fixed record wider than kMaxTileStride cannot be built: plan creation
    # refuses more than SRPC_MAX_FIELDS fields or SRPC_MAX_PREFIX prefix bytes,
    # 1280 bytes in all, so the knobs' own stride check is not reachable.)
    k33 = [oracle.INT64] * (_lib.SRPC_MAX_FIELDS + 1)
    with pytest.raises(SrpcError) as e:
        GpuPacker(Schema("X", tuple((f"f{i}", k) for i, k in enumerate(k33))))
    assert e.value.code == _lib.SRPC_E_UNSUPPORTED
