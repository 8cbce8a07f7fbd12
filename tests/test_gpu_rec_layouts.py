"""Every schema-specialised record kernel (srpc_amd/csrc/rec.hip), both
directions, against the C oracle.

The instances, restated from kRec[] in rec.hip.  All have G = 4 records per
lane group; the unpack tile is 64 * G * K records, and that is the real tile
of every instance:

  # layout                                         instance            G K  unpack tile  pack
  0 all_kinds, no envelope, 17 B                   Lay<0,1,1,1,2,4,8>  4 4  1024         k_pack_rec, default
  1 Number behind the square request, 53 B         Lay<49,4>           4 1   256         k_pack_env, default
  2 Number behind a response, 19 B                 Lay<15,4>           4 2   512         k_pack_rec, rec_kernel=2 only
  3 TwoNumbers behind the add request, 58 B        Lay<50,4,4>         4 1   256         k_pack_env, default
  4 TwoNumbers behind subtract / multiply, 63 B    Lay<55,4,4>         4 1   256         k_pack_rec, rec_kernel=2 only
  5 TwoNumbers behind a response, 27 B             Lay<19,4,4>         4 2   512         k_pack_rec, rec_kernel=2 only

k_pack_env packs whole periods of 16 records, so the pack tile of instances 1
and 3 is 16.  They keep k_pack_env at every rec_kernel other than 0: their
k_pack_rec instantiations, k_pack_rec<Lay<49,4>,4,1> and
k_pack_rec<Lay<50,4,4>,4,1>, are compiled but cannot be reached through the
API, and nothing here tries to.

srpc_gpu_pack / srpc_gpu_unpack give the whole tiles to these kernels and the
rest to a generic tile kernel, with the pointers moved on and a `base` for the
status.  So every case runs at record counts around one specialised tile and
around 16, with rec_kernel 1 (the default choice), 2 (specialised in both
directions) and 0 (generic kernels only).

Expected bytes, statuses and indices come from oracle.pack / oracle.unpack and
from the contract in include/srpc_gpu.h, never from a kernel.  Outputs lie
between sentinel pads (Checked), so each case also shows that nothing was
written in front of an output, behind n * stride of a wire, or behind n (or
n_fit) elements of a column.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, Schema, SRPC_ERR_BOUNDS, SRPC_STATUS_BOUNDS, SRPC_STATUS_PREFIX

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests.test_gpu_geometry import Checked  # noqa: E402
from tests.test_gpu_parity import dev, gpu_pack, gpu_unpack, read_status, status_buf  # noqa: E402

CLEAN = (0, 2**64 - 1)
WAVE, G = 64, 4  # kRecWave and the G of every instance

ALL_KINDS = Schema.of("all_kinds", ("a", "bool"), ("b", "int8"), ("c", "char"), ("d", "int16"), ("e", "int32"),
                      ("f", "int64"))

# kRec[] (srpc_amd/csrc/rec.hip): index, schema, how the envelope is made,
# prefix bytes P, record bytes, rounds K, unpack tile TR = 64 * G * K.
Inst = namedtuple("Inst", "index schema envelope P stride K TR")
INSTANCES = {
    "all_kinds": Inst(0, ALL_KINDS, None, 0, 17, 4, 1024),
    "square_request": Inst(1, srpc_amd.NUMBER, ("request", srpc_amd.SQUARE_METHOD), 49, 53, 1, 256),
    "number_response": Inst(2, srpc_amd.NUMBER, ("response", 0), 15, 19, 2, 512),
    "add_request": Inst(3, srpc_amd.TWO_NUMBERS, ("request", "Calculator_servicer::add"), 50, 58, 1, 256),
    # one instance, two method names of the same length and different bytes
    "subtract_request": Inst(4, srpc_amd.TWO_NUMBERS, ("request", "Calculator_servicer::subtract"), 55, 63, 1, 256),
    "multiply_request": Inst(4, srpc_amd.TWO_NUMBERS, ("request", "Calculator_servicer::multiply"), 55, 63, 1, 256),
    "two_numbers_response": Inst(5, srpc_amd.TWO_NUMBERS, ("response", 0), 19, 27, 2, 512),
}
ENVELOPED = [name for name, i in INSTANCES.items() if i.P]
PACK_TILE = 16  # k_pack_env's period


def test_table_matches_the_plans():
    for name, inst in INSTANCES.items():
        assert inst.TR == WAVE * G * inst.K, name
        p = _packer(name)
        assert p.path == srpc_amd.SRPC_PATH_TILE, name
        assert p.prefix == _prefix(name) and len(p.prefix) == inst.P, name
        assert p.record_bytes == inst.stride, name
    assert _prefix("subtract_request") != _prefix("multiply_request")


def _prefix(name):
    """The envelope's bytes, from the oracle."""
    inst = INSTANCES[name]
    if inst.envelope is None:
        return b""
    kind, arg = inst.envelope
    if kind == "request":
        return oracle.request_prefix(arg, inst.schema.name)
    return oracle.response_prefix(arg, inst.schema.name)


def _packer(name, rec_kernel=None):
    inst = INSTANCES[name]
    if inst.envelope is None:
        p = GpuPacker(inst.schema)
    elif inst.envelope[0] == "request":
        p = GpuPacker.for_request(inst.schema, inst.envelope[1])
    else:
        p = GpuPacker.for_response(inst.schema, inst.envelope[1])
    if rec_kernel is not None:
        p.tune(rec_kernel=rec_kernel)
    return p


def _counts(TR):
    out = []
    for t in (TR, PACK_TILE):
        out += [0, 1, 15, 16, 17, t - 1, t, t + 1, 2 * t - 1, 2 * t + 17, 5 * t + 100]
    return sorted(set(out))


def _cols(kinds, n, rng):
    out = []
    for k in kinds:
        dt = np.dtype(oracle.KIND_DTYPE[k])
        c = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
        if k == oracle.BOOL:
            c = c & 1
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _batch(kinds, prefix, n):
    """(columns, the oracle's wire) of n random records; made once, read-only."""
    rng = np.random.default_rng([n, len(prefix), len(kinds), sum(kinds)])
    cols = _cols(kinds, n, rng)
    want = oracle.pack(list(kinds), cols, n, prefix)
    assert len(want) == n * (len(prefix) + sum(oracle.KIND_SIZE[k] for k in kinds))
    for c in cols:
        c.setflags(write=False)
    return cols, want


def _case(name, n):
    return _batch(tuple(INSTANCES[name].schema.kinds), _prefix(name), n)


def _pack_checked(p, cols, n):
    g = Checked([n * p.record_bytes])
    p.pack([dev(c) for c in cols], n, g.slices[0])
    return g


def _unpack_checked(p, wire, wire_len, n, cols):
    """Unpack `wire_len` bytes of `wire` (all of it on the device) into guarded
    columns.  Returns (Checked, return code, status)."""
    w = np.frombuffer(bytes(wire), np.uint8) if len(wire) else np.zeros(16, np.uint8)
    g = Checked([n * c.dtype.itemsize for c in cols])
    st = status_buf()
    rc = p.unpack(dev(w), wire_len, n, g.slices, st)
    return g, rc, read_status(st)


def _assert_both_directions(p, kinds, prefix, n, what):
    cols, want = _batch(tuple(kinds), prefix, n)
    g = _pack_checked(p, cols, n)
    assert g.head(0, len(want)).tobytes() == want, what
    assert g.pads_clean(), what
    out, rc, st = _unpack_checked(p, want, len(want), n, cols)
    assert rc == 0 and st == CLEAN, what
    for i, c in enumerate(cols):
        assert out.head(i, c.nbytes).tobytes() == c.tobytes(), (what, i)
    assert out.pads_clean(), what


# ---- 1. all six instances, both directions ---------------------------------------------

@pytest.mark.parametrize("rec_kernel", [1, 2, 0])
@pytest.mark.parametrize("name,n", [(name, n) for name, i in INSTANCES.items() for n in _counts(i.TR)])
def test_both_directions_vs_oracle(name, n, rec_kernel):
    """Pack into a guarded wire and unpack the oracle's wire into guarded
    columns.  With rec_kernel=2 instances 2, 4 and 5 pack through k_pack_rec;
    instance 4 unpacks through k_unpack_rec by default."""
    inst = INSTANCES[name]
    p = _packer(name, rec_kernel)
    _assert_both_directions(p, inst.schema.kinds, _prefix(name), n, (name, n, rec_kernel))


# ---- 2. arbitrary prefixes -------------------------------------------------------------

def _raw_prefix(name, how):
    inst = INSTANCES[name]
    rng = np.random.default_rng([inst.index, inst.P])
    if how == "random":
        return rng.integers(0, 256, inst.P, dtype=np.uint8).tobytes()
    if how == "high":  # every byte >= 0x80
        return rng.integers(0x80, 256, inst.P, dtype=np.uint8).tobytes()
    pre = bytearray(_prefix(name))  # the Calculator's, but for its last byte
    pre[-1] ^= 0x01
    return bytes(pre)


LAYOUTS = ["all_kinds", "square_request", "number_response", "add_request", "subtract_request",
           "two_numbers_response"]  # one name per kRec[] entry


@pytest.mark.parametrize("how", ["random", "high", "last_byte"])
@pytest.mark.parametrize("name", [n for n in LAYOUTS if INSTANCES[n].P])
def test_instance_matches_whatever_the_prefix_bytes(name, how):
    """rec_kernel_for matches by prefix length and field sizes alone: a raw
    prefix of an instance's length gets its kernels, which must pack and
    compare the plan's bytes."""
    inst = INSTANCES[name]
    prefix = _raw_prefix(name, how)
    assert len(prefix) == inst.P and prefix != _prefix(name)
    p = GpuPacker(inst.schema, prefix)
    assert p.record_bytes == inst.stride
    p.tune(rec_kernel=2)
    n = 2 * inst.TR + 17
    _assert_both_directions(p, inst.schema.kinds, prefix, n, (name, how))
    # the Calculator's records are not this plan's: every record differs, the first is named
    cols, calc = _case(name, n)
    st = status_buf()
    rc, back = gpu_unpack(p, calc, n, [c.dtype for c in cols], status=st)
    assert rc == 0 and read_status(st) == (SRPC_STATUS_PREFIX, 0), (name, how)
    ost, _, _, _, err = oracle.unpack(inst.schema.kinds, calc, n, prefix)
    assert ost == oracle.ORC_ERR_PREFIX and err == 0
    for c, b in zip(cols, back):
        assert c.tobytes() == b.tobytes(), (name, how)


def _near_misses():
    out = []
    for name in LAYOUTS:
        inst = INSTANCES[name]
        kinds = list(inst.schema.kinds)
        out.append((name, "longer", tuple(kinds), inst.P + 1))
        if inst.P:
            out.append((name, "shorter", tuple(kinds), inst.P - 1))
        for f, k in enumerate(kinds):
            if k == oracle.INT32:
                out.append((name, f"int64_at_{f}", tuple(kinds[:f] + [oracle.INT64] + kinds[f + 1:]), inst.P))
    return out


@pytest.mark.parametrize("name,how,kinds,P", _near_misses(), ids=[f"{m[0]}-{m[1]}" for m in _near_misses()])
def test_near_miss_layouts_take_the_generic_kernels(name, how, kinds, P):
    """One prefix byte more or fewer, or an int64 where the instance has an
    int32: no instance, and the oracle's bytes all the same."""
    inst = INSTANCES[name]
    pre = _prefix(name)
    prefix = (pre + b"\x5a")[:P] if P >= len(pre) else pre[:P]
    assert len(prefix) == P
    p = GpuPacker(Schema("X", tuple((f"f{i}", k) for i, k in enumerate(kinds))), prefix)
    p.tune(rec_kernel=2)
    _assert_both_directions(p, kinds, prefix, inst.TR + 1, (name, how))


# ---- 3. the first bad record ------------------------------------------------------------

def _record(inst, tile, k, lane, r):
    """The record that lane `lane` decodes as record r of its group in round k."""
    return tile * inst.TR + (k * WAVE + lane) * G + r


def _check_bad(name, flips, want_first, tune=None, what=None):
    """Flip the given (record, prefix byte) pairs of the oracle's wire of
    2 * TR + 17 records; the unpack must name `want_first`, as the oracle
    does, and still decode every field."""
    inst = INSTANCES[name]
    n = 2 * inst.TR + 17
    cols, want = _case(name, n)
    wire = bytearray(want)
    for rec, b in flips:
        assert 0 <= rec < n and 0 <= b < inst.P
        wire[rec * inst.stride + b] ^= 1 << ((rec + b) % 8)
    p = _packer(name, 2)
    if tune:
        p.tune(**tune)
    st = status_buf()
    rc, back = gpu_unpack(p, bytes(wire), n, [c.dtype for c in cols], status=st)
    assert rc == 0, what
    assert read_status(st) == (SRPC_STATUS_PREFIX, want_first), what
    ost, _, _, _, err = oracle.unpack(inst.schema.kinds, bytes(wire), n, _prefix(name))
    assert ost == oracle.ORC_ERR_PREFIX and err == want_first, what
    for c, b in zip(cols, back):
        assert c.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("r", range(G))
@pytest.mark.parametrize("lane", [0, 1, 63])
@pytest.mark.parametrize("name,tile,k", [(name, t, k) for name in ENVELOPED for t in (0, 1)
                                         for k in range(INSTANCES[name].K)])
def test_bad_record_index_every_round_lane_and_slot(name, tile, k, lane, r):
    inst = INSTANCES[name]
    rec = _record(inst, tile, k, lane, r)
    assert tile * inst.TR <= rec < (tile + 1) * inst.TR
    _check_bad(name, [(rec, rec % inst.P)], rec)


@pytest.mark.parametrize("name,b", [(name, b) for name in ENVELOPED for b in range(INSTANCES[name].P)])
def test_every_prefix_byte_is_compared(name, b):
    """Byte b of the prefix, flipped in one record of the last round."""
    inst = INSTANCES[name]
    rec = _record(inst, 1, inst.K - 1, 37, 2)
    _check_bad(name, [(rec, b)], rec)


@pytest.mark.parametrize("which", ["round0_beats_lower_lane", "same_lane_both_rounds", "same_group", "second_tile",
                                   "last_round_first"])
@pytest.mark.parametrize("name", ENVELOPED)
def test_several_bad_records_smallest_index_wins(name, which):
    inst = INSTANCES[name]
    K, TR = inst.K, inst.TR
    tail = 2 * TR + 9
    recs = {
        # a later lane's round 0 in front of an earlier lane's last round
        "round0_beats_lower_lane": [_record(inst, 0, K - 1, 5, 1), _record(inst, 0, 0, 60, 3), _record(inst, 1, 0, 0, 0)],
        # one lane finds a bad record in every round, and other lanes later ones
        "same_lane_both_rounds": [_record(inst, 0, k, 17, 3 - k % 4) for k in range(K)] + [_record(inst, 0, K - 1, 18, 0)],
        # two records of one group: the lower bit of the mask
        "same_group": [_record(inst, 0, K - 1, 41, 3), _record(inst, 0, K - 1, 41, 1), _record(inst, 1, 0, 2, 2)],
        "second_tile": [_record(inst, 1, K - 1, 63, 3), _record(inst, 1, K - 1, 9, 2)],
        "last_round_first": [_record(inst, 0, K - 1, 0, 2), _record(inst, 1, 0, 0, 0), _record(inst, 1, K - 1, 1, 1)],
    }[which] + [tail]
    flips = [(rec, (7 * i + rec) % inst.P) for i, rec in enumerate(recs)]
    _check_bad(name, flips, min(recs), what=(name, which, recs))


@pytest.mark.parametrize("tune", [None, {"wave_unpack_bytes": 0}, {"wave_unpack_bytes": 2048}],
                         ids=["plan", "workgroup_tiles", "wave_tiles"])
@pytest.mark.parametrize("name", ENVELOPED)
def test_bad_record_in_the_tail_only(name, tune):
    """The tail goes to a generic kernel behind two specialised tiles.  An
    enveloped plan has workgroup tiles as it stands (wave tiles are the
    default only for records under 16 bytes without an envelope), so the first
    two run k_unpack_tile; wave_unpack_bytes=2048 makes it k_unpack_tile_wave,
    tiles of 16 or 32 records.  Both kernels must add `base`."""
    inst = INSTANCES[name]
    rec = 2 * inst.TR + 3
    _check_bad(name, [(rec, inst.P - 1)], rec, tune=tune)


@pytest.mark.parametrize("rec_kernel", [2, 0])
@pytest.mark.parametrize("name", ENVELOPED)
def test_value_bytes_do_not_count_as_prefix(name, rec_kernel):
    """The first field's bytes differ from anything a comparison loop that runs
    past the prefix could hold them against (zero, the prefix's first, last
    and same-numbered bytes): no flag."""
    inst = INSTANCES[name]
    n = 2 * inst.TR + 17
    pre = _prefix(name)
    cols, _ = _case(name, n)
    first = np.empty((n, 4), np.uint8)
    for j in range(4):
        v = 0xFF ^ pre[-1]  # the complement of a prefix byte
        while v in (0, pre[0], pre[-1], pre[j]):
            v = (v + 0x55) & 0xFF
        first[:, j] = v
    cols = [first.reshape(-1).view(np.int32)] + list(cols[1:])
    want = oracle.pack(inst.schema.kinds, cols, n, pre)
    p = _packer(name, rec_kernel)
    out, rc, st = _unpack_checked(p, want, len(want), n, cols)
    assert rc == 0 and st == CLEAN
    for i, c in enumerate(cols):
        assert out.head(i, c.nbytes).tobytes() == c.tobytes()
    assert out.pads_clean()


# ---- 4. short wires across the seam ------------------------------------------------------

CUTS = {  # wire_len from (n, TR, stride)
    "all_but_a_byte": lambda n, TR, s: n * s - 1,
    "2TR_less_a_byte": lambda n, TR, s: 2 * TR * s - 1,
    "2TR_less_a_record": lambda n, TR, s: (2 * TR - 1) * s,
    "TR_less_a_byte": lambda n, TR, s: TR * s - 1,
    "TR_less_a_record": lambda n, TR, s: (TR - 1) * s,
    "TR+1_less_a_byte": lambda n, TR, s: (TR + 1) * s - 1,
    "TR+1_less_a_record": lambda n, TR, s: TR * s,
    "nothing_fits": lambda n, TR, s: s - 1,
    "zero": lambda n, TR, s: 0,
}


def _assert_cut_columns(g, cols, n_fit, what):
    for i, c in enumerate(cols):
        sz = c.dtype.itemsize
        assert g.head(i, n_fit * sz).tobytes() == c[:n_fit].tobytes(), (what, i)
        assert g.untouched(i, n_fit * sz), (what, i)  # elements >= n_fit
    assert g.pads_clean(), what


@pytest.mark.parametrize("rec_kernel", [2, 0])
@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("name", list(INSTANCES))
def test_short_wire(name, cut, rec_kernel):
    """wire_len short of n records: n_fit / TR tiles go to the specialised
    kernel and the rest of the n_fit to a generic one.  The whole wire is on
    the device, so a record decoded from behind wire_len shows in the column."""
    inst = INSTANCES[name]
    n = 2 * inst.TR + 17
    cols, want = _case(name, n)
    wire_len = CUTS[cut](n, inst.TR, inst.stride)
    n_fit = wire_len // inst.stride
    assert 0 <= wire_len < len(want) and n_fit < n
    p = _packer(name, rec_kernel)
    g, rc, st = _unpack_checked(p, want, wire_len, n, cols)
    assert rc == SRPC_ERR_BOUNDS
    assert st == (SRPC_STATUS_BOUNDS, n_fit)
    _assert_cut_columns(g, cols, n_fit, (name, cut, rec_kernel))
    ost, _, _, _, err = oracle.unpack(inst.schema.kinds, want[:wire_len], n, _prefix(name))
    assert ost == oracle.ORC_ERR_BOUNDS and err == n_fit


def _front_and_fit(inst, where):
    """(n_fit, the bad record in front of it) for the combined cases."""
    TR, K = inst.TR, inst.K
    return {
        "front_in_last_round_of_tile_1": (2 * TR + 5, _record(inst, 1, K - 1, 63, 1)),
        "front_in_the_tail": (2 * TR + 5, 2 * TR + 2),
        "fit_is_one_tile": (TR, _record(inst, 0, K - 1, 30, 3)),
        "front_is_the_last_that_fits": (TR + 1, TR),
        "nothing_in_front": (2 * TR + 5, None),
    }[where]


@pytest.mark.parametrize("rec_kernel", [2, 0])
@pytest.mark.parametrize("where", ["front_in_last_round_of_tile_1", "front_in_the_tail", "fit_is_one_tile",
                                   "front_is_the_last_that_fits", "nothing_in_front"])
@pytest.mark.parametrize("name", ENVELOPED)
def test_short_wire_with_bad_prefixes(name, where, rec_kernel):
    """A cut and flipped prefixes, one in front of n_fit and two behind it:
    in the record that the cut divides (its flipped byte lies behind
    wire_len) and three records on.  Records behind n_fit are not decoded and
    must not be reported."""
    inst = INSTANCES[name]
    n = 2 * inst.TR + 17
    cols, want = _case(name, n)
    n_fit, front = _front_and_fit(inst, where)
    wire_len = n_fit * inst.stride + inst.P - 1  # all of record n_fit's prefix but its last byte
    wire = bytearray(want)
    wire[n_fit * inst.stride + inst.P - 1] ^= 0x80
    wire[(n_fit + 3) * inst.stride + 2] ^= 0x04
    if front is not None:
        assert front < n_fit
        wire[front * inst.stride + front % inst.P] ^= 0x20
    p = _packer(name, rec_kernel)
    g, rc, st = _unpack_checked(p, wire, wire_len, n, cols)
    assert rc == SRPC_ERR_BOUNDS
    ost, _, _, _, err = oracle.unpack(inst.schema.kinds, bytes(wire[:wire_len]), n, _prefix(name))
    if front is None:
        assert st == (SRPC_STATUS_BOUNDS, n_fit)
        assert ost == oracle.ORC_ERR_BOUNDS and err == n_fit
    else:
        assert st == (SRPC_STATUS_BOUNDS | SRPC_STATUS_PREFIX, min(n_fit, front))
        assert ost == oracle.ORC_ERR_PREFIX and err == front  # the oracle stops at its first error
    _assert_cut_columns(g, cols, n_fit, (name, where, rec_kernel))
