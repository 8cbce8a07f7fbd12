"""The AoS kernels (srpc_amd/csrc/aos.hip) under the struct layouts of
tests/aos_layouts.py: nested messages with a vtable slot between the fields,
runs at other places than offset 8, layouts one step away from a run or from a
compile-time layout, strides off the 8- and 4-byte grid, arrays at every shift
their fields allow, and structs too wide for a staged tile of 16 in LDS.

Everything is byte-exact.  The wire reference is oracle.pack of the columns
read out of the struct array with numpy; the struct reference is a numpy
image of the WHOLE array (aos_layouts.expect_in_place / expect_fresh), so a
kernel that touches a vtable slot, padding or an unnamed member is seen.  The
struct array and the wire both lie between 64-byte 0xA5 pads."""
import ctypes
import zlib

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import GpuPacker, Schema, _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

from tests import aos_layouts as al  # noqa: E402
from tests.test_gpu_parity import dev, empty, host, read_status, status_buf  # noqa: E402

PAD = 64
OK_STATUS = (0, 2**64 - 1)


class Padded:
    """`nbytes` of device memory at `shift` bytes past a 16-byte boundary,
    between PAD-byte 0xA5 pads."""

    def __init__(self, data=None, nbytes=None, shift=0):
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()
        self.n = data.size if data is not None else nbytes
        self.at = PAD + shift
        self.t = empty(self.at + self.n + PAD + 16)
        assert self.t.data_ptr() % 16 == 0
        if data is not None and self.n:
            self.t[self.at:self.at + self.n].copy_(torch.from_numpy(data))
        self.ptr = self.t[self.at:]

    def read(self):
        """The payload, after checking both pads."""
        b = host(self.t, self.t.numel())
        assert (b[:self.at] == 0xA5).all(), "bytes before the buffer were written"
        assert (b[self.at + self.n:] == 0xA5).all(), "bytes after the buffer were written"
        return b[self.at:self.at + self.n].copy()


def packer(lay):
    sch = Schema(al.SCHEMA_NAME, tuple((f"f{i}", k) for i, k in enumerate(lay.kinds)))
    if lay.envelope == "request":
        return GpuPacker.for_request(sch, al.METHOD)
    if lay.envelope == "response":
        return GpuPacker.for_response(sch, 0)
    return GpuPacker(sch)


def image(buf, lay, n):
    return buf.read().reshape(n, lay.stride)


def same(got, want):
    """Whole-array equality, naming the first wrong byte."""
    if not np.array_equal(got, want):
        r, b = np.argwhere(got != want)[0]
        pytest.fail(f"record {r} byte {b}: got {got[r, b]:#04x}, want {want[r, b]:#04x} "
                    f"({int((got != want).sum())} bytes differ in {int((got != want).any(axis=1).sum())} records)")


def check_layout(name, n, shift=0):
    lay = al.LAYOUTS[name]
    stride, offs = lay.stride, list(lay.offsets)
    p = packer(lay)
    assert p.prefix == al.prefix(lay) and p.record_bytes == len(p.prefix) + al.wire_stride(lay)
    W = p.record_bytes
    rng = np.random.default_rng(zlib.crc32(f"{name}/{n}/{shift}".encode()))
    src, old = al.records(lay, n, rng), al.records(lay, n, rng)
    want = np.frombuffer(oracle.pack(list(lay.kinds), al.columns(lay, src), n, p.prefix), np.uint8)
    assert want.size == n * W

    # pack: the oracle's wire, nothing outside it, the structs read only
    arr, wire = Padded(src, shift=shift), Padded(nbytes=n * W)
    p.pack_aos(arr.ptr, stride, offs, n, wire.ptr)
    assert wire.read().tobytes() == want.tobytes()
    same(image(arr, lay, n), src)

    # unpack in place into different structs: only the leaf bytes change
    arr, wire, st = Padded(old, shift=shift), Padded(want), status_buf()
    assert p.unpack_aos(wire.ptr, n * W, n, arr.ptr, stride, offs, st) == 0
    assert read_status(st) == OK_STATUS
    same(image(arr, lay, n), al.expect_in_place(lay, old, src))
    assert wire.read().tobytes() == want.tobytes()

    # unpack into fresh objects
    fill = rng.integers(0, 256, stride, dtype=np.uint8).tobytes()
    fresh_ok = stride <= al.FILL_MAX or al.covered(lay)
    arr, st = Padded(old, shift=shift), status_buf()
    if fresh_ok:
        assert p.unpack_aos_fill(wire.ptr, n * W, n, arr.ptr, stride, offs, fill, st) == 0
        assert read_status(st) == OK_STATUS
        got = image(arr, lay, n)
        same(got, al.expect_fresh(lay, fill, src, n, old))
        if al.covered(lay):
            same(got, src)
    else:  # a struct wider than the fill record
        with pytest.raises(srpc_amd.SrpcError) as e:
            p.unpack_aos_fill(wire.ptr, n * W, n, arr.ptr, stride, offs, fill, st)
        assert e.value.code == _lib.SRPC_E_UNSUPPORTED
        same(image(arr, lay, n), old)

    # a wire that ends one byte short of record k: records < k decoded, the rest as they were
    if n >= 17:
        k = n // 2
        short = k * W + W - 1
        cut = Padded(want[:short])
        arr, st = Padded(old, shift=shift), status_buf()
        assert p.unpack_aos(cut.ptr, short, n, arr.ptr, stride, offs, st) == srpc_amd.SRPC_ERR_BOUNDS
        assert read_status(st) == (srpc_amd.SRPC_STATUS_BOUNDS, k)
        exp = old.copy()
        exp[:k] = al.expect_in_place(lay, old, src)[:k]
        same(image(arr, lay, n), exp)
        if fresh_ok:
            arr, st = Padded(old, shift=shift), status_buf()
            assert p.unpack_aos_fill(cut.ptr, short, n, arr.ptr, stride, offs, fill, st) == srpc_amd.SRPC_ERR_BOUNDS
            assert read_status(st) == (srpc_amd.SRPC_STATUS_BOUNDS, k)
            same(image(arr, lay, n), al.expect_fresh(lay, fill, src, k, old))

    # a foreign envelope byte in a record of the first tile and one of the last
    if lay.envelope:
        first, last = min(3, n - 1), n - 1
        bad = want.copy()
        bad[first * W + len(p.prefix) - 1] ^= 0x40
        bad[last * W + 1] ^= 0x01
        arr, st = Padded(old, shift=shift), status_buf()
        assert p.unpack_aos(Padded(bad).ptr, n * W, n, arr.ptr, stride, offs, st) == 0
        assert read_status(st) == (srpc_amd.SRPC_STATUS_PREFIX, first)
        same(image(arr, lay, n), al.expect_in_place(lay, old, src))


def _cases():
    out = []
    for name, lay in al.LAYOUTS.items():
        ns = al.counts(lay)
        if name in al.OVERSIZED:  # thinned: one tile and less, two tiles and a record
            ns = [n for n in ns if n in (1, 17, 33)]
        out += [pytest.param(name, n, 0, id=f"{name}-n{n}") for n in ns]
    for name in al.ALIGNED_NAMES:  # thinned: a short-wire size below a tile, one past a tile
        lay = al.LAYOUTS[name]
        out += [pytest.param(name, n, s, id=f"{name}-n{n}-shift{s}")
                for s in al.shifts(lay) for n in (17, al.staged_tile(lay) + 1)]
    return out


@pytest.mark.parametrize("name,n,shift", _cases())
def test_aos_layout(name, n, shift):
    check_layout(name, n, shift)


@pytest.fixture
def lay_unpack_hook():
    hook = _lib.lib().srpc_debug_aos_lay_unpack
    hook.argtypes, hook.restype = [ctypes.c_int], ctypes.c_int
    prev = []

    def select(mode):
        prev.append(hook(mode))
    yield select
    if prev:
        hook(prev[0])


@pytest.mark.parametrize("mode", [0, 1], ids=["staged_unpack", "layout_unpack"])
@pytest.mark.parametrize("name", list(al.RUNS) + list(al.NEAR_LAYOUTS))
def test_aos_layout_under_alternative_unpack_families(name, mode, lay_unpack_hook):
    """srpc_debug_aos_lay_unpack picks the unpack family of the two
    compile-time layouts (2, the default, is what test_aos_layout ran).  A run
    layout or a near-layout is none of them: whichever is selected, the bytes
    are the same."""
    lay_unpack_hook(mode)
    check_layout(name, 257)


# ---- refusals ---------------------------------------------------------------------
def _refused(code, lay_kinds, offs, stride, n=40, arr_shift=0, wire_shift=0, alloc_stride=None):
    """pack_aos, unpack_aos and unpack_aos_fill all answer `code`, and neither
    the struct array nor the wire (nor their pads, nor the status) is written."""
    p = GpuPacker(Schema(al.SCHEMA_NAME, tuple((f"f{i}", k) for i, k in enumerate(lay_kinds))))
    rng = np.random.default_rng(stride + len(offs))
    room = n * (alloc_stride or stride)
    recs = rng.integers(0, 256, room, dtype=np.uint8)
    wbytes = rng.integers(0, 256, n * p.record_bytes, dtype=np.uint8)
    fill = bytes(stride)
    calls = [
        lambda a, w, st: p.pack_aos(a.ptr, stride, offs, n, w.ptr),
        lambda a, w, st: p.unpack_aos(w.ptr, w.n, n, a.ptr, stride, offs, st),
        lambda a, w, st: p.unpack_aos_fill(w.ptr, w.n, n, a.ptr, stride, offs, fill, st),
    ]
    for call in calls:
        arr, wire = Padded(recs, shift=arr_shift), Padded(wbytes, shift=wire_shift)
        st = dev(np.full(16, 0x5A, np.uint8))
        with pytest.raises(srpc_amd.SrpcError) as e:
            call(arr, wire, st)
        assert e.value.code == code
        assert arr.read().tobytes() == recs.tobytes() and wire.read().tobytes() == wbytes.tobytes()
        if code != _lib.SRPC_E_ALIGN or not wire_shift:  # (a misaligned wire is found after the status reset)
            assert host(st, 16).tobytes() == b"\x5a" * 16
    return p


def test_aos_refuses_overlapping_fields():
    """Two fields sharing bytes would make the fields' sizes add up to a
    stride they do not cover (the staged unpack would then skip reading the
    struct tile and write LDS garbage over the unnamed bytes)."""
    _refused(_lib.SRPC_E_INVALID, [al.I32, al.I32], [0, 0], 8)          # same offset; sizes sum to the stride
    _refused(_lib.SRPC_E_INVALID, [al.I64, al.I32], [0, 4], 16)         # the second inside the first
    _refused(_lib.SRPC_E_INVALID, [al.I16, al.I8, al.I32], [4, 5, 0], 8)  # out of order, the middle two collide
    _refused(_lib.SRPC_E_INVALID, [al.I8] * 32, list(range(31)) + [7], 32)
    # adjacent fields in any order are fine
    check_layout("i8x3_rot_s3", 17)


def test_aos_refuses_field_past_the_stride():
    _refused(_lib.SRPC_E_INVALID, [al.I32] * 4, [8, 12, 16, 20], 20, alloc_stride=24)
    _refused(_lib.SRPC_E_INVALID, [al.I64], [8], 8, alloc_stride=16)


def test_aos_refuses_unnatural_alignment():
    q = [al.I32] * 4
    _refused(_lib.SRPC_E_ALIGN, q, [8, 12, 18, 20], 24)            # a field offset off its size
    _refused(_lib.SRPC_E_ALIGN, [al.I64, al.I8], [8, 16], 20)     # a stride off its largest field
    _refused(_lib.SRPC_E_ALIGN, q, [8, 12, 16, 20], 24, arr_shift=2)   # the array base off its largest field
    _refused(_lib.SRPC_E_ALIGN, [al.I64], [8], 16, arr_shift=4)
    _refused(_lib.SRPC_E_ALIGN, [al.I16, al.I8], [0, 2], 4, arr_shift=1)


@pytest.mark.parametrize("name,shift", [("outer", 0), ("outer", 8)], ids=["staged", "per_field"])
def test_aos_refuses_wire_8_bytes_off_16(name, shift):
    """As test_aos_run_unpack_refuses_wire_8_bytes_off_16 does for the run
    layouts: the staged and per-field kernels move the wire in 16-byte pieces
    too, and every entry point refuses one that is not 16-byte aligned."""
    lay = al.LAYOUTS[name]
    _refused(_lib.SRPC_E_ALIGN, list(lay.kinds), list(lay.offsets), lay.stride, arr_shift=shift, wire_shift=8)
    check_layout(name, 40, shift)
