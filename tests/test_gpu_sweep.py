"""SRPC_TUNE_SWEEP: the DWORD kernels walk their blocks upwards or downwards
(bit 0 pack, bit 1 unpack) and the bytes never change.

The kernels can only go wrong at block and tail edges, so the sizes sit
around one lane, one x4 quad, one workgroup (256 records) and a few blocks;
capped grids (1, 3) force the grid-stride loop with block counts that are and
are not multiples of the grid.  Every output is a slice between 256-byte
sentinel pads of one larger tensor, so a wrong block number shows up as a
failed assert on the pads.  SRPC_TUNE_UNPACK_NONTEMPORAL (unpack's load/store
flavour apart from pack's) is checked the same way.
"""
import numpy as np
import pytest

import oracle
from srpc_amd import (NUMBER, QUAD, TWO_NUMBERS, GpuPacker, Schema, SrpcError, SRPC_ERR_BOUNDS,
                      SRPC_PATH_DWORD, SRPC_STATUS_BOUNDS, _lib)

gpu = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 256

# W = 1, 2, 4 run the tuning matrix; W = 3 (an 8-byte and a 4-byte field)
# runs the one untuned instantiation launch_dword_v<W, 4, 0>
SCHEMAS = {
    "number": NUMBER,
    "two": TWO_NUMBERS,
    "quad": QUAD,
    "i64_i32": Schema.of("Odd", ("x", "int64"), ("y", "int32")),
}

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 8 * 256 * 4 + 1]

# (records_per_lane, iters, grid): every iters and both records_per_lane with
# a full grid (0) and with capped ones.  At n = 8193, (1, 1, 3) has 33 blocks
# (a multiple of the grid), (1, 2, 3) 17 and (4, 1, 3) 8 (not multiples).
CONFIGS = [(1, 1, 0), (4, 1, 0), (1, 1, 3), (1, 2, 3), (4, 1, 3), (1, 4, 1), (4, 2, 1), (1, 8, 3),
           (4, 8, 0), (4, 4, 3)]


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():  # pragma: no cover - CPU container
        pytest.skip("no GPU")
    return torch


class Guarded:
    """Slices of the given byte sizes inside one sentinel-filled device tensor:
    PAD sentinel bytes before, between and after them, every slice 256-byte
    aligned (the x4 kernels need 16)."""

    def __init__(self, sizes):
        torch = _torch()
        self.spans = []
        at = PAD
        for s in sizes:
            self.spans.append((at, s))
            at += -(-max(s, 1) // PAD) * PAD + PAD
        self.t = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        assert self.t.data_ptr() % 256 == 0
        self.slices = [self.t[a:a + max(s, 1)] for a, s in self.spans]

    def read(self):
        """Host copies of the slices, after checking every byte outside them."""
        h = self.t.cpu().numpy()
        outside = np.ones(h.size, bool)
        for a, s in self.spans:
            outside[a:a + s] = False
        assert (h[outside] == SENTINEL).all(), "bytes written outside the output"
        return [h[a:a + s] for a, s in self.spans]


def _columns(kinds, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n * oracle.KIND_SIZE[k], dtype=np.uint8).view(oracle.KIND_DTYPE[k])
            for k in kinds]


def _upload(a):
    torch = _torch()
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.empty(max(b.size, 16), dtype=torch.uint8, device="cuda:0")
    t[:b.size].copy_(torch.from_numpy(b.copy()))
    return t


def _status():
    return _torch().zeros(16, dtype=_torch().uint8, device="cuda:0")


def _read_status(t):
    b = t.cpu().numpy()
    return int(b[:4].view(np.uint32)[0]), int(b[8:16].view(np.uint64)[0])


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("schema", sorted(SCHEMAS))
def test_sweep_pack_unpack_vs_oracle(schema, n):
    sch = SCHEMAS[schema]
    kinds = sch.kinds
    cols = _columns(kinds, n, n * 31 + len(kinds))
    want = oracle.pack(kinds, cols, n)
    p = GpuPacker(sch)
    assert p.path == SRPC_PATH_DWORD and p.record_bytes * n == len(want)
    dcols = [_upload(c) for c in cols]
    dwire = _upload(np.frombuffer(want, np.uint8))
    col_bytes = [c.nbytes for c in cols]
    packed, unpacked = set(), set()
    for rpl, it, grid in CONFIGS:
        for sweep in range(4):
            p.tune(rpl, it, grid=grid, sweep=sweep)
            w = Guarded([len(want)])
            p.pack(dcols, n, w.slices[0])
            got = w.read()[0].tobytes()
            assert got == want, (rpl, it, grid, sweep)
            packed.add(got)
            out = Guarded(col_bytes)
            rc = p.unpack(dwire, len(want), n, out.slices)
            assert rc == 0
            back = out.read()
            for a, b in zip(cols, back):
                assert a.tobytes() == b.tobytes(), (rpl, it, grid, sweep)
            unpacked.add(b"".join(b.tobytes() for b in back))
    assert len(packed) == 1 and len(unpacked) == 1  # identical for every sweep value and variant


@gpu
@pytest.mark.parametrize("schema", sorted(SCHEMAS))
def test_unpack_nontemporal_identical(schema):
    """SRPC_TUNE_UNPACK_NONTEMPORAL picks unpack's load/store flavour apart
    from pack's; SRPC_TUNE_NONTEMPORAL still sets both.  Bytes never change."""
    sch = SCHEMAS[schema]
    kinds, n = sch.kinds, 2049
    cols = _columns(kinds, n, 5)
    want = oracle.pack(kinds, cols, n)
    p = GpuPacker(sch)
    dcols = [_upload(c) for c in cols]
    dwire = _upload(np.frombuffer(want, np.uint8))
    for nt in (0, 3):
        for unt in range(4):
            p.tune(records_per_lane=4, nontemporal=nt, unpack_nontemporal=unt, sweep=unt ^ 1)
            w = Guarded([len(want)])
            p.pack(dcols, n, w.slices[0])
            assert w.read()[0].tobytes() == want, (nt, unt)
            out = Guarded([c.nbytes for c in cols])
            assert p.unpack(dwire, len(want), n, out.slices) == 0
            for a, b in zip(cols, out.read()):
                assert a.tobytes() == b.tobytes(), (nt, unt)


@gpu
@pytest.mark.parametrize("sweep", [0, 2])
@pytest.mark.parametrize("n", [5, 1025, 2049])
@pytest.mark.parametrize("schema", sorted(SCHEMAS))
def test_sweep_truncated_wire_bounds(schema, n, sweep):
    """wire_len = k*stride + 5 short of n records: the fit whole records are
    decoded, nothing at or past them is written, and BOUNDS is reported at
    the first record that does not fit.  That is record k for every stride
    above 5; the 5 spare bytes hold one more 4-byte Number record, so there
    it is k + 1 (n_fit = wire_len / stride, include/srpc_gpu.h)."""
    sch = SCHEMAS[schema]
    kinds = sch.kinds
    cols = _columns(kinds, n, n * 17 + len(kinds))
    want = oracle.pack(kinds, cols, n)
    dwire = _upload(np.frombuffer(want, np.uint8))  # whole wire present: a read past k would decode real values
    p = GpuPacker(sch)
    stride = p.record_bytes
    for rpl, it, grid in [(1, 1, 0), (4, 1, 0), (1, 2, 3), (4, 2, 1)]:
        p.tune(rpl, it, grid=grid, sweep=sweep)
        for k in sorted({0, 1, n // 2, n - 2, n - 1}):
            fit = (k * stride + 5) // stride
            assert fit == (k + 1 if stride == 4 else k)
            if fit >= n:
                continue
            out = Guarded([c.nbytes for c in cols])
            st = _status()
            rc = p.unpack(dwire, k * stride + 5, n, out.slices, st)
            assert rc == SRPC_ERR_BOUNDS
            back = out.read()
            assert _read_status(st) == (SRPC_STATUS_BOUNDS, fit)
            for c, b, kind in zip(cols, back, kinds):
                sz = oracle.KIND_SIZE[kind]
                assert b[:fit * sz].tobytes() == c.tobytes()[:fit * sz], (rpl, it, grid, k)
                assert (b[fit * sz:] == SENTINEL).all(), (rpl, it, grid, k)


@gpu
@pytest.mark.parametrize("sweep", [0, 1, 2, 3])
def test_sweep_zero_records(sweep):
    p = GpuPacker(QUAD)
    p.tune(sweep=sweep)
    bufs = Guarded([64] * 5)
    assert p.pack(bufs.slices[:4], 0, bufs.slices[4]) == 0
    assert p.unpack(bufs.slices[4], 64, 0, bufs.slices[:4]) == 0
    _torch().cuda.synchronize()
    assert (bufs.t.cpu().numpy() == SENTINEL).all()


@gpu
@pytest.mark.parametrize("sweep", [0, 3])
def test_sweep_timed_call_brackets_both_launches(sweep):
    """records_per_lane = 4 makes two launches, the x4 body and the
    one-record tail, the tail first when descending: srpc_time_next_call's
    events bracket both in either order (begin of the first launched, end of
    the last), and the call after it is not armed."""
    torch = _torch()
    import srpc_amd
    n = 4 * 300_000 + 3
    cols = _columns(NUMBER.kinds, n, 9)
    want = oracle.pack(NUMBER.kinds, cols, n)
    p = GpuPacker(NUMBER)
    p.tune(records_per_lane=4, iters=1, sweep=sweep)
    dcols = [_upload(c) for c in cols]
    w = Guarded([len(want)])
    out = Guarded([c.nbytes for c in cols])
    s = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    for e in ev:
        e.record(s)
    torch.cuda.synchronize()
    srpc_amd.time_next_call(ev[0], ev[1])
    p.pack(dcols, n, w.slices[0], stream=s)
    ev[2].record(s)
    srpc_amd.time_next_call(ev[3], ev[4])
    p.unpack(w.slices[0], len(want), n, out.slices, stream=s)
    ev[5].record(s)
    torch.cuda.synchronize()
    # begin before end, and the end not after an event recorded behind the call
    assert 0 < ev[0].elapsed_time(ev[1]) < 100 and 0 < ev[3].elapsed_time(ev[4]) < 100
    assert ev[1].elapsed_time(ev[2]) >= 0 and ev[4].elapsed_time(ev[5]) >= 0
    assert w.read()[0].tobytes() == want
    assert out.read()[0].tobytes() == cols[0].tobytes()


def test_sweep_knob_validation():
    """SRPC_TUNE_SWEEP (knob 14) takes 0..3 and nothing else; no GPU needed.
    The plan has no getter, so the Python keyword is checked the same way:
    every valid value is accepted and a bad one raises INVALID."""
    L = _lib.lib()
    for sch in (QUAD, SCHEMAS["i64_i32"]):
        p = GpuPacker(sch)
        for v in range(4):
            assert L.srpc_plan_tune(p._h, 14, v) == _lib.SRPC_OK
            p.tune(sweep=v)
        for v in (-1, 4, 5, 255, 2**31 - 1, -2**31):
            assert L.srpc_plan_tune(p._h, 14, v) == _lib.SRPC_E_INVALID
        with pytest.raises(SrpcError) as e:
            p.tune(sweep=4)
        assert e.value.code == _lib.SRPC_E_INVALID
        p.tune(records_per_lane=4, iters=2, grid=3, sweep=2)  # beside the other knobs
        # SRPC_TUNE_UNPACK_NONTEMPORAL (knob 15): the same two bits as knob 3
        for v in range(4):
            assert L.srpc_plan_tune(p._h, 15, v) == _lib.SRPC_OK
            p.tune(nontemporal=3 - v, unpack_nontemporal=v)
        for v in (-1, 4, 16):
            assert L.srpc_plan_tune(p._h, 15, v) == _lib.SRPC_E_INVALID
