"""Every size-unbounded device call, once, on a wire whose byte positions pass
2^32 (include/srpc_gpu.h: the batch calls take uint64_t n and wire_len with no
cap; the frame calls refuse 4 GiB and are tests/test_gpu_frames_top.py's).

The batches are tests/giant.py's: every byte of the reference wire and of the
inputs is the CPU oracle's, concatenated on the device with torch.cat alone.
Outputs are 0xA5-filled and sit between two 1 MiB guards that must survive;
whole arrays are compared on the device, and two windows (around byte 2^32 and
the end) are downloaded and compared on the host with the oracle's own bytes of
those windows, in case a device compare is itself mistaken.  A wrapped 32-bit
position lands inside the allocation: the aperiodic data (asserted by the
helper) makes it a mismatch.

Each test prints one `PAST4G` line: the case, the plan's path, n, W, the record
that holds byte 2^32 and the byte's position in it, and the call's wall time.

What was read before the first run (where positions widen, what bounds a cast):
- DWORD (k_(un)pack_dword, _x4): the block number is a uint64_t loop variable from
  blockIdx.x, slot r0 = b * (kBlock * ITER) + lane and wire + r * 4W, column + (r << lg)
  are 64-bit; no position is narrowed; launch_dword_v refuses more than 2^31 - 1 blocks.
- TILE (k_pack_tile, _flat, k_unpack_tile): tile is a uint64_t loop variable, rbase =
  tile * R; the uint32_t values (nr, nbytes, tbytes, chunk c, ph) count inside one tile
  image of at most 48 KiB; the grid is min(tiles, 2^30), the kernels grid-stride.
- one-wave tiles: rbase = uint64_t(blockIdx.x) * R; the grid is n / R rounded up, below
  2^26 by the switch in srpc_gpu_pack / _unpack (64 lanes each: at most 2^32 lanes).
- rec.hip: tile = blockIdx.x widened, q = (tile * K + k) * 64 + lane and the tile's wire
  offset tile * (uint64_t(TR) * STRIDE) are 64-bit, `int c` counts a tile's chunks;
  k_pack_env: c0 = uint64_t(blockIdx.x) * (U * kBlock), period T = c / S in 64 bits, the
  int32_t e, o and uint32_t tc, lb count inside one 16-record period; tiles and chunk
  blocks above 2^31 - 1 are refused (SRPC_E_UNSUPPORTED) before any launch.
- aos.hip: run kernels e = uint64_t(blockIdx.x) * kBlock + lane, recs + e * rstride and
  wire + e * W; lay / piece kernels t0 = uint64_t(blockIdx.x) * TR, their uint32_t byte
  counts are those of 256 structs of at most 256 bytes; staged kernels rbase widened, nr *
  rstride inside the 24 KiB tile; every grid above 2^31 - 1 is refused or falls through.
- var.hip, pack: r0 = t * kBlock and a tile's base r0 * fixed_bytes + chars_before are
  64-bit; lofs[i], cb - c0, lo - A, len are narrowed only on the branch whose span fits
  the LDS image (h + total <= img_cap <= 64 KiB) or the stage; the walk fallback keeps
  uint64_t p0, lo, hi and narrows counts of at most 16 bytes.  Unpack: grid n / 256
  refused above 2^31 - 1; pos - start, p - sw are offsets into the tile's staged window;
  s_ioff saturates at 2^32 - 1 and is used only inside the image.
- sdx.hip: block b and b0 = b * kSB are 64-bit everywhere; the uint32_t o and J values
  are offsets from the staged block's base (under 2 * kSB); more than 2^31 - 1 blocks or
  W >= 2^40 are refused.
No signed 32-bit index of a global position was found.

What these tests cannot establish, and why:
- Which kernel ran is not observable through the ABI (srpc_plan_path names the path only).  The
  one-wave cases state which side of the `n / R < 2^26` switch they mean by restating
  configure_wave_tile's R = 16 * max(1, target / (16 * stride)) in `_wave_records`: if that
  formula moves, these asserts no longer say which kernel ran.  The AoS cases pick layouts
  that aos.hip's launch_aos_run / launch_aos_lay / staged_fits send to the run, lay / piece and
  staged kernels as written today; nothing asserts it.
- tile_full_grid is hard-wired on (plan.h, configure_tile) and srpc_plan_tune has no knob for
  it: the grid-stride form of k_pack_tile / k_unpack_tile (a grid of tile_grid workgroups) does
  not run here, only the one-workgroup-per-tile form.
- Fixed records of 16 bytes and of 1 byte meet byte 2^32 on a record boundary by arithmetic.
- The stream decode's other two `W < 2^32` tests (the landing-slot window, chunk_mask_z against
  chunk_mask) choose between two filters that give the same candidates for every string length
  under 2^32: flipped, they change no output, so only k_sx_repair's test is pinned, by
  test_unpack_var_stream_missed_blocks.
"""

import time

import numpy as np
import pytest

import oracle
import srpc_amd
from srpc_amd import (NUMBER, QUAD, SQUARE_METHOD, GpuPacker, Schema, SRPC_ERR_BOUNDS, SRPC_PATH_DWORD,
                      SRPC_PATH_TILE, SRPC_PATH_VAR, SRPC_STATUS_BOUNDS)
from tests import aos_layouts as AL
from tests import giant

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
B = 2**32
GUARD = 1 << 20
GIB = 1 << 30
WIN = 32 * 1024  # half a host window, in bytes
NWIN = 2048      # ... of an offsets array, in entries
BUILD = dict(device=DEV)  # giant.build's arguments: the boundary is its default, 2^32
I8, I16, I32, I64, BOOL, CHAR, STR = (oracle.INT8, oracle.INT16, oracle.INT32, oracle.INT64, oracle.BOOL,
                                      oracle.CHAR, oracle.STRING)
SIX = [BOOL, I8, CHAR, I16, I32, I64]
GOOD = (0, 2**64 - 1)


def _schema(name, kinds):
    return Schema(name, tuple((f"f{i}", k) for i, k in enumerate(kinds)))


# ---- outputs between guards ----------------------------------------------------
class Guarded:
    """nbytes of 0xA5 between two 1 MiB guards of 0xA5 (`shift`: the output's address modulo 16)."""

    def __init__(self, nbytes, shift=0):
        self.nbytes, self.at = nbytes, GUARD + shift
        self.raw = torch.full((2 * GUARD + nbytes + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        self.view = self.raw[self.at:self.at + nbytes]
        assert (self.view.data_ptr() - shift) % 16 == 0

    def check_guards(self, what):
        lo, hi = self.raw[:self.at], self.raw[self.at + self.nbytes:]
        assert not bool((lo != 0xA5).any()), f"{what}: the guard before the output was written"
        assert not bool((hi != 0xA5).any()), f"{what}: the guard behind the output was written"


def need(nbytes, what, limit=24 * GIB):
    """The test's device memory, all told: under `limit`, and free now (else the test skips and says so)."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    assert nbytes < limit, f"{what}: a test of {nbytes / GIB:.1f} GiB"
    if free < nbytes:
        print(f"{what}: needs {nbytes / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB free")
        pytest.skip(f"{what}: needs {nbytes / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB free")


def u8(t):
    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def same(out, ref, what):
    """Whole arrays on the device; on a mismatch the first differing 256 bytes."""
    out, ref = u8(out), u8(ref)
    assert out.numel() == ref.numel(), f"{what}: {out.numel()} bytes against {ref.numel()}"
    if torch.equal(out, ref):
        return
    step = 1 << 28
    for lo in range(0, out.numel(), step):
        ne = out[lo:lo + step] != ref[lo:lo + step]
        if bool(ne.any()):
            i = lo + int(ne.to(torch.uint8).argmax())
            got = out[i:i + 256].cpu().numpy().tobytes().hex()
            want = ref[i:i + 256].cpu().numpy().tobytes().hex()
            pytest.fail(f"{what}: first difference at byte {i} (= 2^32 {i - B:+d})\n got  {got}\n want {want}")
    pytest.fail(f"{what}: torch.equal says different, no chunk does")


def host_same(out, lo, hi, want, what):
    """Bytes [lo, hi) of a device array against the oracle's, on the host."""
    got = u8(out)[lo:hi].cpu().numpy()
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.tobytes() == want.tobytes(), f"{what}: host window [{lo}, {hi}) differs from the oracle's bytes"


def status_buf():
    return torch.full((16,), 0x5A, dtype=torch.uint8, device=DEV)


def read_status(st):
    b = st.cpu().numpy()
    return int(b[:4].view(np.uint32)[0]), int(b[8:16].view(np.uint64)[0])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = fn()
    torch.cuda.synchronize()
    return rc, (time.perf_counter() - t0) * 1e3


def report(case, p, g, ms, extra=""):
    print(f"PAST4G {case}: path={p.path} n={g.n} W={g.W} (2^32{g.W - B:+d}) record_at_2^32={g.rec_index} "
          f"byte_in_record={g.into} call_ms={ms:.1f} {extra}")


def wire_windows(out, g, what):
    host_same(out, B - WIN, B + WIN, g.wire_window(B - WIN, B + WIN), what + " around 2^32")
    host_same(out, g.W - 2 * WIN, g.W, g.wire_window(g.W - 2 * WIN, g.W), what + " tail")


def col_windows(out, g, f, what):
    """A fixed column around the record that holds byte 2^32, and its end."""
    sz = oracle.KIND_SIZE[g.kinds[f]]
    per = min(2 * WIN // sz, g.n)
    a = max(0, g.rec_index - per // 2)
    host_same(out, a * sz, (a + per) * sz, g.col_window(f, a, a + per), f"{what} column {f} around 2^32")
    host_same(out, (g.n - per) * sz, g.n * sz, g.col_window(f, g.n - per, g.n), f"{what} column {f} tail")


# ---- the batches: one alive at a time ----------------------------------------
FIXED = {  # kinds, T::name, the request's method or None
    "quad": (QUAD.kinds, "Quad", None),
    "i32_i64": ([I32, I64], "S", None),
    "six": (SIX, "all_kinds", None),
    "six_request": (SIX, "all_kinds", "Svc_servicer::m"),
    "square_request": (NUMBER.kinds, "Number", SQUARE_METHOD),
    "i8_i16": ([I8, I16], "S", None),
    "i8": ([I8], "S", None),
}
ONE_STRING = [I8, CHAR, I64, STR]          # multiple_primitives
TWO_STRINGS = [STR, I32, I8, STR, I16]     # two strings with fixed fields between
VAR = {"one_string": ONE_STRING, "two_strings": TWO_STRINGS}


@pytest.fixture(scope="module")
def batch(request):
    """request.param: a FIXED name, ("aos", an AOS name), or (a VAR name, straddle[, "zero_heavy"])."""
    torch.cuda.empty_cache()
    if isinstance(request.param, tuple) and request.param[0] == "aos":
        g = giant.build(list(AOS[request.param[1]].kinds), b"", "short", **BUILD)
    elif isinstance(request.param, tuple):
        name, straddle = request.param[:2]
        g = giant.build(VAR[name], b"", straddle, zero_heavy=len(request.param) > 2, **BUILD)
    else:
        kinds, name, method = FIXED[request.param]
        g = giant.build(kinds, oracle.request_prefix(method, name) if method else b"", "short", **BUILD)
    assert g.boundary == B and g.W > B + BUILD.get("tail", 64 * giant.MIB) and g.n % 2 == 1
    yield g
    g.free()
    del g
    torch.cuda.empty_cache()


def _plan(name):
    kinds, tname, method = FIXED[name]
    return GpuPacker.for_request(_schema(tname, kinds), method) if method else GpuPacker(_schema(tname, kinds))


def _wave_records(target, stride):
    """configure_wave_tile's records per wave tile, restated."""
    return 16 * max(1, target // (16 * stride))


# (batch, variant): the plan's path, then the knobs
FIXED_CASES = [
    ("quad", "dword_x4"),          # k_(un)pack_dword_x4 and the remainder's k_(un)pack_dword
    ("quad", "dword_x1"),          # one record per lane
    ("quad", "dword_down"),        # both directions walk the records downwards
    ("quad", "tile"),              # equal field widths: k_pack_tile / k_unpack_tile
    ("i32_i64", "dword"),          # 12 bytes, not all fields 4 bytes: the plain dword kernels
    ("six", "rec"),                # rec.hip's k_(un)pack_rec for the whole tiles, the generic kernels for the rest
    ("six", "tile"),               # k_pack_tile_flat / k_unpack_tile
    ("six_request", "tile"),       # the prefix template at high positions, every prefix byte checked
    ("square_request", "rec"),     # k_pack_env's chunk count, k_unpack_rec behind an envelope
    ("i8_i16", "wave"),            # one-wave tiles, 2.1 M of them
    ("i8", "wave"),                # n > 2^32
    ("i8", "wave80"),              # n / R just under the 2^26 switch: 54 M one-wave tiles
    ("i8", "wave16"),              # n / R past it: the workgroup tiles
]


def _configure(name, variant, n):
    p = _plan(name)
    S = p.record_bytes
    if variant.startswith("dword"):
        assert p.path == SRPC_PATH_DWORD
        if variant in ("dword_x4", "dword_down"):
            p.tune(records_per_lane=4)
        if variant == "dword_x1":
            p.tune(records_per_lane=1)
        if variant == "dword_down":
            p.tune(sweep=3)
    elif variant == "tile":
        p.force_path(SRPC_PATH_TILE)
        p.tune(rec_kernel=0)
        assert p.path == SRPC_PATH_TILE
    elif variant == "rec":
        assert p.path == SRPC_PATH_TILE
        p.tune(rec_kernel=2)
    elif variant == "wave":
        assert p.path == SRPC_PATH_TILE and S < 16
        assert n // _wave_records(2048, S) < 2**26 and n // _wave_records(3072, S) < 2**26
    elif variant == "wave80":
        p.tune(wave_pack_bytes=80, wave_unpack_bytes=80)
        assert _wave_records(80, S) == 80 and 2**25 < n // 80 < 2**26
    elif variant == "wave16":
        p.tune(wave_pack_bytes=16, wave_unpack_bytes=16)
        assert _wave_records(16, S) == 16 and n // 16 >= 2**26
    return p


def _fixed_id(c):
    return f"{c[0]}-{c[1]}"


@pytest.mark.parametrize("batch,variant", FIXED_CASES, indirect=["batch"], ids=[_fixed_id(c) for c in FIXED_CASES])
def test_pack(batch, variant, request):
    g = batch
    name = request.node.callspec.params["batch"]
    need(3 * g.W + GIB, f"pack {name}")
    p = _configure(name, variant, g.n)
    assert p.wire_bytes(g.n) == g.W and p.prefix == g.prefix
    out = Guarded(g.W)
    _, ms = timed(lambda: p.pack(g.cols, g.n, out.view))
    report(f"pack {name}/{variant}", p, g, ms)
    out.check_guards("pack")
    same(out.view, g.ref, "wire")
    wire_windows(out.view, g, "wire")


@pytest.mark.parametrize("batch,variant", FIXED_CASES, indirect=["batch"], ids=[_fixed_id(c) for c in FIXED_CASES])
def test_unpack(batch, variant, request):
    g = batch
    name = request.node.callspec.params["batch"]
    need(3 * g.W + GIB, f"unpack {name}")
    p = _configure(name, variant, g.n)
    outs = [Guarded(c.numel() * c.element_size()) for c in g.cols]
    st = status_buf()
    rc, ms = timed(lambda: p.unpack(g.ref, g.W, g.n, [o.view for o in outs], st))
    report(f"unpack {name}/{variant}", p, g, ms)
    assert rc == 0 and read_status(st) == GOOD
    for f, (o, c) in enumerate(zip(outs, g.cols)):
        o.check_guards(f"unpack column {f}")
        same(o.view, c, f"column {f}")
        col_windows(o.view, g, f, "unpack")


# ---- the short-wire rule ---------------------------------------------------------
@pytest.mark.parametrize("batch", ["quad"], indirect=True)
@pytest.mark.parametrize("call", ["unpack", "unpack_aos"])
def test_short_wire_past_4gib(batch, call):
    """wire_len = 2^32 + 24: SRPC_ERR_BOUNDS, first_bad_record = wire_len / 16 = 2^28 + 1 (a value a
    truncated division or a 32-bit byte count would mangle); the records that fit are decoded, the rest untouched."""
    g = batch
    need(3 * g.W + GIB, f"short wire {call}")
    p = GpuPacker(QUAD)
    wire_len = B + 24
    n_fit = wire_len // 16
    assert n_fit == B // 16 + 1 and n_fit < g.n
    st = status_buf()
    if call == "unpack":
        outs = [Guarded(4 * g.n) for _ in range(4)]
        rc, ms = timed(lambda: p.unpack(g.ref, wire_len, g.n, [o.view for o in outs], st))
    else:
        lay = AL.PLAIN["quad_plain"]
        out = Guarded(16 * g.n)
        rc, ms = timed(lambda: p.unpack_aos(g.ref, wire_len, g.n, out.view, lay.stride, lay.offsets, st))
    report(f"short wire {call}", p, g, ms)
    assert rc == SRPC_ERR_BOUNDS
    assert read_status(st) == (SRPC_STATUS_BOUNDS, n_fit)
    if call == "unpack":
        for f, o in enumerate(outs):
            o.check_guards(f"column {f}")
            same(o.view[:4 * n_fit], u8(g.cols[f])[:4 * n_fit], f"column {f}, the records that fit")
            assert not bool((o.view[4 * n_fit:] != 0xA5).any()), f"column {f}: a record past the wire was written"
            host_same(o.view, 4 * (n_fit - NWIN), 4 * n_fit, g.col_window(f, n_fit - NWIN, n_fit), f"column {f}")
    else:
        out.check_guards("structs")
        same(out.view[:16 * n_fit], g.ref[:16 * n_fit], "the structs that fit")
        assert not bool((out.view[16 * n_fit:] != 0xA5).any()), "a struct past the wire was written"
        host_same(out.view, B - WIN, B + 16, g.wire_window(B - WIN, B + 16), "structs")


# ---- struct arrays -----------------------------------------------------------------
AOS = {
    # layout: the kernels aos.hip picks for it
    "quad_plain": AL.PLAIN["quad_plain"],                        # the struct is the wire body: the staged kernels
    "quad_run": AL.RUNS["run16_at0_s24"],                        # Quad and 8 bytes it does not name: the run kernels
    "six_lay": AL.Layout(AL.ALL6, AL.LAY_ALL_KINDS_V[0], AL.LAY_ALL_KINDS_V[2], None, 8),  # lay / piece kernels
    "six_staged": AL.NEAR_LAYOUTS["all_s32"][0],                 # next to that layout: the staged kernels
}


def _fill_record(lay):
    rng = np.random.default_rng(lay.stride)
    f = rng.integers(0, 256, lay.stride, dtype=np.uint8)
    f[f == 0xA5] = 0x5B  # a fill byte is never the 0xA5 of an untouched output
    return f


def _struct_array(g, lay, pattern):
    """The expected struct array, with torch: `pattern` repeated, the leaf bytes laid over it."""
    S = torch.from_numpy(pattern).to(DEV).repeat(g.n)
    S2 = S.view(g.n, lay.stride)
    for f, (o, k) in enumerate(zip(lay.offsets, lay.kinds)):
        sz = oracle.KIND_SIZE[k]
        S2[:, o:o + sz] = u8(g.cols[f]).view(g.n, sz)
    return S


def _host_structs(g, lay, pattern, a, b):
    out = np.tile(pattern, (b - a, 1))
    for f, (o, k) in enumerate(zip(lay.offsets, lay.kinds)):
        sz = oracle.KIND_SIZE[k]
        out[:, o:o + sz] = g.col_window(f, a, b).view(np.uint8).reshape(b - a, sz)
    return out


def struct_windows(out, g, lay, pattern, what):
    per = 2 * WIN // lay.stride
    for a, tag in [(g.rec_index - per // 2, "around 2^32"), (g.n - per, "tail")]:
        host_same(out, a * lay.stride, (a + per) * lay.stride, _host_structs(g, lay, pattern, a, a + per),
                  f"{what} {tag}")


def same_in_place(out, S, lay, what):
    """Leaf bytes as S's, every other byte still 0xA5 (row chunks: no array-sized temporary)."""
    m = torch.from_numpy(AL.field_mask(lay)).to(DEV)
    o2, s2 = out.view(-1, lay.stride), S.view(-1, lay.stride)
    step = 1 << 23
    for lo in range(0, o2.shape[0], step):
        o, s = o2[lo:lo + step], s2[lo:lo + step]
        assert torch.equal(o[:, m], s[:, m]), f"{what}: a leaf byte differs in structs [{lo}, {lo + step})"
        if not bool(m.all()):
            assert not bool((o[:, ~m] != 0xA5).any()), f"{what}: a byte no leaf covers was written in [{lo}, {lo + step})"


@pytest.mark.parametrize("batch", [("aos", k) for k in AOS], indirect=True, ids=list(AOS))
def test_aos(batch, request):
    """pack_aos, unpack_aos_fill and unpack_aos of one layout (the expected struct array is built
    once; the batch is this test's alone, and its columns are freed once the array is made)."""
    g = batch
    key = request.node.callspec.params["batch"][1]
    lay = AOS[key]
    asz = g.n * lay.stride
    need(g.W + 2 * asz + GIB, f"aos {key}")
    p = GpuPacker(_schema("S", list(lay.kinds)))
    assert p.path == (SRPC_PATH_DWORD if lay.kinds == (I32,) * 4 else SRPC_PATH_TILE) and p.record_bytes * g.n == g.W
    fill = _fill_record(lay)
    S = _struct_array(g, lay, fill)
    g.cols = None
    torch.cuda.empty_cache()
    assert giant.wrap_visible(S, B, BUILD.get("win", 4096), "struct array")

    out = Guarded(g.W)
    _, ms = timed(lambda: p.pack_aos(S, lay.stride, lay.offsets, g.n, out.view))
    report(f"pack_aos {key} stride={lay.stride}", p, g, ms)
    out.check_guards("pack_aos")
    same(out.view, g.ref, "pack_aos wire")
    wire_windows(out.view, g, "pack_aos wire")
    del out

    out = Guarded(asz)
    st = status_buf()
    rc, ms = timed(lambda: p.unpack_aos_fill(g.ref, g.W, g.n, out.view, lay.stride, lay.offsets, fill.tobytes(), st))
    report(f"unpack_aos_fill {key} stride={lay.stride}", p, g, ms)
    assert rc == 0 and read_status(st) == GOOD
    out.check_guards("unpack_aos_fill")
    same(out.view, S, "unpack_aos_fill structs")
    struct_windows(out.view, g, lay, fill, "unpack_aos_fill")
    del out

    out = Guarded(asz)
    st = status_buf()
    rc, ms = timed(lambda: p.unpack_aos(g.ref, g.W, g.n, out.view, lay.stride, lay.offsets, st))
    report(f"unpack_aos {key} stride={lay.stride}", p, g, ms)
    assert rc == 0 and read_status(st) == GOOD
    out.check_guards("unpack_aos")
    same_in_place(out.view, S, lay, "unpack_aos")
    struct_windows(out.view, g, lay, np.full(lay.stride, 0xA5, np.uint8), "unpack_aos")


# ---- string schemas -----------------------------------------------------------------
VAR_BATCHES = [(name, st) for name in VAR for st in ("short", "long")]
VAR_IDS = [f"{n}-{s}" for n, s in VAR_BATCHES]


def _var_plan(g, vk=None):
    p = GpuPacker(_schema("S", g.kinds))
    assert p.path == SRPC_PATH_VAR and p.record_bytes == 0
    if vk is not None:
        p.tune(var_kernel=vk)
    return p


def _var_report(case, p, g, ms, extra=""):
    longs = f"long_records={g.long_records}" if g.long_records else ""
    report(case, p, g, ms, f"{longs} {extra}")


def _scratch(nbytes, byte=0xA5, align=16):
    raw = torch.full((nbytes + 2 * align,), byte, dtype=torch.uint8, device=DEV)
    at = (-raw.data_ptr()) % align
    return raw, raw[at:at + nbytes]


def _var_outputs(g):
    """Per field: the column (a string field: room for W bytes), its offsets (n + 1) or None."""
    outs, offs = [], []
    for k in g.kinds:
        if k == STR:
            outs.append(Guarded(g.W))
            offs.append(Guarded(8 * (g.n + 1)))
        else:
            outs.append(Guarded(g.n * oracle.KIND_SIZE[k]))
            offs.append(None)
    return outs, offs


def _check_var_outputs(g, outs, offs, what):
    r = g.rec_index
    for f, k in enumerate(g.kinds):
        outs[f].check_guards(f"{what} column {f}")
        if k != STR:
            same(outs[f].view, g.cols[f], f"{what} column {f}")
            col_windows(outs[f].view, g, f, what)
            continue
        offs[f].check_guards(f"{what} offsets {f}")
        same(offs[f].view, g.offs[f], f"{what} string offsets {f}")
        m = g.col_len(f)
        same(outs[f].view[:m], g.cols[f], f"{what} chars {f}")
        # host windows: the offsets and the chars of the records around byte 2^32 of the wire, and the ends
        a = max(0, r - NWIN)
        host_same(offs[f].view, 8 * a, 8 * (a + 2 * NWIN), g.off_window(f, a, a + 2 * NWIN),
                  f"{what} offsets {f} around 2^32")
        host_same(offs[f].view, 8 * (g.n + 1 - 2 * NWIN), 8 * (g.n + 1), g.off_window(f, g.n + 1 - 2 * NWIN, g.n + 1),
                  f"{what} offsets {f} tail")
        c = int(g.off_window(f, r, r + 1)[0])
        lo, hi = max(0, c - WIN), min(m, c + WIN)
        host_same(outs[f].view, lo, hi, g.col_window(f, lo, hi), f"{what} chars {f} around 2^32")
        host_same(outs[f].view, m - 2 * WIN, m, g.col_window(f, m - 2 * WIN, m), f"{what} chars {f} tail")


def _var_need(g, what, extra=0, limit=24 * GIB):
    """The batch, a decode's outputs (a string column has room for W bytes, as the header asks) and `extra`."""
    ns = sum(k == STR for k in g.kinds)
    inputs = g.W + sum(c.numel() * c.element_size() for c in g.cols) + 8 * (g.n + 1) * (ns + 1)
    outputs = sum(g.W if k == STR else g.n * oracle.KIND_SIZE[k] for k in g.kinds) + 8 * (g.n + 1) * (ns + 1)
    need(inputs + outputs + extra + GIB // 2, what, limit)


@pytest.mark.parametrize("vk", [None, 0], ids=["default", "walk"])
@pytest.mark.parametrize("batch", VAR_BATCHES, indirect=True, ids=VAR_IDS)
def test_pack_var(batch, vk):
    g = batch
    p = _var_plan(g, vk)
    sb = p.var_scratch_bytes(g.n, g.W)
    need(2 * g.W + sum(c.numel() * c.element_size() for c in g.cols) + 8 * (g.n + 1) * 4 + sb + GIB // 2, "pack_var")
    out, rec = Guarded(g.W), Guarded(8 * (g.n + 1))
    raw, scratch = _scratch(sb)
    st = status_buf()
    _, ms = timed(lambda: p.pack_var(g.cols, g.offs, g.n, out.view, g.W, rec.view, scratch, sb, st))
    _var_report(f"pack_var {g.straddle} kinds={g.kinds} var_kernel={vk}", p, g, ms)
    assert read_status(st)[0] == 0
    out.check_guards("wire")
    rec.check_guards("rec_offs")
    same(rec.view, g.rec_offs, "rec_offs")
    same(out.view, g.ref, "wire")
    wire_windows(out.view, g, "wire")
    a = g.rec_index - NWIN
    host_same(rec.view, 8 * a, 8 * (a + 2 * NWIN), g.rec_window(a, a + 2 * NWIN), "rec_offs around 2^32")
    host_same(rec.view, 8 * (g.n + 1 - 2 * NWIN), 8 * (g.n + 1), g.rec_window(g.n + 1 - 2 * NWIN, g.n + 1), "rec_offs tail")


@pytest.mark.parametrize("how", ["default", "tiles", "tiled_table"])
@pytest.mark.parametrize("batch", VAR_BATCHES, indirect=True, ids=VAR_IDS)
def test_unpack_var(batch, how):
    """unpack_var as the library runs it, with the record tiles forced, and unpack_var_tiled
    with the tile table var_tile_table makes of the string offsets."""
    g = batch
    p = _var_plan(g, 2 if how == "tiles" else None)
    sb = p.var_scratch_bytes(g.n, g.W)
    _var_need(g, "unpack_var", sb)
    outs, offs = _var_outputs(g)
    raw, scratch = _scratch(sb)
    st = status_buf()
    cols, so = [o.view for o in outs], [None if o is None else o.view for o in offs]
    if how == "tiled_table":
        words = p.var_tile_table_words(g.n)
        table = Guarded(8 * words)
        p.var_tile_table(g.offs, g.n, table.view)
        _, ms = timed(lambda: p.unpack_var_tiled(g.ref, g.W, g.n, g.rec_offs, table.view, cols, so, scratch, sb, st))
        table.check_guards("tile table")
    else:
        _, ms = timed(lambda: p.unpack_var(g.ref, g.W, g.n, g.rec_offs, cols, so, scratch, sb, st))
    _var_report(f"unpack_var {how} {g.straddle} kinds={g.kinds}", p, g, ms)
    assert read_status(st) == GOOD
    _check_var_outputs(g, outs, offs, f"unpack_var {how}")


STREAM_BATCHES = VAR_BATCHES + [(name, "short", "zero_heavy") for name in VAR]
TABLE_MODES = {"tables": 0, "primary": 1, "walk": 2}  # srpc_debug_stream_tables, as tests/test_gpu_stream.py names them


def _table_hook():
    import ctypes
    hook = srpc_amd._lib.lib().srpc_debug_stream_tables
    hook.argtypes, hook.restype = [ctypes.c_int], ctypes.c_int
    return hook


class StreamRun:
    """One batch's stream decodes within 24 GiB.  The call's arguments alone -- the wire, a W-byte
    column per string field, the call's own scratch (5.2 GiB for one string, 7.0 GiB for two at
    this length) -- leave no room for the expected arrays next to them.  So the wire is held once,
    at an odd address (the batch's aligned copy is dropped and made again afterwards), the
    batch's inputs are dropped for each call, and after it the scratch is freed and the inputs are
    made again from the segments to compare.  The outputs are allocated once and refilled."""

    def __init__(self, g, p):
        self.g, self.p = g, p
        self.sb = p.var_stream_scratch_bytes(g.n, g.W)
        ns = sum(k == STR for k in g.kinds)
        inputs = sum(c.numel() * c.element_size() for c in g.cols) + 8 * (g.n + 1) * (ns + 1)
        outputs = sum(g.W if k == STR else g.n * oracle.KIND_SIZE[k] for k in g.kinds) + 8 * (g.n + 1) * (ns + 1)
        need(g.W + outputs + max(self.sb, inputs) + GIB // 2, "unpack_var_stream")
        self.odd = Guarded(g.W, shift=1)
        self.odd.view.copy_(g.ref)
        assert self.odd.view.data_ptr() % 2 == 1
        g.ref = None
        g.drop_inputs()
        torch.cuda.empty_cache()
        self.outs, self.offs = _var_outputs(g)
        self.rec = Guarded(8 * (g.n + 1))

    def call(self, mode, fill, wire_len=None, n=None):
        """One decode on 0xA5 outputs and scratch of `fill` -> (ms, status.reserved); the inputs are back after it."""
        g, p = self.g, self.p
        W, n = (g.W, g.n) if wire_len is None else (wire_len, n)
        for o in self.outs + [o for o in self.offs if o is not None] + [self.rec]:
            o.raw.fill_(0xA5)
        g.drop_inputs()
        torch.cuda.empty_cache()
        sb = p.var_stream_scratch_bytes(n, W)
        assert sb <= self.sb
        raw, scratch = _scratch(sb, fill, 256)
        st = status_buf()
        cols, so = [o.view for o in self.outs], [None if o is None else o.view for o in self.offs]
        hook = _table_hook()
        prev = hook(TABLE_MODES[mode])
        try:
            _, ms = timed(lambda: p.unpack_var_stream(self.odd.view, W, n, self.rec.view, cols, so, scratch, sb, st))
        finally:
            hook(prev)
        del raw, scratch
        torch.cuda.empty_cache()
        g.upload_inputs()
        assert read_status(st) == GOOD, f"tables={mode}, scratch of {fill:#x}"
        return ms, int(st.cpu().numpy()[4:8].view(np.uint32)[0])

    def check(self, what):
        g = self.g
        self.rec.check_guards("rec_offs")
        same(self.rec.view, g.rec_offs, f"{what} rec_offs")
        a = g.rec_index - NWIN
        host_same(self.rec.view, 8 * a, 8 * (a + 2 * NWIN), g.rec_window(a, a + 2 * NWIN), "rec_offs around 2^32")
        _check_var_outputs(g, self.outs, self.offs, what)

    def close(self):
        """The batch as it was: the aligned wire from the odd copy (whose guards and bytes are checked)."""
        self.outs = self.offs = self.rec = None
        torch.cuda.empty_cache()
        self.g.ref = self.odd.view.clone()
        if self.g.cols is None:
            self.g.upload_inputs()
        self.odd.check_guards("the wire")
        wire_windows(self.g.ref, self.g, "the wire after the decode")


@pytest.mark.parametrize("batch", STREAM_BATCHES, indirect=True, ids=["-".join(b) for b in STREAM_BATCHES])
def test_unpack_var_stream(batch):
    """The index-free decode of the same wire at an odd address, with the library's own tables.
    rec_offs are the helper's; a second run on scratch pre-filled with 0xFF gives the same
    outputs.  The same call on the wire cut at the last record boundary under 2^32 is timed."""
    g = batch
    p = _var_plan(g)
    run = StreamRun(g, p)
    try:
        times, reserved = [], []
        for fill in (0xA5, 0xFF):
            ms, res = run.call("tables", fill)
            times.append(ms)
            reserved.append(res)
            run.check(f"unpack_var_stream (scratch of {fill:#x})")
        # the same data cut just under 2^32 (timed; what it decodes is the existing suite's business)
        r = g.rec_index
        cut = int(g.rec_window(r, r + 1)[0])
        assert cut < B
        ms_cut, res = run.call("tables", 0xA5, cut, r)
        reserved.append(res)
        same(run.rec.view[:8 * (r + 1)], g.rec_offs[:r + 1], "rec_offs of the cut wire")
        _var_report(f"unpack_var_stream {g.straddle} kinds={g.kinds}", p, g, times[0],
                    f"second_run_ms={times[1]:.1f} scratch_GiB={run.sb / GIB:.1f} status.reserved="
                    f"{[hex(x) for x in reserved]} cut_under_2^32: W={cut} n={r} call_ms={ms_cut:.1f} "
                    f"ratio={times[0] / ms_cut:.2f}")
    finally:
        run.close()


@pytest.mark.parametrize("mode", ["primary", "walk"])
@pytest.mark.parametrize("batch", [("one_string", "short")], indirect=True, ids=["one_string-short"])
def test_unpack_var_stream_missed_blocks(batch, mode):
    """The decode when its tables miss, forced with the library's test hook: tables that hold
    only each block's first speculated start, and empty tables.  Under 4 GiB the repair pass then
    gives every block the exits of the block before; from 4 GiB on it does nothing (sdx.hip
    k_sx_repair: its offsets are 32-bit) and the second scan walks every block it enters.  So the
    outputs are the helper's as ever, and with empty tables status.reserved says that blocks were
    walked (bit 1, and a count of walking waves in bits 8-31): with a repair pass that ran it
    says neither, as it does under 4 GiB.  The walk is slow (seconds at this length; the time is
    printed, not asserted)."""
    g = batch
    p = _var_plan(g)
    run = StreamRun(g, p)
    try:
        ms, reserved = run.call(mode, 0xA5)
        _var_report(f"unpack_var_stream tables={mode} kinds={g.kinds}", p, g, ms, f"status.reserved={reserved:#x}")
        run.check(f"unpack_var_stream tables={mode}")
        if mode == "walk":
            assert reserved & 2 and reserved >> 8, f"no block was walked: status.reserved = {reserved:#x}"
    finally:
        run.close()
