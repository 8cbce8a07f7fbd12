"""Struct layouts for the AoS kernels whose shape, not their bytes, is the
point (pure numpy: used by tests/test_gpu_aos_layouts.py, proven to be what
they say by tests/test_aos_layouts_cpu.py).

srpc_amd/csrc/aos.hip picks a kernel family from the caller's layout alone:
field offsets, struct stride, array alignment, envelope, fill record.  A
layout here is (kinds, field_offsets, stride, envelope) in T::fields order
(nested messages flattened), plus `align`, the smallest array alignment it
allows (its largest field).  Bytes of the struct no field names -- vtable
slots, padding, members the schema does not carry -- are random in every
array these helpers make, so a kernel that touches one is seen.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np

import oracle

I8, I16, I32, I64, BOOL, CHAR = oracle.INT8, oracle.INT16, oracle.INT32, oracle.INT64, oracle.BOOL, oracle.CHAR

SCHEMA_NAME = "S"
METHOD = "Svc_servicer::m"
FILL_MAX = 256  # struct bytes srpc_gpu_unpack_aos_fill takes (include/srpc_gpu.h)


class Layout(NamedTuple):
    kinds: Tuple[int, ...]
    offsets: Tuple[int, ...]
    stride: int
    envelope: Optional[str]  # None, "request" or "response"
    align: int


def _lay(kinds, offsets, stride, envelope=None):
    return Layout(tuple(kinds), tuple(offsets), stride, envelope, max(oracle.KIND_SIZE[k] for k in kinds))


def wire_stride(lay):
    """Wire bytes of one record body (the envelope prefix not counted)."""
    return sum(oracle.KIND_SIZE[k] for k in lay.kinds)


def wire_offsets(lay):
    return tuple(int(o) for o in np.cumsum([0] + [oracle.KIND_SIZE[k] for k in lay.kinds])[:-1])


def prefix(lay):
    if lay.envelope == "request":
        return oracle.request_prefix(METHOD, SCHEMA_NAME)
    if lay.envelope == "response":
        return oracle.response_prefix(0, SCHEMA_NAME)
    return b""


def field_mask(lay):
    """True at the struct bytes a leaf field owns."""
    m = np.zeros(lay.stride, bool)
    for o, k in zip(lay.offsets, lay.kinds):
        m[o:o + oracle.KIND_SIZE[k]] = True
    return m


def covered(lay):
    return bool(field_mask(lay).all())


def ident(lay):
    """The struct is the wire body: same offsets, same stride, no envelope."""
    return lay.envelope is None and lay.stride == wire_stride(lay) and lay.offsets == wire_offsets(lay)


# ---- the table ---------------------------------------------------------------
ALL6 = (BOOL, I8, CHAR, I16, I32, I64)
QUAD_V = (8, 12, 16, 20)       # Quad behind a vtable slot: one run of 16 bytes at 8
QUAD_SPLIT = (8, 12, 16, 24)   # ... with a 4-byte member the schema does not name before the last field

NESTED = {
    # gpu_batch_test.cpp's Outer: vptr | id | Inner{vptr | tag . small ....} | flag c .. v
    "outer": _lay((I64, I8, I16, BOOL, CHAR, I32), (8, 24, 26, 32, 33, 36), 40),
    # vptr | Quad{vptr | 4 x int32} | Quad{vptr | 4 x int32}: two runs split by a slot
    "two_quads": _lay((I32,) * 8, (16, 20, 24, 28, 40, 44, 48, 52), 56),
    # vptr | Inner{vptr | tag . small ....} | id | flag ... v: the nested message is the first member
    "inner_first": _lay((I8, I16, I64, BOOL, I32), (16, 18, 24, 32, 36), 40),
}

RUN_BODIES = {8: (I64,), 16: (I32,) * 4, 24: (I64, I32, I32, I64), 32: (I32, I32, I64, I64, I32, I32)}
RUN_SHAPES = [(16, 0, 24), (16, 16, 32), (16, 16, 40), (8, 24, 32), (24, 16, 48), (32, 0, 40), (32, 24, 56),
              (16, 8, 248), (16, 8, 256), (16, 8, 264), (24, 8, 1024)]  # (W, boff, stride)


def run_name(W, boff, stride):
    return f"run{W}_at{boff}_s{stride}"


def _run(W, boff, stride, envelope=None):
    kinds = RUN_BODIES[W]
    return _lay(kinds, [boff + o for o in wire_offsets(_lay(kinds, [0] * len(kinds), W))], stride, envelope)


RUNS = {run_name(*s): _run(*s) for s in RUN_SHAPES}

# what a run kernel needs of a layout (aos.hip launch_aos_run, aos_args); each
# near-run below fails exactly the one named
RUN_CONDITIONS = ("one_shift", "no_envelope", "body_8_16_24_32", "grid8")
NEAR_RUNS = {
    "quad_permuted": (_lay((I32,) * 4, (8, 12, 20, 16), 24), "one_shift"),       # contiguous, not in wire order
    "quad_last_plus8": (_lay((I32,) * 4, (8, 12, 16, 28), 32), "one_shift"),
    "quad_v_request": (_run(16, 8, 24, "request"), "no_envelope"),
    "i32x3_body12": (_lay((I32,) * 3, (8, 12, 16), 24), "body_8_16_24_32"),
    "hdr_quad_s20": (_lay((I32,) * 4, (4, 8, 12, 16), 20), "grid8"),             # {int32 hdr; int32 x 4}
}

# the two compile-time layouts of aos.hip (AosLayAllKindsV / AosLayAllKinds),
# restated: (ROFF, SZ, RS); no envelope
LAY_ALL_KINDS_V = ((8, 9, 10, 12, 16, 24), (1, 1, 1, 2, 4, 8), 32)
LAY_ALL_KINDS = ((0, 1, 2, 4, 8, 16), (1, 1, 1, 2, 4, 8), 24)
# (layout, the compile-time layout it is next to, the one respect it differs in)
NEAR_LAYOUTS = {
    "allv_s40": (_lay(ALL6, (8, 9, 10, 12, 16, 24), 40), LAY_ALL_KINDS_V, "RS"),
    "allv_i16_at14": (_lay(ALL6, (8, 9, 10, 14, 16, 24), 32), LAY_ALL_KINDS_V, "ROFF"),
    "all_s32": (_lay(ALL6, (0, 1, 2, 4, 8, 16), 32), LAY_ALL_KINDS, "RS"),
    "allv_response": (_lay(ALL6, (8, 9, 10, 12, 16, 24), 32, "response"), LAY_ALL_KINDS_V, "envelope"),
}

# no 8-byte field: strides off the 8-byte (and the 4-byte) grid
ODD = {
    "i8x3_rot_s3": _lay((I8, CHAR, BOOL), (2, 0, 1), 3),    # covered, not ident
    "i16_i8_s4": _lay((I16, I8), (0, 2), 4),
    "i8_i16_i8_s6": _lay((I8, I16, I8), (0, 2, 4), 6),      # stride % 4 != 0: the byte-wise fill paths
    "i16x5_s10": _lay((I16,) * 5, (0, 2, 4, 6, 8), 10),     # ident
    "i32_i8_s8": _lay((I32, I8), (0, 4), 8),
}
ODD_STATE = {"i8x3_rot_s3": "covered", "i16_i8_s4": "not_covered", "i8_i16_i8_s6": "not_covered",
             "i16x5_s10": "ident", "i32_i8_s8": "not_covered"}

PLAIN = {"quad_plain": _lay((I32,) * 4, (0, 4, 8, 12), 16)}  # Quad without a vptr: ident

WIDE_STRIDES = (1528, 1536, 1544)                            # the staged tile: 16 records, then pinned at 16
OVERSIZED_STRIDES = (4096, 8192, 10_224, 10_232, 16_384, 65_536)
WIDE = {
    "i64x32_s264": _lay((I64,) * 32, range(8, 264, 8), 264),  # wire 256 B behind a vptr
    "i64x32_s272": _lay((I64,) * 32, range(8, 264, 8), 272),  # ... and 8 unnamed bytes after the fields
}
# Quad behind a vptr is a run layout at every stride that is a multiple of 8
# (the run kernels: no LDS).  Its twin with an unnamed member before the last
# field is not, and takes the staged kernels -- the ones whose LDS grows with
# the stride.
for _s in WIDE_STRIDES:
    WIDE[f"quad_v_s{_s}"] = _lay((I32,) * 4, QUAD_V, _s)
    WIDE[f"quad_split_s{_s}"] = _lay((I32,) * 4, QUAD_SPLIT, _s)
# (wire + struct bytes reach 1536 at stride 1520: the last tile of 16 records by division)
WIDE["quad_split_s1520"] = _lay((I32,) * 4, QUAD_SPLIT, 1520)
OVERSIZED = {}
for _s in OVERSIZED_STRIDES:
    OVERSIZED[f"quad_v_s{_s}"] = _lay((I32,) * 4, QUAD_V, _s)
    OVERSIZED[f"quad_split_s{_s}"] = _lay((I32,) * 4, QUAD_SPLIT, _s)

GROUPS = {
    "nested": NESTED, "runs": RUNS, "near_runs": {k: v[0] for k, v in NEAR_RUNS.items()},
    "near_layouts": {k: v[0] for k, v in NEAR_LAYOUTS.items()}, "odd": ODD, "plain": PLAIN, "wide": WIDE,
    "oversized": OVERSIZED,
}
LAYOUTS = {name: lay for g in GROUPS.values() for name, lay in g.items()}
assert sum(len(g) for g in GROUPS.values()) == len(LAYOUTS), "layout names are unique"

# the array's shift inside a 16-byte-aligned allocation: every one the
# layout's largest field permits
ALIGNED_NAMES = list(ODD) + ["quad_plain", "outer"]


def shifts(lay):
    return [s for s in (1, 2, 4, 8) if s % lay.align == 0]


# ---- record counts -----------------------------------------------------------
# The staged kernels' tile, restated from aos.hip (kAosTileBytes = 24 KiB over
# wire + struct bytes, a multiple of 16, at least 16).  If the constant moves
# the fixed list below still stands.  (A struct that is its wire body keeps one
# LDS image: the tile of wire bytes alone is in the list too.)
STAGED_TILE_BYTES = 24576
N_SMALL = (1, 15, 16, 17, 255, 256, 257, 1025)
N_LARGE = (1, 15, 16, 17, 33)  # strides of 1024 and up


def staged_tile(lay):
    return max(16, (STAGED_TILE_BYTES // (wire_stride(lay) + len(prefix(lay)) + lay.stride)) & ~15)


def counts(lay):
    if lay.stride >= 1024:
        return list(N_LARGE)
    ts = [staged_tile(lay)]
    if ident(lay):
        ts.append(max(16, (STAGED_TILE_BYTES // wire_stride(lay)) & ~15))
    ns = set(N_SMALL)
    for t in ts:
        ns.update((t - 1, t, t + 1, 2 * t + 1))
    return sorted(ns)


# ---- the LDS a staged launch asks for ------------------------------------------
LDS_PER_WORKGROUP = 163_840  # the bytes a workgroup of an MI355X may use


def staged_carve(lay, fill=False):
    """Dynamic LDS bytes of the staged kernels for this layout, restated from
    aos.hip staged_tiling: wire image | struct image (unless ident) |
    envelope template and mask | fill record."""
    w = wire_stride(lay) + len(prefix(lay))
    per = w if ident(lay) else w + lay.stride
    R = max(16, (STAGED_TILE_BYTES // per) & ~15)
    r16 = lambda b: (b + 15) & ~15  # noqa: E731
    end = r16(R * w) + (0 if ident(lay) else r16(R * lay.stride))
    L = w // np.gcd(w, 16) * 16
    return int(end + (2 * L if lay.envelope else 0) + (FILL_MAX if fill else 0))


# ---- data ------------------------------------------------------------------------
def records(lay, n, rng):
    """(n, stride) uint8: random bytes everywhere, BOOL fields 0 / 1."""
    recs = rng.integers(0, 256, (n, lay.stride), dtype=np.uint8)
    for o, k in zip(lay.offsets, lay.kinds):
        if k == BOOL:
            recs[:, o] &= 1
    return recs


def columns(lay, recs):
    """The field columns of a struct array, as oracle.pack takes them."""
    cols = []
    for o, k in zip(lay.offsets, lay.kinds):
        sz = oracle.KIND_SIZE[k]
        cols.append(np.ascontiguousarray(recs[:, o:o + sz]).reshape(-1).view(oracle.KIND_DTYPE[k]).copy())
    return cols


def expect_in_place(lay, old, src):
    """The whole array after an in-place unpack of src's fields: `old` with
    only the leaf bytes taken from `src`."""
    out = old.copy()
    m = field_mask(lay)
    out[:, m] = src[:, m]
    return out


def expect_fresh(lay, fill, src, n_fit, old):
    """The whole array after an unpack into fresh objects: the fill record
    with src's leaf bytes for records < n_fit, `old` beyond (a short wire)."""
    out = old.copy()
    m = field_mask(lay)
    out[:n_fit] = np.frombuffer(bytes(fill), np.uint8)
    out[:n_fit, m] = src[:n_fit, m]
    return out
