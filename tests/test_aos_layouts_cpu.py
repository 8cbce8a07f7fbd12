"""The struct layouts of tests/aos_layouts.py are what they claim, proven from
the table alone (no GPU): every one is legal for srpc_gpu_pack_aos, each group
has the property that names it, the expected-image helpers are
self-consistent, the oracle round-trips every layout's columns, and the LDS a
staged launch would ask for is on the stated side of a workgroup's limit."""
import numpy as np
import pytest

import oracle
from tests import aos_layouts as al

ALL = sorted(al.LAYOUTS)


def _sizes(lay):
    return [oracle.KIND_SIZE[k] for k in lay.kinds]


@pytest.mark.parametrize("name", ALL)
def test_layout_is_legal(name):
    """What aos_args asks: fields inside the stride, natural alignment of
    offset, stride and (at `align`) base, no two fields sharing a byte."""
    lay = al.LAYOUTS[name]
    assert 1 <= len(lay.kinds) <= 32 and len(lay.kinds) == len(lay.offsets)
    owner = np.zeros(lay.stride, np.int32)
    for o, sz in zip(lay.offsets, _sizes(lay)):
        assert o + sz <= lay.stride
        assert o % sz == 0 and lay.stride % sz == 0 and lay.align % sz == 0
        owner[o:o + sz] += 1
    assert owner.max() == 1
    assert lay.align == max(_sizes(lay))
    assert lay.envelope in (None, "request", "response")
    # no case moves more than about 2 MiB
    assert max(al.counts(lay)) * lay.stride <= (2 << 20) + lay.stride


def _run_conditions(lay):
    """Which of the run kernels' conditions a layout meets."""
    woff = al.wire_offsets(lay)
    sh = lay.offsets[0] - woff[0]
    one_shift = sh >= 0 and all(o == w + sh for o, w in zip(lay.offsets, woff)) and sh + al.wire_stride(lay) <= lay.stride
    return {"one_shift": one_shift, "no_envelope": lay.envelope is None,
            "body_8_16_24_32": al.wire_stride(lay) in (8, 16, 24, 32),
            "grid8": lay.stride % 8 == 0 and (not one_shift or sh % 8 == 0)}


@pytest.mark.parametrize("shape", al.RUN_SHAPES, ids=lambda s: al.run_name(*s))
def test_runs_are_runs(shape):
    W, boff, stride = shape
    lay = al.RUNS[al.run_name(*shape)]
    assert all(_run_conditions(lay).values())
    assert al.wire_stride(lay) == W and lay.offsets[0] == boff and lay.stride == stride
    assert all(k in (al.I32, al.I64) for k in lay.kinds)
    assert not al.ident(lay) and not al.covered(lay)


def test_run_shapes_are_the_listed_ones():
    assert set(al.RUN_SHAPES) == {(16, 0, 24), (16, 16, 32), (16, 16, 40), (8, 24, 32), (24, 16, 48), (32, 0, 40),
                                  (32, 24, 56), (16, 8, 248), (16, 8, 256), (16, 8, 264), (24, 8, 1024)}
    # 256 is the last stride the fill record and the piece kernel take
    assert al.FILL_MAX == 256 and al.RUNS["run16_at8_s256"].stride == al.FILL_MAX < al.RUNS["run16_at8_s264"].stride


@pytest.mark.parametrize("name", sorted(al.NEAR_RUNS))
def test_near_runs_break_exactly_one_condition(name):
    lay, broken = al.NEAR_RUNS[name]
    cond = _run_conditions(lay)
    assert set(cond) == set(al.RUN_CONDITIONS)
    assert [c for c, ok in cond.items() if not ok] == [broken]


def test_near_run_details():
    perm = al.NEAR_RUNS["quad_permuted"][0]
    assert sorted(perm.offsets) == [8, 12, 16, 20] and perm.offsets != tuple(sorted(perm.offsets))  # contiguous, permuted
    hdr = al.NEAR_RUNS["hdr_quad_s20"][0]
    assert hdr.offsets[0] % 8 and hdr.stride % 8 and hdr.align == 4  # both off the 8-byte grid
    assert al.wire_stride(al.NEAR_RUNS["i32x3_body12"][0]) == 12
    last = al.NEAR_RUNS["quad_last_plus8"][0]
    assert last.offsets == al.QUAD_V[:3] + (al.QUAD_V[3] + 8,)


@pytest.mark.parametrize("name", sorted(al.NEAR_LAYOUTS))
def test_near_layouts_differ_in_exactly_the_named_respect(name):
    lay, (roff, sz, rs), respect = al.NEAR_LAYOUTS[name]
    diff = []
    if tuple(_sizes(lay)) != sz:
        diff.append("SZ")
    if lay.offsets != roff:
        diff.append("ROFF")
    if lay.stride != rs:
        diff.append("RS")
    if lay.envelope is not None:
        diff.append("envelope")
    assert diff == [respect]
    if respect == "ROFF":  # one field moved
        assert sum(a != b for a, b in zip(lay.offsets, roff)) == 1


def test_compile_time_layouts_restated():
    """{bool, int8, char, int16, int32, int64} with C alignment, behind a
    vtable slot and without one."""
    dt = np.dtype({"names": list("abcdef"), "formats": [np.uint8, np.int8, np.int8, np.int16, np.int32, np.int64]},
                  align=True)
    offs = tuple(dt.fields[c][1] for c in "abcdef")
    assert (offs, dt.itemsize) == (al.LAY_ALL_KINDS[0], al.LAY_ALL_KINDS[2])
    assert (tuple(o + 8 for o in offs), dt.itemsize + 8) == (al.LAY_ALL_KINDS_V[0], al.LAY_ALL_KINDS_V[2])


@pytest.mark.parametrize("name", sorted(al.ODD))
def test_odd_layouts_cover_as_stated(name):
    lay = al.ODD[name]
    assert 8 not in _sizes(lay)
    state = "ident" if al.ident(lay) else "covered" if al.covered(lay) else "not_covered"
    assert state == al.ODD_STATE[name]
    if state == "ident":
        assert al.covered(lay)


def test_nested_and_plain_layouts():
    outer = al.NESTED["outer"]
    assert (outer.offsets, outer.stride) == ((8, 24, 26, 32, 33, 36), 40)
    m = al.field_mask(outer)
    assert not m[0:8].any() and not m[16:24].any()  # both vtable slots are unnamed bytes
    two = al.NESTED["two_quads"]
    m = al.field_mask(two)
    assert two.stride == 56 and m[16:32].all() and m[40:56].all() and not m[0:16].any() and not m[32:40].any()
    first = al.NESTED["inner_first"]
    assert first.offsets[0] == 16 and not al.field_mask(first)[0:16].any()  # outer vptr, inner vptr, then a field
    for lay in al.NESTED.values():
        assert not _run_conditions(lay)["one_shift"]
    assert al.ident(al.PLAIN["quad_plain"])


def test_alignment_shifts():
    assert {n: al.shifts(al.LAYOUTS[n]) for n in al.ALIGNED_NAMES} == {
        "i8x3_rot_s3": [1, 2, 4, 8], "i16_i8_s4": [2, 4, 8], "i8_i16_i8_s6": [2, 4, 8], "i16x5_s10": [2, 4, 8],
        "i32_i8_s8": [4, 8], "quad_plain": [4, 8], "outer": [8]}


@pytest.mark.parametrize("name", ALL)
def test_counts(name):
    lay = al.LAYOUTS[name]
    ns = al.counts(lay)
    if lay.stride >= 1024:
        assert ns == [1, 15, 16, 17, 33]
    else:
        T = max(16, (24576 // (al.wire_stride(lay) + len(al.prefix(lay)) + lay.stride)) & ~15)
        assert {1, 15, 16, 17, 255, 256, 257, 1025, T - 1, T, T + 1, 2 * T + 1} <= set(ns)


# ---- the staged kernels' LDS ------------------------------------------------------
def test_wide_and_oversized_are_the_listed_strides():
    assert al.WIDE_STRIDES == (1528, 1536, 1544)
    assert al.OVERSIZED_STRIDES == (4096, 8192, 10_224, 10_232, 16_384, 65_536)
    for s in al.WIDE_STRIDES + al.OVERSIZED_STRIDES:
        g = al.WIDE if s in al.WIDE_STRIDES else al.OVERSIZED
        run, split = g[f"quad_v_s{s}"], g[f"quad_split_s{s}"]
        assert run.stride == split.stride == s
        # Quad behind a vptr is a run at each of these strides (no LDS at all);
        # the split twin is what reaches the staged kernels
        assert all(_run_conditions(run).values())
        assert [c for c, ok in _run_conditions(split).items() if not ok] == ["one_shift"]
    assert al.wire_stride(al.WIDE["i64x32_s264"]) == 256 == al.wire_stride(al.WIDE["i64x32_s272"])
    assert not _run_conditions(al.WIDE["i64x32_s264"])["body_8_16_24_32"]


def test_staged_tile_pins_at_16_records():
    """wire + struct bytes of 1536: the last tile of (24576 // 1536) & ~15 = 16
    records by division; past it the tile is 16 because it cannot be less."""
    assert [al.staged_tile(al.WIDE[f"quad_split_s{s}"]) for s in al.WIDE_STRIDES] == [16, 16, 16]
    assert [24576 // (16 + s) for s in al.WIDE_STRIDES] == [15, 15, 15]
    # ... and the last stride whose tile is 16 by division
    assert 24576 // (16 + 1520) == 16 and 24576 // (16 + 1521) == 15 and al.WIDE["quad_split_s1520"].stride == 1520


@pytest.mark.parametrize("name", ALL)
def test_staged_carve_against_a_workgroups_lds(name):
    """a workgroup of an MI355X may use 163,840 B of LDS.  The
    carve of every layout up to stride 10,224 is within it (10,224 exactly at
    it); 10,232, 16,384 and 65,536 are past it, and only a check in the
    library keeps those launches from being made."""
    lay = al.LAYOUTS[name]
    assert al.LDS_PER_WORKGROUP == 163_840
    carve = al.staged_carve(lay, fill=lay.stride <= al.FILL_MAX and not al.covered(lay))
    if lay.stride <= 10_224:
        assert carve <= al.LDS_PER_WORKGROUP
    else:
        assert lay.stride in (10_232, 16_384, 65_536) and carve > al.LDS_PER_WORKGROUP


def test_staged_carve_values():
    c = {s: al.staged_carve(al.OVERSIZED[f"quad_split_s{s}"]) for s in al.OVERSIZED_STRIDES}
    assert c == {s: 16 * (16 + s) for s in al.OVERSIZED_STRIDES}
    assert c[10_224] == 163_840 and c[10_232] == 163_968
    assert al.staged_carve(al.PLAIN["quad_plain"]) == 24576  # ident: one image
    # an enveloped layout adds template and mask of one period lcm(wire record, 16)
    req = al.NEAR_RUNS["quad_v_request"][0]
    w = 16 + len(al.prefix(req))
    R = (24576 // (w + 24)) & ~15
    assert al.staged_carve(req) == ((R * w + 15) & ~15) + R * 24 + 2 * np.lcm(w, 16)


# ---- the helpers ------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_helpers_self_consistent_and_oracle_round_trip(name):
    lay = al.LAYOUTS[name]
    n = 37
    rng = np.random.default_rng(len(name) + lay.stride)
    src, old = al.records(lay, n, rng), al.records(lay, n, rng)
    assert src.shape == (n, lay.stride) and src.dtype == np.uint8
    for o, k in zip(lay.offsets, lay.kinds):
        if k == al.BOOL:
            assert src[:, o].max() <= 1
    m = al.field_mask(lay)
    assert m.sum() == al.wire_stride(lay) and al.covered(lay) == (m.sum() == lay.stride)
    cols = al.columns(lay, src)
    assert [c.dtype.itemsize for c in cols] == _sizes(lay) and all(len(c) == n for c in cols)
    # unnamed bytes are random too: vtable slots and padding are not zeros
    if lay.stride - m.sum() >= 4:
        assert src[:, ~m].any() and (src[:, ~m] != old[:, ~m]).any()

    inp = al.expect_in_place(lay, old, src)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(al.columns(lay, inp), cols))
    assert np.array_equal(inp[:, ~m], old[:, ~m])
    fill = rng.integers(0, 256, lay.stride, dtype=np.uint8).tobytes()
    for n_fit in (n, n // 2):
        fr = al.expect_fresh(lay, fill, src, n_fit, old)
        assert all(a[:n_fit].tobytes() == b[:n_fit].tobytes() for a, b in zip(al.columns(lay, fr), cols))
        assert np.array_equal(fr[:n_fit, ~m], np.tile(np.frombuffer(fill, np.uint8)[~m], (n_fit, 1)))
        assert np.array_equal(fr[n_fit:], old[n_fit:])
    if al.covered(lay):
        assert np.array_equal(al.expect_fresh(lay, fill, src, n, old), src)
    assert np.array_equal(src, al.expect_in_place(lay, src, src))  # the inputs are left alone

    pre = al.prefix(lay)
    assert bool(pre) == (lay.envelope is not None)
    wire = oracle.pack(list(lay.kinds), cols, n, pre)
    assert len(wire) == n * (len(pre) + al.wire_stride(lay))
    rc, back, _, consumed, _ = oracle.unpack(list(lay.kinds), wire, n, pre)
    assert rc == oracle.ORC_OK and consumed == len(wire)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back, cols))
