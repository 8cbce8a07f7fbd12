"""Kernel-clock time of the mixed batches whose plans are held, plan by plan, in
columns or in struct arrays (srpc_frames_pack_requests_mixed_legs,
srpc_frames_unpack_replies_mixed_legs) beside the existing calls on the same
input.

Data: the Calculator set (K = 4), `--calls` calls in uniformly random order, the
natural layouts (TwoNumbers and Number behind a vtable slot: 16-byte structs),
all replies full; and Calculator + echo (multiple_primitives both ways, K = 5),
`--text-calls` calls in uniformly random order, strings of 0..`--maxlen` bytes:
the call mix of tools/mixed_var_bench.py.

  rows, each for the pack and for the decode
    (a) _mixed_legs, every plan in columns        (b) _mixed_var, the same input
    (c) _mixed_legs, every fixed plan in records  (d) _mixed_aos, the same input
    (m) _mixed, the same frames (the column call (d) is measured against)
    (e) _mixed_legs over Calculator + echo: add and multiply in records, square
        and subtract in columns, the string leg present

Yardsticks, fixed before anything was measured, on medians:
  1. kind-awareness costs the column case nothing it can avoid: (a) <= 1.05 * (b);
  2. struct arrays cost the new decode no more than they cost the existing
     pair: (c)/(a) <= 1.10 * (d)/(m).
Every figure is srpc_time_next_call's interval, all rows interleaved in each of
`--reps` rounds after one warm-up round; medians, extremes and every sample are
printed.  Rows of one group read the same frames, and the 256 MB Infinity Cache
keeps them from one row to the next: the first row of a group would pay for the
cold stream and the rows behind it would not.  So every row starts cold: a
1 GiB buffer is rewritten before each one (`--warm` leaves that out).

    python tools/mixed_legs_bench.py [--calls 4000000] [--text-calls 1000000] [--maxlen 64] [--reps 10]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from srpc_amd import (NUMBER, RPC_ERR_RECV_TIMEOUT, TWO_NUMBERS, GpuPacker, MixedAosFrames, MixedFrames,  # noqa: E402
                      MixedLegFrames, MixedVarFrames, Schema, framed_request_prefix, framed_response_prefix,
                      time_next_call)

DEV = torch.device("cuda:0")
PEAK = 8e12  # bytes/s, MI355X HBM3E
SVC = "Calculator_servicer::"
MP = Schema.of("multiple_primitives", ("arg1", "int8"), ("arg2", "char"), ("arg3", "int64"), ("arg4", "string"))
CALC = [("square", NUMBER), ("add", TWO_NUMBERS), ("subtract", TWO_NUMBERS), ("multiply", TWO_NUMBERS)]
STRIDE = 16                       # sizeof(TwoNumbers) == sizeof(Number): a vtable slot, then the int32s
OFFS = {1: [8], 2: [8, 12]}       # leaf offsets by the number of leaves


def zeros(nbytes):
    return torch.zeros(int(nbytes) + 16, dtype=torch.uint8, device=DEV)


def structs(cols, count, gen):
    """count 16-byte structs with random bytes around the int32 leaves of `cols`."""
    a = torch.randint(0, 256, (count * STRIDE + 16,), dtype=torch.uint8, device=DEV, generator=gen)
    w = a[:count * STRIDE].view(torch.int32).view(count, STRIDE // 4)
    for f, c in enumerate(cols):
        w[:, 2 + f] = c[:count]
    return a


def u64_at(t, i=0):
    return int(t[8 * i:8 * i + 8].cpu().numpy().view(np.uint64)[0])


def mp_leg(count, maxlen, gen):
    """multiple_primitives columns: (cols, str_offs, chars)."""
    lens = torch.randint(0, maxlen + 1, (count,), dtype=torch.int64, device=DEV, generator=gen)
    offs = torch.zeros(count + 1, dtype=torch.int64, device=DEV)
    offs[1:] = torch.cumsum(lens, 0)
    chars = int(offs[count].item())
    cols = [torch.randint(0, 127, (count + 16,), dtype=torch.int8, device=DEV, generator=gen),
            torch.randint(0, 127, (count + 16,), dtype=torch.int8, device=DEV, generator=gen),
            torch.randint(-2**62, 2**62, (count + 2,), dtype=torch.int64, device=DEV, generator=gen),
            torch.randint(0, 256, (chars + 16,), dtype=torch.uint8, device=DEV, generator=gen)]
    return cols, [None, None, None, offs], chars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4_000_000)
    ap.add_argument("--text-calls", type=int, default=1_000_000)
    ap.add_argument("--maxlen", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", action="store_true", help="do not evict the caches before each row")
    a = ap.parse_args()
    evict = None if a.warm else torch.zeros(1 << 30, dtype=torch.uint8, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda c: torch.randint(-2**31, 2**31 - 1, (c + 4,), dtype=torch.int32, device=DEV, generator=gen)  # noqa: E731
    st = zeros(16)

    # ---- Calculator, K = 4 ----
    n, K = a.calls, len(CALC)
    method = torch.randint(0, K, (n,), dtype=torch.uint8, device=DEV, generator=gen)
    count = torch.bincount(method.to(torch.int64), minlength=K).tolist()
    rq_plans = [GpuPacker(s, framed_request_prefix(s, SVC + m)) for m, s in CALC]
    rs_plans = [GpuPacker(NUMBER, framed_response_prefix(NUMBER, 0)) for _ in CALC]
    Fq, Fr = [p.record_bytes for p in rq_plans], [p.record_bytes for p in rs_plans]
    q_cols = [[rnd(count[k]) for _ in s.kinds] for k, (_, s) in enumerate(CALC)]
    s_cols = [[rnd(count[k])] for k in range(K)]                      # the replies' values
    q_recs = [structs(q_cols[k], count[k], gen) for k in range(K)]
    q_offs = [OFFS[len(s.kinds)] for _, s in CALC]
    none = [None] * K
    q_legs_c, s_legs_c = MixedLegFrames(rq_plans, [0] * K, none), MixedLegFrames(rs_plans, [0] * K, none)
    q_legs_r, s_legs_r = MixedLegFrames(rq_plans, [STRIDE] * K, q_offs), MixedLegFrames(rs_plans, [STRIDE] * K, [OFFS[1]] * K)
    q_var, s_var = MixedVarFrames(rq_plans), MixedVarFrames(rs_plans)
    q_aos, s_aos = MixedAosFrames(rq_plans, [STRIDE] * K, q_offs), MixedAosFrames(rs_plans, [STRIDE] * K, [OFFS[1]] * K)
    q_col, s_col = MixedFrames(rq_plans), MixedFrames(rs_plans)
    nb = MixedFrames.index_bytes(n, K)
    index, counts = zeros(nb), zeros(8 * (K + 1))
    assert MixedFrames.index(method, n, K, index, nb, counts, st) == 0
    q_total = sum(c * f for c, f in zip(count, Fq))
    out_cap = n * max(Fq)
    outs = {r: zeros(out_cap) for r in "abcdm"}
    offs = {r: zeros(4 * (n + 1)) for r in "abcdm"}
    totals = {r: zeros(8) for r in "abc"}
    sb = max(m.scratch_bytes(n) for m in (q_legs_c, s_legs_c, q_legs_r, s_legs_r, q_var, s_var))
    scratch = zeros(sb)
    sb_aos = s_aos.scratch_bytes
    scratch_aos = zeros(sb_aos)
    # the reply stream: every call's full reply in call order, packed by the column call with the reply plans
    buf, roffs = zeros(n * max(Fr)), zeros(4 * (n + 1))
    assert s_col.pack(s_cols, None, count, method, index, n, buf, n * max(Fr), roffs, st) == 0
    torch.cuda.synchronize()
    buf_len = int(roffs[:4 * (n + 1)].view(torch.int32)[n].item())
    d_recs = {r: [zeros(count[k] * STRIDE) for k in range(K)] for r in "cd"}
    d_cols = {r: [[zeros(4 * count[k])] for k in range(K)] for r in "abm"}
    codes = {r: zeros(n) for r in "abcdm"}
    ends = zeros(64)
    fills = [np.random.default_rng(k).integers(0, 256, STRIDE, dtype=np.uint8).tobytes() for k in range(K)]
    T = RPC_ERR_RECV_TIMEOUT

    # ---- Calculator + echo, K = 5 ----
    n5, K5 = a.text_calls, K + 1
    method5 = torch.randint(0, K5, (n5,), dtype=torch.uint8, device=DEV, generator=gen)
    count5 = torch.bincount(method5.to(torch.int64), minlength=K5).tolist()
    rq5 = rq_plans + [GpuPacker.for_request(MP, "Echo_servicer::echo")]
    rs5 = rs_plans + [GpuPacker.for_response(MP, 0)]
    q5_cols = [[rnd(count5[k]) for _ in s.kinds] for k, (_, s) in enumerate(CALC)]
    s5_cols = [[rnd(count5[k])] for k in range(K)]
    q_echo, s_echo = mp_leg(count5[4], a.maxlen, gen), mp_leg(count5[4], a.maxlen, gen)
    rec5 = [False, True, False, True, False]  # add and multiply in records
    strides5 = [STRIDE if r else 0 for r in rec5]
    q5 = MixedLegFrames(rq5, strides5, [q_offs[k] if rec5[k] else None for k in range(K)] + [None])
    s5 = MixedLegFrames(rs5, strides5, [OFFS[1] if rec5[k] else None for k in range(K)] + [None])
    s5_all_cols = MixedVarFrames(rs5)
    e_cols = [None if rec5[k] else q5_cols[k] for k in range(K)] + [q_echo[0]]
    e_so = [None] * K + [q_echo[1]]
    e_recs = [structs(q5_cols[k], count5[k], gen) if rec5[k] else None for k in range(K)] + [None]
    nb5 = MixedFrames.index_bytes(n5, K5)
    index5, counts5 = zeros(nb5), zeros(8 * (K5 + 1))
    assert MixedFrames.index(method5, n5, K5, index5, nb5, counts5, st) == 0
    fixed_q = 4 + len(rq5[4].prefix) + 1 + 1 + 8 + 8
    fixed_r = 4 + len(rs5[4].prefix) + 1 + 1 + 8 + 8
    q5_total = sum(c * f for c, f in zip(count5, Fq)) + count5[4] * fixed_q + q_echo[2]
    r5_total = sum(c * f for c, f in zip(count5, Fr)) + count5[4] * fixed_r + s_echo[2]
    out5, offs5, total5 = zeros(q5_total), zeros(4 * (n5 + 1)), zeros(8)
    sb5 = max(q5.scratch_bytes(n5), s5.scratch_bytes(n5), s5_all_cols.scratch_bytes(n5))
    scratch5 = zeros(sb5)
    # the reply stream of that set, packed from columns by the existing string-aware call
    buf5, roffs5 = zeros(r5_total), zeros(4 * (n5 + 1))
    assert s5_all_cols.pack(s5_cols + [s_echo[0]], [None] * K + [s_echo[1]], None, count5, method5, index5, n5, buf5,
                            r5_total, roffs5, total5, st, scratch5, sb5) == 0
    torch.cuda.synchronize()
    assert u64_at(total5) == r5_total
    o_cols = [None if rec5[k] else [zeros(4 * count5[k])] for k in range(K)] + [[zeros(c.numel() * c.element_size()) for c in s_echo[0]]]
    o_so = [None] * K + [[None, None, None, zeros(8 * (count5[4] + 1))]]
    o_cap = [None] * K + [[None, None, None, s_echo[2]]]
    o_recs = [zeros(count5[k] * STRIDE) if rec5[k] else None for k in range(K)] + [None]
    fills5 = [fills[k] if rec5[k] else None for k in range(K)] + [None]
    codes5, ends5 = zeros(n5), zeros(64)

    calls = {
        "a  pack   legs, columns": lambda: q_legs_c.pack(q_cols, none, none, None, count, method, index, n, outs["a"], out_cap,
                                                         offs["a"], totals["a"], st, scratch, sb),
        "b  pack   mixed_var": lambda: q_var.pack(q_cols, none, None, count, method, index, n, outs["b"], out_cap, offs["b"],
                                                  totals["b"], st, scratch, sb),
        "c  pack   legs, records": lambda: q_legs_r.pack(none, none, q_recs, None, count, method, index, n, outs["c"], out_cap,
                                                         offs["c"], totals["c"], st, scratch, sb),
        "d  pack   mixed_aos": lambda: q_aos.pack(q_recs, None, count, method, index, n, outs["d"], out_cap, offs["d"], st),
        "m  pack   mixed": lambda: q_col.pack(q_cols, None, count, method, index, n, outs["m"], out_cap, offs["m"], st),
        "e  pack   legs, half records + echo": lambda: q5.pack(e_cols, e_so, e_recs, None, count5, method5, index5, n5, out5,
                                                               q5_total, offs5, total5, st, scratch5, sb5),
        "a' decode legs, columns": lambda: s_legs_c.unpack(buf, buf_len, roffs, n, method, index, n, T, d_cols["a"], none, none,
                                                           none, none, None, count, codes["a"], ends, st, scratch, sb),
        "b' decode mixed_var": lambda: s_var.unpack(buf, buf_len, roffs, n, method, index, n, T, d_cols["b"], none, none, None,
                                                    count, codes["b"], ends, st, scratch, sb),
        "c' decode legs, records": lambda: s_legs_r.unpack(buf, buf_len, roffs, n, method, index, n, T, none, none, none,
                                                           d_recs["c"], fills, None, count, codes["c"], ends, st, scratch, sb),
        "d' decode mixed_aos": lambda: s_aos.unpack(buf, buf_len, roffs, n, method, index, n, T, d_recs["d"], fills, None, count,
                                                    codes["d"], scratch_aos, sb_aos, st),
        "m' decode mixed": lambda: s_col.unpack(buf, buf_len, roffs, n, method, index, n, T, d_cols["m"], None, count,
                                                codes["m"], st),
        "e' decode legs, half records + echo": lambda: s5.unpack(buf5, r5_total, roffs5, n5, method5, index5, n5, T, o_cols,
                                                                 o_so, o_cap, o_recs, fills5, None, count5, codes5, ends5, st,
                                                                 scratch5, sb5),
    }
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s), e1.record(s)
    torch.cuda.synchronize()
    samples = {k: [] for k in calls}
    for r in range(a.reps + 1):
        for k, fn in calls.items():
            st.zero_()
            if evict is not None:
                evict.add_(1)  # four times the Infinity Cache: the row's inputs and outputs start in HBM
            time_next_call(e0, e1)
            rc = fn()
            torch.cuda.synchronize()
            assert rc == 0 and not st[:4].any(), (k, rc)
            if r:
                samples[k].append(e0.elapsed_time(e1) * 1e3)  # us

    # every form of each group computed the same
    for r in "abcd":
        assert torch.equal(outs[r][:q_total], outs["m"][:q_total]), r
        assert torch.equal(offs[r][:4 * (n + 1)], offs["m"][:4 * (n + 1)]), r
    assert all(u64_at(totals[r]) == q_total for r in "abc") and u64_at(total5) == q5_total
    for r in "abcdm":
        assert not codes[r][:n].any(), r
    for k in range(K):
        want = s_cols[k][0][:count[k]]
        for r in "abm":
            assert torch.equal(d_cols[r][k][0][:4 * count[k]].view(torch.int32), want), (r, k)
        fill = torch.frombuffer(bytearray(fills[k]), dtype=torch.uint8).to(DEV)
        for r in "cd":
            got = d_recs[r][k][:count[k] * STRIDE].view(count[k], STRIDE)
            assert torch.equal(got.view(torch.int32).view(count[k], 4)[:, 2], want), (r, k)
            assert torch.equal(got[:, :8], fill[:8].expand(count[k], 8)) and torch.equal(got[:, 12:], fill[12:].expand(count[k], 4))
    assert not codes5[:n5].any() and u64_at(ends5) == s_echo[2]
    for k in range(K):
        want = s5_cols[k][0][:count5[k]]
        if rec5[k]:
            assert torch.equal(o_recs[k][:count5[k] * STRIDE].view(torch.int32).view(count5[k], 4)[:, 2], want), k
        else:
            assert torch.equal(o_cols[k][0][:4 * count5[k]].view(torch.int32), want), k
    assert torch.equal(o_cols[4][3][:s_echo[2]], s_echo[0][3][:s_echo[2]])
    assert torch.equal(o_so[4][3][:8 * (count5[4] + 1)].view(torch.int64), s_echo[1][3])
    assert torch.equal(o_cols[4][2][:8 * count5[4]].view(torch.int64), s_echo[0][2][:count5[4]])

    print(f"calculator: calls {n} K {K} counts {count} request frames {Fq} reply frames {Fr} struct bytes {STRIDE} "
          f"tiles: legs columns {s_legs_c.tile} legs records {s_legs_r.tile} mixed_var {s_var.tile} mixed_aos {s_aos.tile}")
    print(f"calculator + echo: calls {n5} K {K5} counts {count5} maxlen {a.maxlen} request bytes {q5_total} reply bytes "
          f"{r5_total} tile {s5.tile}   reps {a.reps}   caches {'as the row before left them' if a.warm else 'evicted before every row'}")
    med = {}
    for k, v in samples.items():
        med[k[:2].strip()] = statistics.median(v)
        print(f"{k:38s} median {statistics.median(v):9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  samples "
              + " ".join(f"{x:.1f}" for x in v))
    for what, q in (("pack", ""), ("decode", "'")):
        A, B, C, D, M = (med[r + q] for r in "abcdm")
        ok1 = A <= 1.05 * B
        print(f"{what}: yardstick 1  (a)/(b) = {A / B:.3f}  bar 1.05: {'within' if ok1 else 'MISSED'}")
        ok2 = C / A <= 1.10 * D / M
        print(f"{what}: yardstick 2  (c)/(a) = {C / A:.3f}  (d)/(m) = {D / M:.3f}  bar 1.10 * {D / M:.3f} = {1.10 * D / M:.3f}: "
              f"{'within' if ok2 else 'MISSED'}{'' if q else '  (the yardstick names the decode; the pack is shown beside it)'}")
    alg = {"a": q_total + n * (4 + 1) + 4 * sum(c * len(s.kinds) for c, (_, s) in zip(count, CALC)),
           "c": q_total + n * (4 + 1) + 4 * sum(c * len(s.kinds) for c, (_, s) in zip(count, CALC)),
           "a'": buf_len + n * (4 + 1 + 1 + 4), "c'": buf_len + n * (4 + 1 + 1 + STRIDE)}
    for r, b in alg.items():
        print(f"({r}) algorithmic bytes {b} -> {b / (med[r] * 1e-6) / 1e12:.2f} TB/s = {b / (med[r] * 1e-6) / PEAK:.3f} of 8 TB/s")


if __name__ == "__main__":
    main()
