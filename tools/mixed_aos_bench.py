"""Kernel-clock time of the struct-array legs of the mixed batches
(srpc_frames_pack_requests_mixed_aos, srpc_frames_unpack_replies_mixed_aos)
beside the calls that bracket them: the Calculator set, K = 4,
`--calls` calls in uniformly random order, the natural layouts (TwoNumbers and
Number behind a vtable slot: 16-byte structs), all replies full.

  pack    (a)  _pack_requests_mixed_aos      (b)  _pack_requests_mixed, same values
          (c)  srpc_gpu_pack_aos             (d)  srpc_gpu_pack: the framed `square`
                                                  request plan, the same struct
  decode  (a') _unpack_replies_mixed_aos     (b') _unpack_replies_mixed
          (c') srpc_frames_unpack_replies_aos (d') srpc_frames_unpack_replies:
                                                  indexed, Number replies, the same struct

(c)/(d) and (c')/(d') are what struct arrays cost the single-plan calls on this
box; the yardstick, fixed before measuring: (a)/(b) <= 1.1 * (c)/(d), and
likewise for the decode.  Every figure is srpc_time_next_call's interval, all
eight calls interleaved in each of `--reps` rounds after one warm-up round;
medians, extremes and every sample are printed.

    python tools/mixed_aos_bench.py [--calls 4000000] [--reps 10]
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
                      framed_request_prefix, framed_response_prefix, time_next_call)

DEV = torch.device("cuda:0")
PEAK = 8e12  # bytes/s, MI355X HBM3E
SVC = "Calculator_servicer::"
METHODS = [("square", NUMBER), ("add", TWO_NUMBERS), ("subtract", TWO_NUMBERS), ("multiply", TWO_NUMBERS)]
STRIDE = 16                       # sizeof(TwoNumbers) == sizeof(Number): a vtable slot, then the int32s
OFFS = {1: [8], 2: [8, 12]}       # leaf offsets by the number of leaves


def zeros(nbytes):
    return torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)


def structs(cols, count, gen):
    """count 16-byte structs with random bytes around the int32 leaves of `cols`."""
    a = torch.randint(0, 256, (count * STRIDE + 16,), dtype=torch.uint8, device=DEV, generator=gen)
    w = a[:count * STRIDE].view(torch.int32).view(count, STRIDE // 4)
    for f, c in enumerate(cols):
        w[:, 2 + f] = c[:count]
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    n, K = a.calls, len(METHODS)
    gen = torch.Generator(device=DEV).manual_seed(1)
    method = torch.randint(0, K, (n,), dtype=torch.uint8, device=DEV, generator=gen)
    count = torch.bincount(method.to(torch.int64), minlength=K).tolist()
    rq_plans = [GpuPacker(s, framed_request_prefix(s, SVC + m)) for m, s in METHODS]
    rs_plans = [GpuPacker(NUMBER, framed_response_prefix(NUMBER, 0)) for _ in METHODS]
    Fq, Fr = [p.record_bytes for p in rq_plans], [p.record_bytes for p in rs_plans]
    rnd = lambda c: torch.randint(-2**31, 2**31 - 1, (c + 4,), dtype=torch.int32, device=DEV, generator=gen)
    q_cols = [[rnd(count[k]) for _ in s.kinds] for k, (_, s) in enumerate(METHODS)]
    s_cols = [[rnd(count[k])] for k in range(K)]                      # the replies' values
    q_recs = [structs(q_cols[k], count[k], gen) for k in range(K)]
    s_recs = [structs(s_cols[k], count[k], gen) for k in range(K)]
    q_aos = MixedAosFrames(rq_plans, [STRIDE] * K, [OFFS[len(s.kinds)] for _, s in METHODS])
    s_aos = MixedAosFrames(rs_plans, [STRIDE] * K, [OFFS[1]] * K)
    q_col, s_col = MixedFrames(rq_plans), MixedFrames(rs_plans)
    nb = MixedFrames.index_bytes(n, K)
    index, counts, st = zeros(nb), zeros(8 * (K + 1)), zeros(16)
    assert MixedFrames.index(method, n, K, index, nb, counts, st) == 0
    out_cap = n * max(Fq)
    out_a, out_b, offs_a, offs_b = zeros(out_cap), zeros(out_cap), zeros(4 * (n + 1)), zeros(4 * (n + 1))
    # the reply stream: every call's full reply in call order, packed by the column call with the reply plans
    buf, roffs = zeros(n * max(Fr)), zeros(4 * (n + 1))
    assert s_col.pack(s_cols, None, count, method, index, n, buf, n * max(Fr), roffs, st) == 0
    torch.cuda.synchronize()
    buf_len = int(roffs[:4 * (n + 1)].view(torch.int32)[n].item())
    d_recs = [zeros(count[k] * STRIDE) for k in range(K)]
    d_cols = [[zeros(4 * count[k])] for k in range(K)]
    codes_a, codes_b = zeros(n), zeros(n)
    fills = [np.random.default_rng(k).integers(0, 256, STRIDE, dtype=np.uint8).tobytes() for k in range(K)]
    sb = s_aos.scratch_bytes
    scratch = zeros(sb)
    # the single-plan rows: n `square` requests / Number replies from and into the same struct
    one_q, one_s = rq_plans[0], rs_plans[0]
    one_col = [rnd(n)]
    one_recs = structs(one_col, n, gen)
    wire_c, wire_d = zeros(n * Fq[0]), zeros(n * Fq[0])
    rbuf = zeros(n * Fr[0])
    one_s.pack(one_col, n, rbuf)
    uoffs = (torch.arange(n, dtype=torch.int64, device=DEV) * Fr[0]).to(torch.int32)
    one_out, one_cols, one_codes = zeros(n * STRIDE), [zeros(4 * n)], zeros(n)
    calls = {
        "a  pack_requests_mixed_aos": lambda: q_aos.pack(q_recs, None, count, method, index, n, out_a, out_cap, offs_a, st),
        "b  pack_requests_mixed": lambda: q_col.pack(q_cols, None, count, method, index, n, out_b, out_cap, offs_b, st),
        "c  pack_aos": lambda: one_q.pack_aos(one_recs, STRIDE, OFFS[1], n, wire_c) * 0,
        "d  pack": lambda: one_q.pack(one_col, n, wire_d) * 0,
        "a' unpack_replies_mixed_aos": lambda: s_aos.unpack(buf, buf_len, roffs, n, method, index, n, RPC_ERR_RECV_TIMEOUT,
                                                            d_recs, fills, None, count, codes_a, scratch, sb, st),
        "b' unpack_replies_mixed": lambda: s_col.unpack(buf, buf_len, roffs, n, method, index, n, RPC_ERR_RECV_TIMEOUT,
                                                        d_cols, None, count, codes_b, st),
        "c' unpack_replies_aos": lambda: one_s.unpack_replies_aos(rbuf, n * Fr[0], uoffs, n, one_out, STRIDE, OFFS[1],
                                                                  fills[0], one_codes, st),
        "d' unpack_replies": lambda: one_s.unpack_replies(rbuf, n * Fr[0], uoffs, n, one_cols, one_codes, st),
    }
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s), e1.record(s)
    torch.cuda.synchronize()
    samples = {k: [] for k in calls}
    for r in range(a.reps + 1):
        for k, fn in calls.items():
            st.zero_()
            time_next_call(e0, e1)
            rc = fn()
            torch.cuda.synchronize()
            assert rc == 0 and not st[:4].any(), (k, rc)
            if r:
                samples[k].append(e0.elapsed_time(e1) * 1e3)  # us
    # both forms of each pair computed the same
    total = int(offs_a[:4 * (n + 1)].view(torch.int32)[n].item())
    assert total == sum(c * f for c, f in zip(count, Fq)) and torch.equal(out_a[:total], out_b[:total])
    assert torch.equal(offs_a[:4 * (n + 1)], offs_b[:4 * (n + 1)]) and torch.equal(wire_c[:n * Fq[0]], wire_d[:n * Fq[0]])
    assert not codes_a[:n].any() and not codes_b[:n].any() and not one_codes[:n].any()
    for k in range(K):
        leaves = d_recs[k][:count[k] * STRIDE].view(torch.int32).view(count[k], 4)[:, 2]
        assert torch.equal(leaves, s_cols[k][0][:count[k]])
        assert torch.equal(leaves, d_cols[k][0][:4 * count[k]].view(torch.int32))
        want = torch.frombuffer(bytearray(fills[k]), dtype=torch.uint8).to(DEV)
        got = d_recs[k][:count[k] * STRIDE].view(count[k], STRIDE)
        assert torch.equal(got[:, :8], want[:8].expand(count[k], 8)) and torch.equal(got[:, 12:], want[12:].expand(count[k], 4))
    assert torch.equal(one_out[:n * STRIDE].view(torch.int32).view(n, 4)[:, 2], one_col[0][:n])
    print(f"calls {n} K {K} counts {count} request frames {Fq} reply frames {Fr} struct bytes {STRIDE} reps {a.reps} "
          f"tiles: pack {q_col.tile} decode {s_aos.tile} scratch {sb} B")
    med = {}
    for k, v in samples.items():
        med[k] = statistics.median(v)
        print(f"{k:30s} median {med[k]:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  samples "
              + " ".join(f"{x:.1f}" for x in v))
    ma, mb, mc, md, na, nb_, nc, nd = (med[k] for k in calls)
    for what, x, y, z, w in (("pack", ma, mb, mc, md), ("decode", na, nb_, nc, nd)):
        print(f"{what}: mixed aos/columns = {x / y:.3f}   single-plan aos/columns = {z / w:.3f}   yardstick 1.1 * "
              f"{z / w:.3f} = {1.1 * z / w:.3f}   the mixed AoS call {'is within' if x / y <= 1.1 * z / w else 'MISSES'} it")
    alg_p = total + n * (STRIDE + 1)
    alg_d = buf_len + n * (STRIDE + 1 + 1 + 4)
    print(f"(a)  algorithmic bytes {alg_p} -> {alg_p / (ma * 1e-6) / 1e12:.2f} TB/s = {alg_p / (ma * 1e-6) / PEAK:.3f} of 8 TB/s")
    print(f"(a') algorithmic bytes {alg_d} -> {alg_d / (na * 1e-6) / 1e12:.2f} TB/s = {alg_d / (na * 1e-6) / PEAK:.3f} of 8 TB/s")


if __name__ == "__main__":
    main()
