"""Kernel-clock time of the server's arrival-order decode into struct arrays
(srpc_frames_unpack_requests_mixed_aos) beside the calls that bracket it
(DESIGN §4.15): the Calculator set, K = 4, `--frames` request frames in
uniformly random order, the natural layouts (TwoNumbers and Number behind a
vtable slot: 16-byte structs).

  request decode  (a)  _unpack_requests_mixed_aos   (b)  _unpack_requests_mixed,
                                                         the same frames
  reply decode    (a') _unpack_replies_mixed_aos    (b') _unpack_replies_mixed
                       (the pair of tools/mixed_aos_bench.py, in the same run)
  context         (e)  what the bucket route spends on the same frames:
                       srpc_frames_classify, then per method srpc_frames_gather
                       and srpc_gpu_unpack_aos_fill (the sum of the nine calls)

The yardstick, fixed before measuring: struct arrays cost the request decode no
more than they cost the reply decode on the same box, (a)/(b) <= 1.10 * (a')/(b').
Every figure is srpc_time_next_call's interval, all calls interleaved in each of
`--reps` rounds after one warm-up round; medians, extremes and every sample are
printed.  `--rows a,b` times a subset (A/B runs of two builds of the library,
SRPC_GPU_LIB, alternate whole processes of it).

    python tools/requests_mixed_aos_bench.py [--frames 4000000] [--reps 10] [--rows a,b,a',b',e]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from srpc_amd import (NUMBER, RPC_ERR_RECV_TIMEOUT, TWO_NUMBERS, FrameClassifier, GpuPacker, MixedAosFrames,  # noqa: E402
                      MixedFrames, framed_request_prefix, framed_response_prefix, time_next_call)

DEV = torch.device("cuda:0")
PEAK = 8e12  # bytes/s, MI355X HBM3E
SVC = "Calculator_servicer::"
METHODS = [("square", NUMBER), ("add", TWO_NUMBERS), ("subtract", TWO_NUMBERS), ("multiply", TWO_NUMBERS)]
STRIDE = 16                       # sizeof(TwoNumbers) == sizeof(Number): a vtable slot, then the int32s
OFFS = {1: [8], 2: [8, 12]}       # leaf offsets by the number of leaves
ROWS = ["a", "b", "a'", "b'", "e"]


def zeros(nbytes):
    return torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default=",".join(ROWS))
    a = ap.parse_args()
    rows = a.rows.split(",")
    assert set(rows) <= set(ROWS), rows
    n, K = a.frames, len(METHODS)
    gen = torch.Generator(device=DEV).manual_seed(1)
    method = torch.randint(0, K, (n,), dtype=torch.uint8, device=DEV, generator=gen)
    count = torch.bincount(method.to(torch.int64), minlength=K).tolist()
    rq_plans = [GpuPacker(s, framed_request_prefix(s, SVC + m)) for m, s in METHODS]
    rs_plans = [GpuPacker(NUMBER, framed_response_prefix(NUMBER, 0)) for _ in METHODS]
    Fq, Fr = [p.record_bytes for p in rq_plans], [p.record_bytes for p in rs_plans]
    rnd = lambda c: torch.randint(-2**31, 2**31 - 1, (c + 4,), dtype=torch.int32, device=DEV, generator=gen)
    q_cols = [[rnd(count[k]) for _ in s.kinds] for k, (_, s) in enumerate(METHODS)]
    s_cols = [[rnd(count[k])] for k in range(K)]                      # the replies' values
    q_offs = [OFFS[len(s.kinds)] for _, s in METHODS]
    q_aos = MixedAosFrames(rq_plans, [STRIDE] * K, q_offs)
    s_aos = MixedAosFrames(rs_plans, [STRIDE] * K, [OFFS[1]] * K)
    q_col, s_col = MixedFrames(rq_plans), MixedFrames(rs_plans)
    nb = MixedFrames.index_bytes(n, K)
    index, counts, st = zeros(nb), zeros(8 * (K + 1)), zeros(16)
    assert MixedFrames.index(method, n, K, index, nb, counts, st) == 0
    # both streams: every call's request and its full reply in call order, packed by the column calls
    qbuf, qoffs = zeros(n * max(Fq)), zeros(4 * (n + 1))
    assert q_col.pack(q_cols, None, count, method, index, n, qbuf, n * max(Fq), qoffs, st) == 0
    rbuf, roffs = zeros(n * max(Fr)), zeros(4 * (n + 1))
    assert s_col.pack(s_cols, None, count, method, index, n, rbuf, n * max(Fr), roffs, st) == 0
    torch.cuda.synchronize()
    qlen = int(qoffs[:4 * (n + 1)].view(torch.int32)[n].item())
    rlen = int(roffs[:4 * (n + 1)].view(torch.int32)[n].item())
    fills = [np.random.default_rng(k).integers(0, 256, STRIDE, dtype=np.uint8).tobytes() for k in range(K)]
    # (a), (b): outputs of their own
    recs_a = [zeros(count[k] * STRIDE) for k in range(K)]
    cols_b = [[zeros(4 * count[k]) for _ in s.kinds] for k, (_, s) in enumerate(METHODS)]
    cls_a, cls_b, index_a, index_b = zeros(n), zeros(n), zeros(nb), zeros(nb)
    counts_a, counts_b = zeros(8 * (K + 1)), zeros(8 * (K + 1))
    sb_q, sb_s = q_aos.scratch_bytes, s_aos.scratch_bytes
    scratch_q, scratch_s = zeros(sb_q), zeros(sb_s)
    # (a'), (b')
    recs_r = [zeros(count[k] * STRIDE) for k in range(K)]
    cols_r = [[zeros(4 * count[k])] for k in range(K)]
    codes_a, codes_b = zeros(n), zeros(n)
    # (e)
    clf = FrameClassifier(list(zip(rq_plans, Fr)))
    sb_e = clf.scratch_bytes(n)
    cls_e, idx_e, counts_e, out_off_e, scratch_e = zeros(n), zeros(4 * K * n), zeros(8 * (K + 2)), zeros(8 * (n + 1)), zeros(sb_e)
    gathered = zeros(n * max(Fq))
    recs_e = [zeros(count[k] * STRIDE) for k in range(K)]

    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s), e1.record(s)
    torch.cuda.synchronize()

    def timed(fn):
        """One C-ABI call's kernels, us."""
        st.zero_()
        time_next_call(e0, e1)
        rc = fn()
        torch.cuda.synchronize()
        assert not rc and not st[:4].any(), rc
        return e0.elapsed_time(e1) * 1e3

    def bucket_route():
        t = timed(lambda: clf.classify(qbuf, qlen, qoffs, n, cls_e, idx_e, counts_e, out_off_e, scratch_e, sb_e))
        for k in range(K):
            t += timed(lambda: FrameClassifier.gather(qbuf, qoffs, idx_e.data_ptr() + 4 * k * n, count[k], Fq[k], gathered))
            t += timed(lambda: rq_plans[k].unpack_aos_fill(gathered, count[k] * Fq[k], count[k], recs_e[k], STRIDE,
                                                           q_offs[k], fills[k], st))
        return t

    calls = {
        "a": ("unpack_requests_mixed_aos", lambda: timed(lambda: q_aos.unpack_requests(
            qbuf, qlen, qoffs, n, recs_a, fills, None, count, cls_a, index_a, nb, counts_a, scratch_q, sb_q, st))),
        "b": ("unpack_requests_mixed", lambda: timed(lambda: q_col.unpack_requests(
            qbuf, qlen, qoffs, n, cols_b, None, count, cls_b, index_b, nb, counts_b, st))),
        "a'": ("unpack_replies_mixed_aos", lambda: timed(lambda: s_aos.unpack(
            rbuf, rlen, roffs, n, method, index, n, RPC_ERR_RECV_TIMEOUT, recs_r, fills, None, count, codes_a, scratch_s,
            sb_s, st))),
        "b'": ("unpack_replies_mixed", lambda: timed(lambda: s_col.unpack(
            rbuf, rlen, roffs, n, method, index, n, RPC_ERR_RECV_TIMEOUT, cols_r, None, count, codes_b, st))),
        "e": ("classify + 4 x (gather + unpack_aos_fill)", bucket_route),
    }
    samples = {k: [] for k in rows}
    for r in range(a.reps + 1):
        for k in rows:
            t = calls[k][1]()
            if r:
                samples[k].append(t)
    # every form computed the same
    want_counts = torch.tensor(count + [0], dtype=torch.int64, device=DEV)
    for k in range(K):
        want = torch.frombuffer(bytearray(fills[k]), dtype=torch.uint8).to(DEV)
        for row, recs, cols in (("a", recs_a, q_cols), ("a'", recs_r, s_cols)):
            if row not in rows:
                continue
            got = recs[k][:count[k] * STRIDE].view(count[k], STRIDE)
            words = got.view(torch.int32).view(count[k], 4)
            for f, c in enumerate(cols[k]):
                assert torch.equal(words[:, 2 + f], c[:count[k]]), (row, k, f)
            tail = 12 + 4 * (len(cols[k]) - 1)
            assert torch.equal(got[:, :8], want[:8].expand(count[k], 8)), (row, k)
            if tail < STRIDE:
                assert torch.equal(got[:, tail:], want[tail:].expand(count[k], STRIDE - tail)), (row, k)
        if "b" in rows:
            for f, c in enumerate(q_cols[k]):
                assert torch.equal(cols_b[k][f][:4 * count[k]].view(torch.int32), c[:count[k]])
        if "e" in rows:  # bucket order is whatever the atomics gave: the same leaves as a set
            for f, c in enumerate(q_cols[k]):
                got = recs_e[k][:count[k] * STRIDE].view(torch.int32).view(count[k], 4)[:, 2 + f]
                assert torch.equal(got.sort().values, c[:count[k]].sort().values)
    if "a" in rows:
        assert torch.equal(cls_a[:n], method) and torch.equal(counts_a[:8 * (K + 1)].view(torch.int64), want_counts)
        assert torch.equal(index_a[:nb], index[:nb])
    if "a" in rows and "b" in rows:
        assert torch.equal(cls_a[:n], cls_b[:n]) and torch.equal(index_a[:nb], index_b[:nb])
    if "a'" in rows:
        assert not codes_a[:n].any()
    print(f"frames {n} K {K} counts {count} request frames {Fq} reply frames {Fr} struct bytes {STRIDE} reps {a.reps} "
          f"tiles: request decode {q_aos.tile} (columns {q_col.tile}) reply decode {s_aos.tile} scratch {sb_q} B "
          f"library {os.environ.get('SRPC_GPU_LIB', 'in-tree')}")
    med = {}
    for k in rows:
        v = samples[k]
        med[k] = statistics.median(v)
        print(f"{k:2s} {calls[k][0]:42s} median {med[k]:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  samples "
              + " ".join(f"{x:.1f}" for x in v))
    if all(k in med for k in ("a", "b", "a'", "b'")):
        x, y = med["a"] / med["b"], med["a'"] / med["b'"]
        print(f"request decode aos/columns = {x:.3f}   reply decode aos/columns = {y:.3f}   yardstick 1.10 * {y:.3f} = "
              f"{1.10 * y:.3f}   the request decode {'is within' if x <= 1.10 * y else 'MISSES'} it")
    if "a" in med:
        alg = 2 * qlen + n * (4 + 1 + 1 + STRIDE)  # the stream twice, offsets, class byte out and in, structs
        print(f"(a)  algorithmic bytes {alg} -> {alg / (med['a'] * 1e-6) / 1e12:.2f} TB/s = "
              f"{alg / (med['a'] * 1e-6) / PEAK:.3f} of 8 TB/s")
    if "a" in med and "e" in med:
        print(f"(e)/(a) = {med['e'] / med['a']:.2f}: the bucket route's classify, gathers and fills over the ordered decode")


if __name__ == "__main__":
    main()
