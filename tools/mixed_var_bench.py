"""Kernel-clock time of the mixed-method calls with a string-bodied leg
(srpc_frames_pack_requests_mixed_var / _unpack_replies_mixed_var) beside the
grouped calls a client without them makes, one per method.

Workload: Calculator (square, add, subtract, multiply) + echo
(multiple_primitives both ways), `--calls` calls in a uniform random order,
strings of 0..`--maxlen` bytes.  Every figure is srpc_time_next_call's interval
(first kernel's begin to last kernel's end), the median of `--reps` runs after
one warm-up.  The grouped path packs and decodes each method's calls on their
own (srpc_gpu_pack, or srpc_gpu_pack_var + srpc_frames_frame_var, the latter
between two events: the hook does not cover it;
srpc_frames_unpack_replies, or srpc_frames_unpack_replies_var) and is summed
over the methods: it does not keep the call order, so it is context, not a bar.
The fraction of 8 TB/s counts the algorithmic bytes once each: columns, frames
and offsets (string offsets, frame offsets, the method bytes).

    python tools/mixed_var_bench.py [--calls 1000000] [--maxlen 64] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import srpc_amd  # noqa: E402
from srpc_amd import (GpuPacker, MixedFrames, MixedVarFrames, Schema, frame_var, framed_request_prefix,  # noqa: E402
                      framed_response_prefix, time_next_call)

DEV = torch.device("cuda:0")
PEAK = 8e12  # bytes/s, MI355X HBM3E
SVC = "Calculator_servicer::"
MP = Schema.of("multiple_primitives", ("arg1", "int8"), ("arg2", "char"), ("arg3", "int64"), ("arg4", "string"))
METHODS = [(SVC + "square", srpc_amd.NUMBER, srpc_amd.NUMBER), (SVC + "add", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER),
           (SVC + "subtract", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER), (SVC + "multiply", srpc_amd.TWO_NUMBERS, srpc_amd.NUMBER),
           ("Echo_servicer::echo", MP, MP)]
DT = {srpc_amd.INT8: np.int8, srpc_amd.CHAR: np.int8, srpc_amd.INT32: np.int32, srpc_amd.INT64: np.int64}


def dev(a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.empty(max(b.size, 16), dtype=torch.uint8, device=DEV)
    t[:b.size].copy_(torch.from_numpy(b.copy()))
    return t


def buf(nbytes):
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def is_var(s):
    return srpc_amd.STRING in s.kinds


def leg(schema, n, maxlen, rng):
    """Device columns, offsets and the column + offsets bytes of n elements."""
    cols, offs, nbytes, chars = [], [], 0, 0
    for k in schema.kinds:
        if k == srpc_amd.STRING:
            o = np.zeros(n + 1, np.uint64)
            o[1:] = np.cumsum(rng.integers(0, maxlen + 1, n).astype(np.uint64))
            chars = int(o[n])
            cols.append(dev(rng.integers(0, 256, max(chars, 1), dtype=np.uint8)))
            offs.append(dev(o))
            nbytes += chars + 8 * (n + 1)
        else:
            dt = np.dtype(DT[k])
            cols.append(dev(rng.integers(0, 127, max(n, 1)).astype(dt)))
            offs.append(None)
            nbytes += n * dt.itemsize
    return cols, offs, nbytes, chars


def timed(fn, reps):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s), b.record(s)
    torch.cuda.synchronize()
    out = []
    for r in range(reps + 1):
        fn(lambda: time_next_call(a, b))
        torch.cuda.synchronize()
        if r:
            out.append(a.elapsed_time(b) * 1e3)  # us
    return statistics.median(out)


def timed_events(fn, reps):
    """For a call the hook does not cover (srpc_frames_frame_var): events around it."""
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for r in range(reps + 1):
        a.record(s)
        fn()
        b.record(s)
        torch.cuda.synchronize()
        if r:
            out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1_000_000)
    ap.add_argument("--maxlen", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, K = a.calls, len(METHODS)
    rng = np.random.default_rng(1)
    method = rng.integers(0, K, n).astype(np.uint8)
    counts = [int(np.sum(method == k)) for k in range(K)]
    req_p = [GpuPacker.for_request(q, m) if is_var(q) else GpuPacker(q, framed_request_prefix(q, m)) for m, q, _ in METHODS]
    rep_p = [GpuPacker.for_response(r, 0) if is_var(r) else GpuPacker(r, framed_response_prefix(r, 0)) for _, _, r in METHODS]
    req = [leg(q, counts[k], a.maxlen, rng) for k, (_, q, _) in enumerate(METHODS)]
    rep = [leg(r, counts[k], a.maxlen, rng) for k, (_, _, r) in enumerate(METHODS)]
    MQ, MR = MixedVarFrames(req_p), MixedVarFrames(rep_p)
    d_method = dev(method)
    ib = MixedFrames.index_bytes(n, K)
    d_index, d_counts = buf(ib), buf(8 * (K + 1))
    assert MixedFrames.index(d_method, n, K, d_index, ib, d_counts, None) == 0

    def frame_total(plans, legs):
        t = 0
        for p, (m, q, r), (_, _, _, chars), c in zip(plans, METHODS, legs, counts):
            sch = p.schema
            fixed = 4 + len(p.prefix) + sum(8 if k == srpc_amd.STRING else np.dtype(DT[k]).itemsize for k in sch.kinds) \
                if is_var(sch) else p.record_bytes
            t += c * fixed + chars
        return t

    q_total, r_total = frame_total(req_p, req), frame_total(rep_p, rep)
    d_out, d_offs, d_total = buf(q_total + 16), buf(4 * (n + 1)), buf(8)
    sb = max(MQ.scratch_bytes(n), MR.scratch_bytes(n))
    d_scratch = buf(sb)
    st = buf(16)
    res = {"calls": n, "maxlen": a.maxlen, "reps": a.reps, "counts": counts, "request_bytes": q_total,
           "reply_bytes": r_total}

    def mixed_pack(arm):
        arm()
        rc = MQ.pack([l[0] for l in req], [l[1] for l in req], None, counts, d_method, d_index, n, d_out, q_total, d_offs,
                     d_total, st, d_scratch, sb)
        assert rc == 0, rc

    res["mixed_var_pack_us"] = timed(mixed_pack, a.reps)
    assert int(d_total.cpu().numpy().view(np.uint64)[0]) == q_total

    # the reply stream in call order: the same pack over the reply plans and columns
    d_rbuf, d_roffs = buf(r_total + 16), buf(4 * (n + 1))
    rc = MR.pack([l[0] for l in rep], [l[1] for l in rep], None, counts, d_method, d_index, n, d_rbuf, r_total, d_roffs,
                 d_total, st, d_scratch, sb)
    torch.cuda.synchronize()
    assert rc == 0 and int(d_total.cpu().numpy().view(np.uint64)[0]) == r_total
    out_cols = [[buf(c.numel()) for c in l[0]] for l in rep]
    out_offs = [[None if o is None else buf(o.numel()) for o in l[1]] for l in rep]
    scap = [[None if o is None else c.numel() for c, o in zip(l[0], l[1])] for l in rep]
    d_codes, d_ends = buf(n), buf(8 * 8)

    def mixed_unpack(arm):
        arm()
        rc = MR.unpack(d_rbuf, r_total, d_roffs, n, d_method, d_index, n, 2, out_cols, out_offs, scap, None, counts,
                       d_codes, d_ends, st, d_scratch, sb)
        assert rc == 0, rc

    res["mixed_var_decode_us"] = timed(mixed_unpack, a.reps)
    flags = int(st.cpu().numpy()[:4].view(np.uint32)[0])
    assert flags == 0, flags
    for k in range(K):  # the decode reproduces the reply columns
        for c, o in zip(rep[k][0], out_cols[k]):
            assert torch.equal(c, o), k
    assert (d_codes.cpu().numpy()[:n] == 0).all()

    # the grouped path: each method's calls on their own
    g_pack = g_dec = 0.0
    for k, (m, q, r) in enumerate(METHODS):
        c = counts[k]
        if is_var(q):
            cap = c * 64 + req[k][3] + 16
            wire, rec, fr = buf(cap), buf(8 * (c + 1)), buf(cap + 4 * c)
            vs = req_p[k].var_scratch_bytes(c, cap)
            vscr = buf(vs)
            g_pack += timed(lambda arm: (arm(), req_p[k].pack_var(req[k][0], req[k][1], c, wire, cap, rec, vscr, vs)), a.reps)
            g_pack += timed_events(lambda: frame_var(wire, rec, c, fr, cap + 4 * c), a.reps)
        else:
            wire = buf(c * req_p[k].record_bytes)
            g_pack += timed(lambda arm: (arm(), req_p[k].pack(req[k][0], c, wire)), a.reps)
        codes = buf(c)
        if is_var(r):
            cap = c * 64 + rep[k][3] + 16
            wire, rec, fr = buf(cap), buf(8 * (c + 1)), buf(cap + 4 * c + 16)
            vs = rep_p[k].var_scratch_bytes(c, cap)
            vscr = buf(vs)
            rep_p[k].pack_var(rep[k][0], rep[k][1], c, wire, cap, rec, vscr, vs)
            frame_var(wire, rec, c, fr, cap + 4 * c)
            torch.cuda.synchronize()
            ro = rec.cpu().numpy()[:8 * (c + 1)].view(np.uint64)
            flen = int(ro[c]) + 4 * c
            foffs = dev((ro[:c] + 4 * np.arange(c, dtype=np.uint64)).astype(np.uint32))
            rs = rep_p[k].replies_var_scratch_bytes(c)
            rscr = buf(rs)
            oc = [buf(flen if o is not None else x.numel()) for x, o in zip(rep[k][0], rep[k][1])]
            oo = [None if o is None else buf(o.numel()) for o in rep[k][1]]
            g_dec += timed(lambda arm: (arm(), rep_p[k].unpack_replies_var(fr, flen, foffs, c, oc, oo, codes, rscr, rs)),
                           a.reps)
        else:
            F = rep_p[k].record_bytes
            wire = buf(c * F + 16)
            rep_p[k].pack(rep[k][0], c, wire)
            oc = [buf(x.numel()) for x in rep[k][0]]
            g_dec += timed(lambda arm: (arm(), rep_p[k].unpack_replies(wire, c * F, None, c, oc, codes)), a.reps)
    res["grouped_pack_us"], res["grouped_decode_us"] = g_pack, g_dec

    # algorithmic bytes: columns + string offsets, frames, frame offsets, method bytes -- each once
    pack_bytes = sum(l[2] for l in req) + q_total + 4 * (n + 1) + n
    dec_bytes = sum(l[2] for l in rep) + r_total + 4 * n + n + n
    res["pack_bytes"], res["decode_bytes"] = pack_bytes, dec_bytes
    for name, nb in (("mixed_var_pack", pack_bytes), ("mixed_var_decode", dec_bytes), ("grouped_pack", pack_bytes),
                     ("grouped_decode", dec_bytes)):
        res[name + "_fraction_of_8TBps"] = nb / (res[name + "_us"] * 1e-6) / PEAK
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
