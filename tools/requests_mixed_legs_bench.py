"""Kernel-clock time of the server's arrival-order decode whose plans go, plan by
plan, into columns or into struct arrays (srpc_frames_unpack_requests_mixed_legs)
beside the two calls of one kind on the same bytes.

Data: the Calculator set (K = 4), `--frames` request frames in uniformly random
order, the natural layouts (TwoNumbers and Number behind a vtable slot: 16-byte
structs); and Calculator + echo (multiple_primitives, K = 5), `--text-frames`
frames in uniformly random order, strings of 0..`--maxlen` bytes.

  rows, for each of the two sets
    (a) _mixed_legs, every plan in columns          (b) _unpack_requests_mixed_var, the same bytes
    (c) _mixed_legs, every fixed plan in records    (d) _unpack_requests_mixed_aos, the same bytes
                                                        (Calculator only: it takes no string plan)
    (h) _mixed_legs, alternate plans in records (add and multiply): no counterpart

(a) launches (b)'s kernels, so it should cost the same.  No ratio was fixed for
(c) and (h) in advance; (c)/(a) is shown beside 1.27, what struct arrays cost the
client-side legs decode.  Every figure is srpc_time_next_call's
interval, all rows interleaved in each of `--reps` rounds after one warm-up
round; medians, extremes and every sample are printed.  Rows of one set read the
same frames; `--cold` rewrites a 1 GiB buffer before each row, so that every row
starts with its stream in HBM (the default leaves the caches as the row before
left them, as tools/requests_mixed_aos_bench.py does).  `--rows b,d` times a
subset: with SRPC_GPU_LIB naming a build of the parent commit, which has rows
(b) and (d) only, whole processes of the two builds are alternated.

    python tools/requests_mixed_legs_bench.py [--frames 4000000] [--text-frames 1000000] [--maxlen 64] [--reps 10] [--cold] [--rows a,b,c,d,h]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from srpc_amd import (NUMBER, TWO_NUMBERS, GpuPacker, MixedAosFrames, MixedFrames, MixedLegFrames,  # noqa: E402
                      MixedVarFrames, Schema, framed_request_prefix, time_next_call)

DEV = torch.device("cuda:0")
PEAK = 8e12  # bytes/s, MI355X HBM3E
SVC = "Calculator_servicer::"
MP = Schema.of("multiple_primitives", ("arg1", "int8"), ("arg2", "char"), ("arg3", "int64"), ("arg4", "string"))
CALC = [("square", NUMBER), ("add", TWO_NUMBERS), ("subtract", TWO_NUMBERS), ("multiply", TWO_NUMBERS)]
STRIDE = 16                       # sizeof(TwoNumbers) == sizeof(Number): a vtable slot, then the int32s
OFFS = {1: [8], 2: [8, 12]}       # leaf offsets by the number of leaves
KINDS = {"a": [False] * 4, "c": [True] * 4, "h": [False, True, False, True]}  # which Calculator plans are record plans


def zeros(nbytes):
    return torch.zeros(int(nbytes) + 16, dtype=torch.uint8, device=DEV)


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


class Set:
    """One set's stream and, per row, outputs of its own."""

    def __init__(self, n, echo, maxlen, gen, st):
        self.n, self.echo = n, echo
        K = self.K = len(CALC) + echo
        self.method = torch.randint(0, K, (n,), dtype=torch.uint8, device=DEV, generator=gen)
        self.count = count = torch.bincount(self.method.to(torch.int64), minlength=K).tolist()
        self.plans = [GpuPacker(s, framed_request_prefix(s, SVC + m)) for m, s in CALC]
        if echo:
            self.plans.append(GpuPacker.for_request(MP, "Echo_servicer::echo"))
        self.F = [p.record_bytes for p in self.plans[:4]]
        rnd = lambda c: torch.randint(-2**31, 2**31 - 1, (c + 4,), dtype=torch.int32, device=DEV, generator=gen)  # noqa: E731
        self.cols = [[rnd(count[k]) for _ in s.kinds] for k, (_, s) in enumerate(CALC)]
        self.so = [None] * 4
        self.chars = 0
        total = sum(c * f for c, f in zip(count, self.F))
        if echo:
            cols, so, self.chars = mp_leg(count[4], maxlen, gen)
            self.cols.append(cols), self.so.append(so)
            total += count[4] * (4 + len(self.plans[4].prefix) + 1 + 1 + 8 + 8) + self.chars
        self.nb = MixedFrames.index_bytes(n, K)
        self.index = zeros(self.nb)
        assert MixedFrames.index(self.method, n, K, self.index, self.nb, zeros(8 * (K + 1)), st) == 0
        # the stream: every call's request in call order, packed by the existing string-aware call
        var = self.var = MixedVarFrames(self.plans)
        sb = var.scratch_bytes(n)
        self.buf, self.offs, d_total = zeros(total), zeros(4 * (n + 1)), zeros(8)
        assert var.pack(self.cols, self.so, None, count, self.method, self.index, n, self.buf, total, self.offs, d_total, st,
                        zeros(sb), sb) == 0
        torch.cuda.synchronize()
        assert u64_at(d_total) == total and not st[:4].any()
        self.buf_len = total
        self.fills = [np.random.default_rng(k).integers(0, 256, STRIDE, dtype=np.uint8).tobytes() for k in range(4)]
        self.rows = {}

    def outputs(self, rec):
        """-> (cols, str_offs, str_cap, recs): a record plan has no columns, a column plan no array."""
        cols, so, cap, recs = [], [], [], []
        for k in range(self.K):
            if k < 4 and rec[k]:
                cols.append(None), so.append(None), cap.append(None), recs.append(zeros(self.count[k] * STRIDE))
            elif k < 4:
                cols.append([zeros(4 * self.count[k]) for _ in CALC[k][1].kinds])
                so.append(None), cap.append(None), recs.append(None)
            else:
                c = self.count[4]
                cols.append([zeros(c), zeros(c), zeros(8 * c), zeros(self.chars)])
                so.append([None, None, None, zeros(8 * (c + 1))])
                cap.append([None, None, None, self.chars]), recs.append(None)
        return cols, so, cap, recs

    def add_rows(self, st, rows):
        n, K, count = self.n, self.K, self.count
        calls = {}

        def common():
            return zeros(n), zeros(self.nb), zeros(8 * (K + 1)), zeros(64)

        for r, rec4 in KINDS.items():
            if r not in rows:
                continue
            rec = rec4 + [False] * self.echo
            mf = MixedLegFrames(self.plans, [STRIDE if x else 0 for x in rec],
                                [OFFS[len(CALC[k][1].kinds)] if rec[k] else None for k in range(K)])
            cols, so, cap, recs = self.outputs(rec)
            cls, index, counts, ends = common()
            sb = mf.scratch_bytes(n)
            scratch = zeros(sb)
            fills = [self.fills[k] if rec[k] else None for k in range(K)]
            self.rows[r] = dict(rec=rec, cols=cols, so=so, recs=recs, cls=cls, index=index, counts=counts, ends=ends, tile=mf.tile)
            calls[r] = (lambda mf=mf, cols=cols, so=so, cap=cap, recs=recs, fills=fills, cls=cls, index=index, counts=counts,
                        ends=ends, scratch=scratch, sb=sb: mf.unpack_requests(
                            self.buf, self.buf_len, self.offs, n, cols, so, cap, recs, fills, None, count, cls, index, self.nb,
                            counts, ends, st, scratch, sb))
        if "b" in rows:
            cols, so, cap, _ = self.outputs([False] * K)
            cls, index, counts, ends = common()
            sb = self.var.scratch_bytes(n)
            scratch = zeros(sb)
            self.rows["b"] = dict(rec=[False] * K, cols=cols, so=so, recs=[None] * K, cls=cls, index=index, counts=counts,
                                  ends=ends, tile=self.var.tile)
            calls["b"] = lambda: self.var.unpack_requests(self.buf, self.buf_len, self.offs, n, cols, so, cap, None, count, cls,
                                                          index, self.nb, counts, ends, st, scratch, sb)
        if not self.echo and "d" in rows:
            aos = MixedAosFrames(self.plans, [STRIDE] * K, [OFFS[len(s.kinds)] for _, s in CALC])
            _, _, _, recs = self.outputs([True] * K)
            cls_d, index_d, counts_d, _ = common()
            sb_d = aos.scratch_bytes
            scratch_d = zeros(sb_d)
            self.rows["d"] = dict(rec=[True] * K, cols=[None] * K, so=[None] * K, recs=recs, cls=cls_d, index=index_d,
                                  counts=counts_d, ends=None, tile=(aos.tile, None))
            calls["d"] = lambda: aos.unpack_requests(self.buf, self.buf_len, self.offs, n, recs, self.fills, None, count, cls_d,
                                                     index_d, self.nb, counts_d, scratch_d, sb_d, st)
        return calls

    def verify(self):
        """Every row computed the same: classes, index, counts, leaves, fills, chars and offsets."""
        n, K, count = self.n, self.K, self.count
        want_counts = torch.tensor(count + [0], dtype=torch.int64, device=DEV)
        for r, o in self.rows.items():
            assert torch.equal(o["cls"][:n], self.method), r
            assert torch.equal(o["index"][:self.nb], self.index[:self.nb]), r
            assert torch.equal(o["counts"][:8 * (K + 1)].view(torch.int64), want_counts), r
            for k in range(4):
                if o["rec"][k]:
                    got = o["recs"][k][:count[k] * STRIDE].view(count[k], STRIDE)
                    words = got.view(torch.int32).view(count[k], 4)
                    fill = torch.frombuffer(bytearray(self.fills[k]), dtype=torch.uint8).to(DEV)
                    for f, c in enumerate(self.cols[k]):
                        assert torch.equal(words[:, 2 + f], c[:count[k]]), (r, k, f)
                    tail = 12 + 4 * (len(self.cols[k]) - 1)
                    assert torch.equal(got[:, :8], fill[:8].expand(count[k], 8)), (r, k)
                    if tail < STRIDE:
                        assert torch.equal(got[:, tail:], fill[tail:].expand(count[k], STRIDE - tail)), (r, k)
                else:
                    for f, c in enumerate(self.cols[k]):
                        assert torch.equal(o["cols"][k][f][:4 * count[k]].view(torch.int32), c[:count[k]]), (r, k, f)
            if self.echo:
                c = count[4]
                assert u64_at(o["ends"]) == self.chars, r
                assert torch.equal(o["cols"][4][3][:self.chars], self.cols[4][3][:self.chars]), r
                assert torch.equal(o["so"][4][3][:8 * (c + 1)].view(torch.int64), self.so[4][3]), r
                assert torch.equal(o["cols"][4][2][:8 * c].view(torch.int64), self.cols[4][2][:c]), r
                assert torch.equal(o["cols"][4][0][:c].view(torch.int8), self.cols[4][0][:c]), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4_000_000)
    ap.add_argument("--text-frames", type=int, default=1_000_000)
    ap.add_argument("--maxlen", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cold", action="store_true", help="evict the caches before each row")
    ap.add_argument("--rows", default="a,c,h,b,d")
    a = ap.parse_args()
    rows = a.rows.split(",")
    assert set(rows) <= set("abcdh"), rows
    evict = torch.zeros(1 << 30, dtype=torch.uint8, device=DEV) if a.cold else None
    gen = torch.Generator(device=DEV).manual_seed(1)
    st = zeros(16)
    sets = {"calculator": Set(a.frames, 0, a.maxlen, gen, st), "calc_echo": Set(a.text_frames, 1, a.maxlen, gen, st)}
    calls = {(name, r): fn for name, S in sets.items() for r, fn in S.add_rows(st, rows).items()}
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
    for S in sets.values():
        S.verify()
    what = {"a": "legs, every plan in columns", "b": "unpack_requests_mixed_var", "c": "legs, every fixed plan in records",
            "d": "unpack_requests_mixed_aos", "h": "legs, add and multiply in records"}
    for name, S in sets.items():
        print(f"{name}: frames {S.n} K {S.K} counts {S.count} fixed frames {S.F} stream bytes {S.buf_len} chars {S.chars} "
              f"struct bytes {STRIDE} tiles " + " ".join(f"({r}) {o['tile']}" for r, o in S.rows.items()))
    print(f"reps {a.reps}   caches {'evicted before every row' if a.cold else 'as the row before left them'}   maxlen {a.maxlen}   "
          f"library {os.environ.get('SRPC_GPU_LIB', 'in-tree')}")
    med = {}
    for k, v in samples.items():
        med[k] = statistics.median(v)
        print(f"{k[0]:10s} ({k[1]}) {what[k[1]]:34s} median {med[k]:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  samples "
              + " ".join(f"{x:.1f}" for x in v))
    for name, S in sets.items():
        if not all((name, r) in med for r in "abch"):
            continue
        A, B, C, H = (med[(name, r)] for r in "abch")
        line = f"{name}: (a)/(b) = {A / B:.3f}   (c)/(a) = {C / A:.3f} (1.27 on the client side)   (h)/(a) = {H / A:.3f}"
        if (name, "d") in med:
            line += f"   (c)/(d) = {C / med[(name, 'd')]:.3f}"
        print(line)
        alg = 2 * S.buf_len + S.n * (4 + 1 + 1)  # the stream twice, offsets, class byte out and in
        out_cols = sum(4 * c * len(s.kinds) for c, (_, s) in zip(S.count, CALC)) + (S.echo and S.count[4] * 18 + 2 * S.chars)
        out_recs = sum(STRIDE * c for c in S.count[:4]) + (S.echo and S.count[4] * 18 + 2 * S.chars)
        for r, out in (("a", out_cols), ("c", out_recs)):
            b = alg + out
            print(f"{name} ({r}) algorithmic bytes {b} -> {b / (med[(name, r)] * 1e-6) / 1e12:.2f} TB/s = "
                  f"{b / (med[(name, r)] * 1e-6) / PEAK:.3f} of 8 TB/s")


if __name__ == "__main__":
    main()
