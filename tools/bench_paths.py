#!/usr/bin/env python3
"""Throughput of every kernel family on representative schemas (one MI355X).

For each case: pack and unpack of N records through the C ABI, timed on the
kernel clock of srpc_time_next_call (dispatch begin of the call's first
kernel to end of its last; median of R reps after warm-up), reported
as algorithmic GB/s (columns + wire bytes moved once) and fraction of the
8 TB/s HBM3E peak.  Every case is first checked bit-exact against the CPU
oracle on a 4096-record prefix of the same inputs.

    python tools/bench_paths.py [--reps 20] [--out gpurun_out/paths.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="substring filter on case names")
    ap.add_argument("--replies-var-frames", type=int, default=1 << 24,
                    help="frames of the replies_var rows (default 16M, the other reply rows' n)")
    ap.add_argument("--mixed-calls", type=int, default=1 << 24, help="calls of the mixed rows (default 16M)")
    ap.add_argument("--var-kernel", default="", help="VAR cases: comma list of pack kernels to time "
                    "(1 record tiles, 0 scan + walk; default: the plan's default)")
    ap.add_argument("--var-caps", default="", help="VAR record tiles: IMAGE:CHARS bytes (default: the plan's)")
    ap.add_argument("--rec-ab", action="store_true",
                    help="fixed cases: also time the generic TILE kernels (rec_kernel=0) beside the default")
    ap.add_argument("--no-stream", dest="stream", action="store_false",
                    help="VAR cases: skip the index-free stream decode timing")
    args = ap.parse_args()

    import numpy as np
    import torch

    import oracle
    import srpc_amd
    from srpc_amd import NUMBER, QUAD, SQUARE_METHOD, GpuPacker, Schema

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    rows = []

    def timeit(fn):
        for _ in range(3):
            fn()
        ts = []
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(s)
        b.record(s)
        for _ in range(args.reps):
            # kernel clock: the call's first kernel begin -> last kernel end
            srpc_amd.time_next_call(a, b)
            fn()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / 1e3)
        return statistics.median(ts)

    def t_u8(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def fixed_case(name, sch, n, prefix=b"", path=None):
        if args.only not in name:
            return
        p = GpuPacker(sch, prefix)
        if path:
            p.force_path(path)
        rng = np.random.default_rng(1)
        cols = []
        for k in sch.kinds:
            dt = np.dtype(oracle.KIND_DTYPE[k])
            c = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
            cols.append((c & 1).astype(np.uint8) if k == oracle.BOOL else c)
        dcols = [t_u8(c) for c in cols]
        wire = torch.empty(n * p.record_bytes + 16, dtype=torch.uint8, device=dev)
        back = [torch.empty_like(c) for c in dcols]
        p.pack(dcols, n, wire, stream=s)
        torch.cuda.synchronize()
        m = 4096
        ok = wire[: m * p.record_bytes].cpu().numpy().tobytes() == oracle.pack(
            sch.kinds, [c[:m] for c in cols], m, prefix)
        col_bytes = sum(c.nbytes for c in cols)
        alg = col_bytes + n * p.record_bytes
        tp = timeit(lambda: p.pack(dcols, n, wire, stream=s))
        tu = timeit(lambda: p.unpack(wire, n * p.record_bytes, n, back, stream=s))
        ok = ok and all(torch.equal(a, b) for a, b in zip(dcols, back))
        generic = {}
        if args.rec_ab and p.path == 2:
            p.tune(rec_kernel=0)
            gp = timeit(lambda: p.pack(dcols, n, wire, stream=s))
            gu = timeit(lambda: p.unpack(wire, n * p.record_bytes, n, back, stream=s))
            p.tune(rec_kernel=2)
            rp = timeit(lambda: p.pack(dcols, n, wire, stream=s))
            ru = timeit(lambda: p.unpack(wire, n * p.record_bytes, n, back, stream=s))
            p.tune(rec_kernel=1)
            generic = {"generic_pack_frac": round(alg / gp / 8e12, 4), "generic_unpack_frac": round(alg / gu / 8e12, 4),
                       "rec_pack_frac": round(alg / rp / 8e12, 4), "rec_unpack_frac": round(alg / ru / 8e12, 4)}
        rows.append({"case": name, "path": {1: "dword", 2: "tile", 3: "var"}[p.path], "records": n,
                     "record_bytes": p.record_bytes, "alg_bytes": alg, "pack_us": round(tp * 1e6, 2),
                     "unpack_us": round(tu * 1e6, 2), "pack_GBps": round(alg / tp / 1e9, 1),
                     "unpack_GBps": round(alg / tu / 1e9, 1), "pack_frac": round(alg / tp / 8e12, 4),
                     "unpack_frac": round(alg / tu / 8e12, 4), "parity_ok": bool(ok), **generic})

    def spread(ts):
        return {"median_us": round(statistics.median(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2),
                "max_us": round(max(ts) * 1e6, 2)}

    def replies_case(name, sch, n):
        """Reply streams of n frames decoded in call order (srpc_frames_unpack_replies):
        uniform mode, indexed mode on the same all-full stream, indexed mode with
        1 % bare error frames.  Algorithmic bytes: frame bytes + column bytes +
        1 code byte (+ 4 offset bytes when indexed) per frame.  Beside them,
        srpc_gpu_unpack of the same all-success bytes, and the route the call
        replaces on the all-full indexed stream (srpc_frames_classify + _gather +
        srpc_gpu_unpack), timed alternately with the new call on stream events."""
        if args.only not in name:
            return
        from srpc_amd import FrameClassifier, framed_response_prefix
        pre = framed_response_prefix(sch, 0)
        p = GpuPacker(sch, pre)
        F = p.record_bytes
        rng = np.random.default_rng(2)
        cols = []
        for k in sch.kinds:
            dt = np.dtype(oracle.KIND_DTYPE[k])
            c = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
            cols.append((c & 1).astype(np.uint8) if k == oracle.BOOL else c)
        dcols = [t_u8(c) for c in cols]
        col_bytes = sum(c.nbytes for c in cols)
        wire = torch.empty(n * F + 16, dtype=torch.uint8, device=dev)
        p.pack(dcols, n, wire, stream=s)
        torch.cuda.synchronize()
        m = 4096
        opre = (len(pre) - 4 + sch.body_bytes).to_bytes(4, "big") + oracle.response_prefix(0, sch.name)
        made_ok = wire[: m * F].cpu().numpy().tobytes() == oracle.pack(sch.kinds, [c[:m] for c in cols], m, opre)
        back = [torch.empty_like(c) for c in dcols]
        codes = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        st = torch.zeros(16, dtype=torch.uint8, device=dev)

        def clear():
            for b in back:
                b.fill_(0xA5)
            codes.fill_(0xA5)

        def same(want_cols, want_codes):
            torch.cuda.synchronize()
            return (all(torch.equal(a, b) for a, b in zip(want_cols, back)) and torch.equal(codes[:n], want_codes)
                    and not bool(st[:4].any()))

        def row(mode, alg, t, ok, **extra):
            rows.append({"case": f"{name}_{mode}", "replies": True, "frames": n, "frame_bytes": F, "alg_bytes": alg,
                         "us": round(t * 1e6, 2), "GBps": round(alg / t / 1e9, 1), "frac": round(alg / t / 8e12, 4),
                         "parity_ok": bool(ok), **extra})

        zeros = torch.zeros(n, dtype=torch.uint8, device=dev)
        # uniform mode, beside srpc_gpu_unpack of the same bytes
        clear()
        p.unpack_replies(wire, n * F, None, n, back, codes, st, stream=s)
        ok = made_ok and same(dcols, zeros)
        t = timeit(lambda: p.unpack_replies(wire, n * F, None, n, back, codes, st, stream=s))
        tu = timeit(lambda: p.unpack(wire, n * F, n, back, stream=s))
        alg_u = n * F + col_bytes
        row("uniform", alg_u + n, t, ok, unpack_us=round(tu * 1e6, 2), unpack_alg_bytes=alg_u,
            unpack_frac=round(alg_u / tu / 8e12, 4), time_per_byte_vs_unpack=round((t / (alg_u + n)) / (tu / alg_u), 4))
        # indexed mode, all frames full; the route it replaces, alternately
        offs = (torch.arange(n, dtype=torch.int64, device=dev) * F).to(torch.int32).contiguous()
        clear()
        p.unpack_replies(wire, n * F, offs, n, back, codes, st, stream=s)
        ok = made_ok and same(dcols, zeros)
        t = timeit(lambda: p.unpack_replies(wire, n * F, offs, n, back, codes, st, stream=s))
        fc = FrameClassifier([(p, 0)])
        sb = fc.scratch_bytes(n)
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
        d_cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        d_idx = torch.empty(4 * n + 16, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(8 * 3, dtype=torch.uint8, device=dev)
        d_out_off = torch.empty(8 * (n + 1), dtype=torch.uint8, device=dev)
        gathered = torch.empty(n * F + 16, dtype=torch.uint8, device=dev)

        def route():
            fc.classify(wire, n * F, offs, n, d_cls, d_idx, d_counts, d_out_off, scratch, sb, stream=s)
            fc.gather(wire, offs, d_idx, n, F, gathered, stream=s)
            p.unpack(gathered, n * F, n, back, stream=s)

        def ev(fn):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / 1e3

        new = lambda: p.unpack_replies(wire, n * F, offs, n, back, codes, st, stream=s)  # noqa: E731
        for _ in range(3):
            route()
            new()
        t_new, t_route = [], []
        for _ in range(args.reps):
            t_new.append(ev(new))
            t_route.append(ev(route))
        row("indexed_full", alg_u + 5 * n, t, ok, ab_new=spread(t_new), ab_route=spread(t_route))
        # indexed mode, 1 % bare `BE32(1) | code 1` frames
        fr = wire[: n * F].cpu().numpy().reshape(n, F).copy()
        bare = rng.random(n) < 0.01
        fr[bare, :5] = np.array([0, 0, 0, 1, 1], np.uint8)
        keep = np.ones((n, F), bool)
        keep[bare, 5:] = False
        mixed = fr[keep]
        del fr, keep
        lens = np.where(bare, 5, F).astype(np.int64)
        o = np.zeros(n, np.int64)
        np.cumsum(lens[:-1], out=o[1:])
        d_mixed = torch.empty(mixed.size + 16, dtype=torch.uint8, device=dev)
        d_mixed[: mixed.size].copy_(torch.from_numpy(mixed))
        d_o = torch.from_numpy(o.astype(np.uint32).view(np.int32)).to(dev)
        d_bare = torch.from_numpy(bare).to(dev)
        want_cols = [torch.where(d_bare.repeat_interleave(c.numel() // n), torch.zeros_like(c), c) for c in dcols]
        clear()
        p.unpack_replies(d_mixed, mixed.size, d_o, n, back, codes, st, stream=s)
        ok = made_ok and same(want_cols, d_bare.to(torch.uint8))
        t = timeit(lambda: p.unpack_replies(d_mixed, mixed.size, d_o, n, back, codes, st, stream=s))
        row("indexed_1pct_bare", mixed.size + col_bytes + 5 * n, t, ok)

    def replies_var_case(name, sch, n, maxlen):
        """Reply streams of n frames of a string response decoded in call order
        (srpc_frames_unpack_replies_var): all frames full, and with 1 % bare
        error frames.  The stream is made on the device (pack_var + frame_var)
        and its first 4096 frames are checked against the CPU oracle; the
        decode of the whole stream is checked against the inputs.  Algorithmic
        bytes: stream + fixed columns + chars + 8 (n + 1) offset bytes per
        string field + 1 code and 4 frame-offset bytes per frame.  Beside the
        all-full row, the route the library offered before -- srpc_frames_gather_var
        with an identity index, then srpc_gpu_unpack_var -- timed alternately
        with the new call on stream events, and unpack_var alone on the kernel
        clock."""
        if args.only not in name:
            return
        from srpc_amd import FrameClassifier, frame_var
        STRING = oracle.STRING
        kinds = sch.kinds
        pre = oracle.response_prefix(0, sch.name)
        p = GpuPacker.for_response(sch, 0)
        rng = np.random.default_rng(4)
        cols, offs = [], []
        for k in kinds:
            if k == STRING:
                o = np.zeros(n + 1, np.uint64)
                np.cumsum(rng.integers(0, maxlen + 1, n), out=o[1:])
                cols.append(rng.integers(0, 256, max(1, int(o[-1])), dtype=np.uint8))
                offs.append(o)
            else:
                dt = np.dtype(oracle.KIND_DTYPE[k])
                cols.append(rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt))
                offs.append(None)
        dcols = [t_u8(c) for c in cols]
        doffs = [None if o is None else torch.from_numpy(o.view(np.int64)).to(dev) for o in offs]
        nstr = sum(k == STRING for k in kinds)
        fixed = len(pre) + sum(8 if k == STRING else oracle.KIND_SIZE[k] for k in kinds)
        chars = sum(int(o[-1]) for o in offs if o is not None)
        total = n * fixed + chars
        assert total + 4 * n < 1 << 32
        wire = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        rec = torch.empty(n + 1, dtype=torch.int64, device=dev)
        vsb = p.var_scratch_bytes(n, total + 4 * n)
        vscratch = torch.empty(vsb + 16, dtype=torch.uint8, device=dev)
        st = torch.zeros(16, dtype=torch.uint8, device=dev)
        p.pack_var(dcols, doffs, n, wire, total, rec, vscratch, vsb, st, stream=s)
        buf_len = total + 4 * n
        frames = torch.empty(buf_len + 16, dtype=torch.uint8, device=dev)
        frame_var(wire, rec, n, frames, buf_len, st, stream=s)
        torch.cuda.synchronize()
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        f_off = rec[:n] + 4 * ar                 # frame starts
        f_len = rec[1:] - rec[:n] + 4
        m = 4096
        ow = oracle.pack(kinds, [c[:m] if o is None else c for c, o in zip(cols, offs)], m, pre,
                         [None if o is None else o[:m + 1].copy() for o in offs])
        orec = rec[:m + 1].cpu().numpy()
        want = b"".join(int(orec[i + 1] - orec[i]).to_bytes(4, "big") + ow[int(orec[i]):int(orec[i + 1])] for i in range(m))
        made_ok = (not bool(st[:4].any()) and int(rec[n]) == total and len(ow) == int(orec[m])
                   and frames[:len(want)].cpu().numpy().tobytes() == want)
        del wire

        def u32(t):
            return t.to(torch.int32).contiguous()  # values under 2^32 keep their low 32 bits

        def gather_runs(src, starts, lens):
            """src[starts[i] : starts[i] + lens[i]] back to back, 2M runs at a time."""
            ends = torch.cumsum(lens, 0)
            out = torch.empty(int(ends[-1]) + 16, dtype=torch.uint8, device=dev)
            step = 1 << 21
            for a in range(0, n, step):
                b = min(n, a + step)
                l = lens[a:b]
                o0 = int(ends[a] - lens[a])
                tot = int(ends[b - 1]) - o0
                if not tot:
                    continue
                fid = torch.repeat_interleave(torch.arange(b - a, device=dev), l)
                within = torch.arange(tot, device=dev) - (ends[a:b] - l - o0)[fid]
                out[o0:o0 + tot] = src[starts[a:b][fid] + within]
            return out, ends

        back = [torch.empty(buf_len + 16 if k == STRING else c.numel(), dtype=torch.uint8, device=dev)
                for k, c in zip(kinds, dcols)]
        boffs = [torch.empty(n + 1, dtype=torch.int64, device=dev) if k == STRING else None for k in kinds]
        codes = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        sb = p.replies_var_scratch_bytes(n)
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev)

        def clear():
            for b in back:
                b.fill_(0xA5)
            codes.fill_(0xA5)

        def same(want_cols, want_offs, want_codes):
            torch.cuda.synchronize()
            ok = torch.equal(codes[:n], want_codes) and not bool(st[:4].any())
            for k, wc, wo, b, bo in zip(kinds, want_cols, want_offs, back, boffs):
                if k == STRING:
                    ok = ok and torch.equal(bo, wo) and torch.equal(b[:int(wo[n])], wc[:int(wo[n])])
                else:
                    ok = ok and torch.equal(b, wc)
            return bool(ok)

        def row(mode, alg, t, ok, **extra):
            rows.append({"case": f"{name}_{mode}", "replies": True, "frames": n, "frame_bytes": round(buf_len / n, 1),
                         "alg_bytes": alg, "us": round(t * 1e6, 2), "GBps": round(alg / t / 1e9, 1),
                         "frac": round(alg / t / 8e12, 4), "parity_ok": bool(ok), **extra})

        def ev(fn):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / 1e3

        fixed_bytes = sum(c.nbytes for c, k in zip(cols, kinds) if k != STRING)
        zeros = torch.zeros(n, dtype=torch.uint8, device=dev)
        # all frames full
        d_o = u32(f_off)
        new = lambda: p.unpack_replies_var(frames, buf_len, d_o, n, back, boffs, codes, scratch, sb, st, stream=s)  # noqa: E731
        clear()
        new()
        ok = made_ok and same(dcols, doffs, zeros)
        t = timeit(new)
        alg = buf_len + fixed_bytes + chars + 8 * (n + 1) * nstr + 5 * n
        # the old route: payloads gathered with an identity index, then unpack_var
        ident = u32(ar)
        gsb = FrameClassifier([(p, 0)]).scratch_bytes(n)
        gscratch = torch.empty(gsb, dtype=torch.uint8, device=dev)
        gathered = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        grec = torch.empty(n + 1, dtype=torch.int64, device=dev)

        def unpack_var():
            p.unpack_var(gathered, total, n, grec, back, boffs, vscratch, vsb, st, stream=s)

        def route():
            FrameClassifier.gather_var(frames, d_o, ident, n, gathered, grec, gscratch, gsb, stream=s)
            unpack_var()

        clear()
        route()
        route_ok = same(dcols, doffs, codes[:n].clone())  # the route gives no codes
        for _ in range(3):
            route()
            new()
        t_new, t_route = [], []
        for _ in range(args.reps):
            t_new.append(ev(new))
            t_route.append(ev(route))
        tu = timeit(unpack_var)
        alg_u = total + fixed_bytes + chars + 8 * (n + 1) * (nstr + 1)
        row("full", alg, t, ok, ab_new=spread(t_new), ab_route=spread(t_route), route_parity_ok=route_ok,
            route_name="gather_var+unpack_var",
            unpack_var_us=round(tu * 1e6, 2), unpack_var_frac=round(alg_u / tu / 8e12, 4))
        del gathered, grec, gscratch
        # 1 % bare `BE32(1) | code 1` frames
        bare = torch.from_numpy(rng.random(n) < 0.01).to(dev)
        m_len = torch.where(bare, torch.full_like(f_len, 5), f_len)
        mixed, m_end = gather_runs(frames, f_off, m_len)
        m_off = m_end - m_len
        at = m_off[bare]
        for k, v in enumerate((0, 0, 0, 1, 1)):
            mixed[at + k] = v
        m_bytes = int(m_end[-1])
        want_cols, want_offs = [], []
        for k, c, o in zip(kinds, dcols, doffs):
            if k == STRING:
                l = torch.where(bare, torch.zeros_like(f_len), o[1:] - o[:n])
                wc, we = gather_runs(c, o[:n], l)
                want_cols.append(wc)
                want_offs.append(torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), we]))
            else:
                want_cols.append(torch.where(bare.repeat_interleave(c.numel() // n), torch.zeros_like(c), c))
                want_offs.append(None)
        d_mo = u32(m_off)
        new_m = lambda: p.unpack_replies_var(mixed, m_bytes, d_mo, n, back, boffs, codes, scratch, sb, st, stream=s)  # noqa: E731
        clear()
        new_m()
        ok = made_ok and same(want_cols, want_offs, bare.to(torch.uint8))
        t = timeit(new_m)
        m_chars = sum(int(o[n]) for o in want_offs if o is not None)
        row("1pct_bare", m_bytes + fixed_bytes + m_chars + 8 * (n + 1) * nstr + 5 * n, t, ok)

    def mixed_case(name, methods, n):
        """n calls over the methods [(method, request schema, reply schema)] in a
        uniformly random order (srpc_frames_mixed_index, _pack_requests_mixed,
        _unpack_replies_mixed).  The request frames' first 4096 are checked
        against the CPU oracle (each plan's calls packed in rank order, the rows
        interleaved by the method vector); the reply stream is made by the same
        pack over the reply plans, checked the same way, and its decode against
        the inputs.  Algorithmic bytes: frames + fields + 1 method byte per
        call, + 1 code byte and 4 offset bytes per call on the reply side; the
        index reads the method bytes and writes its table.  Beside them, timed
        alternately on stream events, the single-plan calls over the same data:
        one srpc_gpu_pack and one indexed srpc_frames_unpack_replies per method
        on per-method streams (no call order, one exchange per method)."""
        if args.only not in name:
            return
        from srpc_amd import MixedFrames, framed_request_prefix, framed_response_prefix
        K = len(methods)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)

        def dcols_of(sch):
            out = []
            for k in sch.kinds:
                c = torch.randint(0, 256, (n * oracle.KIND_SIZE[k],), dtype=torch.uint8, device=dev, generator=gen)
                out.append(c & 1 if k == oracle.BOOL else c)
            return out

        d_method = torch.randint(0, K, (n,), dtype=torch.uint8, device=dev, generator=gen)
        counts = torch.bincount(d_method.to(torch.int64), minlength=K).cpu().numpy()
        req = [GpuPacker(rq, framed_request_prefix(rq, m)) for m, rq, _ in methods]
        rep = [GpuPacker(rs, framed_response_prefix(rs, 0)) for _, _, rs in methods]
        qcols = [dcols_of(rq) for _, rq, _ in methods]
        scols = [dcols_of(rs) for _, _, rs in methods]
        mq, ms = MixedFrames(req), MixedFrames(rep)
        cap = [n] * K
        nb = MixedFrames.index_bytes(n, K)
        d_index = torch.empty(nb, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(8 * (K + 1), dtype=torch.uint8, device=dev)
        st = torch.zeros(16, dtype=torch.uint8, device=dev)

        def index():
            assert MixedFrames.index(d_method, n, K, d_index, nb, d_counts, st, stream=s) == 0

        def first_frames(plans, cols, out, offs, m=4096):
            """out's first m frames against the oracle's, interleaved on the host."""
            hm = d_method[:m].cpu().numpy()
            want = []
            seen = [0] * K
            rows = []
            for p, cs in zip(plans, cols):
                hc = [c[: m * oracle.KIND_SIZE[k]].cpu().numpy().view(oracle.KIND_DTYPE[k]) for c, k in zip(cs, p.schema.kinds)]
                w = oracle.pack(p.schema.kinds, hc, m, p.prefix)
                rows.append(np.frombuffer(w, np.uint8).reshape(m, p.record_bytes))
            for i in range(m):
                want.append(rows[hm[i]][seen[hm[i]]].tobytes())
                seen[hm[i]] += 1
            want = b"".join(want)
            ho = offs[: m + 1].cpu().numpy().view(np.uint32)
            lens = np.array([plans[k].record_bytes for k in hm])
            return (out[: len(want)].cpu().numpy().tobytes() == want
                    and np.array_equal(ho, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)))

        def side(mf, plans, cols):
            fmax = max(p.record_bytes for p in plans)
            out = torch.empty(n * fmax + 16, dtype=torch.uint8, device=dev)
            offs = torch.empty(n + 1, dtype=torch.int32, device=dev)
            fn = lambda: mf.pack(cols, None, cap, d_method, d_index, n, out, n * fmax, offs, st, stream=s)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            total = int(offs[n].item()) & 0xffffffff
            fields = sum(int(c) * p.schema.body_bytes for c, p in zip(counts, plans))
            return out, offs, total, fields, fn

        def ev(fn):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / 1e3

        def alternate(new, route):
            for _ in range(3):
                route()
                new()
            t_new, t_route = [], []
            for _ in range(args.reps):
                t_new.append(ev(new))
                t_route.append(ev(route))
            return {"ab_new": spread(t_new), "ab_route": spread(t_route)}

        def row(mode, alg, t, ok, **extra):
            rows.append({"case": f"{name}_{mode}", "mixed": True, "calls": n, "plans": K, "alg_bytes": alg,
                         "us": round(t * 1e6, 2), "GBps": round(alg / t / 1e9, 1), "frac": round(alg / t / 8e12, 4),
                         "parity_ok": bool(ok), **extra})

        index()
        torch.cuda.synchronize()
        ok = np.array_equal(d_counts.cpu().numpy().view(np.uint64)[:K], counts.astype(np.uint64)) and not bool(st[:4].any())
        row("index", n + nb, timeit(index), ok, index_bytes=nb)
        # requests
        out, offs, total, fields, pack = side(mq, req, qcols)
        ok = first_frames(req, qcols, out, offs) and not bool(st[:4].any())
        wires = [torch.empty(int(c) * p.record_bytes + 16, dtype=torch.uint8, device=dev) for c, p in zip(counts, req)]

        def route_pack():
            for p, cs, c, w in zip(req, qcols, counts, wires):
                p.pack(cs, int(c), w, stream=s)

        row("pack", total + fields + n, timeit(pack), ok, frame_bytes=round(total / n, 1),
            **alternate(lambda: (index(), pack()), route_pack), route_name=f"{K} x srpc_gpu_pack", new_name="index+pack")
        del out, wires
        # replies: the stream, then its decode
        rbuf, roffs, rtotal, rfields, _ = side(ms, rep, scols)
        made_ok = first_frames(rep, scols, rbuf, roffs)
        back = [[torch.empty_like(c) for c in cs] for cs in scols]
        codes = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        for b in back:
            for c in b:
                c.fill_(0xA5)
        codes.fill_(0xA5)

        def decode():
            assert ms.unpack(rbuf, rtotal, roffs, n, d_method, d_index, n, 13, back, None, cap, codes, st, stream=s) == 0

        decode()
        torch.cuda.synchronize()
        ok = made_ok and not bool(st[:4].any()) and not bool(codes[:n].any())
        for k, p in enumerate(rep):
            for a, b, kind in zip(scols[k], back[k], p.schema.kinds):
                used = int(counts[k]) * oracle.KIND_SIZE[kind]
                ok = ok and torch.equal(a[:used], b[:used])
        streams = []
        for p, cs, c in zip(rep, scols, counts):
            w = torch.empty(int(c) * p.record_bytes + 16, dtype=torch.uint8, device=dev)
            p.pack(cs, int(c), w, stream=s)
            o = (torch.arange(int(c), dtype=torch.int64, device=dev) * p.record_bytes).to(torch.int32).contiguous()
            streams.append((w, o))
        rcodes = torch.empty(n + 16, dtype=torch.uint8, device=dev)

        def route_decode():
            for p, b, c, (w, o) in zip(rep, back, counts, streams):
                p.unpack_replies(w, int(c) * p.record_bytes, o, int(c), b, rcodes, st, stream=s)

        row("decode", rtotal + rfields + 6 * n, timeit(decode), ok, frame_bytes=round(rtotal / n, 1),
            **alternate(decode, route_decode), route_name=f"{K} x srpc_frames_unpack_replies (indexed)",
            new_name="decode")

    def requests_case(name, methods, n):
        """Server side: a stream of n request frames over the methods in a
        uniformly random order, classified and decoded into the methods' columns
        in arrival order by one srpc_frames_unpack_requests_mixed.  The stream is
        srpc_frames_pack_requests_mixed's (its first 4096 frames checked against
        the CPU oracle); the decode is checked against the method vector and the
        columns the frames were packed from.  Algorithmic bytes: frames + fields
        + 1 class byte + 4 offset bytes per frame + the index.  Beside it, timed
        alternately on stream events, the bucket route of batch_server:
        srpc_frames_classify, then per method srpc_frames_gather and
        srpc_gpu_unpack (a batch of one method skips the gather, as the server
        does; the route's host sync for the bucket counts is not in its time)."""
        if args.only not in name:
            return
        from srpc_amd import FrameClassifier, MixedFrames, framed_request_prefix
        K = len(methods)
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        d_method = torch.randint(0, K, (n,), dtype=torch.uint8, device=dev, generator=gen)
        counts = torch.bincount(d_method.to(torch.int64), minlength=K).cpu().numpy()
        req = [GpuPacker(rq, framed_request_prefix(rq, m)) for m, rq, _ in methods]
        qcols = []
        for _, rq, _ in methods:
            cs = []
            for k in rq.kinds:
                c = torch.randint(0, 256, (n * oracle.KIND_SIZE[k],), dtype=torch.uint8, device=dev, generator=gen)
                cs.append(c & 1 if k == oracle.BOOL else c)
            qcols.append(cs)
        mq = MixedFrames(req)
        cap = [n] * K
        nb = MixedFrames.index_bytes(n, K)
        d_index = torch.empty(nb, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(8 * (K + 1), dtype=torch.uint8, device=dev)
        st = torch.zeros(16, dtype=torch.uint8, device=dev)
        assert MixedFrames.index(d_method, n, K, d_index, nb, d_counts, st, stream=s) == 0
        fmax = max(p.record_bytes for p in req)
        buf = torch.empty(n * fmax + 16, dtype=torch.uint8, device=dev)
        offs = torch.empty(n + 1, dtype=torch.int32, device=dev)
        assert mq.pack(qcols, None, cap, d_method, d_index, n, buf, n * fmax, offs, st, stream=s) == 0
        torch.cuda.synchronize()
        total = int(offs[n].item()) & 0xffffffff
        # the stream's first 4096 frames against the oracle's, interleaved on the host
        m = min(4096, n)
        hm = d_method[:m].cpu().numpy()
        orows = []
        for p, cs in zip(req, qcols):
            hc = [c[: m * oracle.KIND_SIZE[k]].cpu().numpy().view(oracle.KIND_DTYPE[k]) for c, k in zip(cs, p.schema.kinds)]
            orows.append(np.frombuffer(oracle.pack(p.schema.kinds, hc, m, p.prefix), np.uint8).reshape(m, p.record_bytes))
        seen = [0] * K
        want = []
        for i in range(m):
            want.append(orows[hm[i]][seen[hm[i]]].tobytes())
            seen[hm[i]] += 1
        want = b"".join(want)
        ok = buf[: len(want)].cpu().numpy().tobytes() == want and not bool(st[:4].any())

        back = [[torch.empty_like(c) for c in cs] for cs in qcols]
        cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)

        def clear():
            for b in back:
                for c in b:
                    c.fill_(0xA5)
            cls.fill_(0xA5)

        def same():
            good = torch.equal(cls[:n], d_method)
            for k, p in enumerate(req):
                for a, b, kind in zip(qcols[k], back[k], p.schema.kinds):
                    used = int(counts[k]) * oracle.KIND_SIZE[kind]
                    good = good and torch.equal(a[:used], b[:used])
            return good

        def decode():
            assert mq.unpack_requests(buf, total, offs, n, back, None, cap, cls, d_index, nb, d_counts, st, stream=s) == 0

        clear()
        decode()
        torch.cuda.synchronize()
        ok = ok and same() and not bool(st[:4].any())
        ok = ok and np.array_equal(d_counts.cpu().numpy().view(np.uint64), np.append(counts, 0).astype(np.uint64))

        # the bucket route
        fc = FrameClassifier([(p, 23) for p in req])
        r_cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        r_idx = torch.empty(4 * K * n + 16, dtype=torch.uint8, device=dev)
        r_counts = torch.empty(8 * (K + 2), dtype=torch.uint8, device=dev)
        r_out_off = torch.empty(8 * (n + 1), dtype=torch.uint8, device=dev)
        sb = fc.scratch_bytes(n)
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
        gathered = torch.empty(n * fmax + 16, dtype=torch.uint8, device=dev)

        def route():
            fc.classify(buf, total, offs, n, r_cls, r_idx, r_counts, r_out_off, scratch, sb, stream=s)
            for k, p in enumerate(req):
                c = int(counts[k])
                if not c:
                    continue
                src = buf
                if c != n:
                    FrameClassifier.gather(buf, offs, r_idx.data_ptr() + 4 * k * n, c, p.record_bytes, gathered, stream=s)
                    src = gathered
                p.unpack(src, c * p.record_bytes, c, back[k], stream=s)

        clear()
        route()
        torch.cuda.synchronize()
        route_ok = torch.equal(r_cls[:n], d_method)
        for k, p in enumerate(req):  # the buckets' order is unspecified: the columns as multisets
            for a, b, kind in zip(qcols[k], back[k], p.schema.kinds):
                used = int(counts[k]) * oracle.KIND_SIZE[kind]
                dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[oracle.KIND_SIZE[kind]]
                route_ok = route_ok and torch.equal(a[:used].view(dt).sort().values, b[:used].view(dt).sort().values)

        def ev(fn):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / 1e3

        for _ in range(3):
            route()
            decode()
        t_new, t_route = [], []
        for _ in range(args.reps):
            t_new.append(ev(decode))
            t_route.append(ev(route))
        clear()
        t = timeit(decode)
        torch.cuda.synchronize()
        ok = ok and same()
        fields = sum(int(c) * p.schema.body_bytes for c, p in zip(counts, req))
        alg = total + fields + 5 * n + nb
        rows.append({"case": f"{name}_decode", "mixed": True, "calls": n, "plans": K, "alg_bytes": alg,
                     "us": round(t * 1e6, 2), "GBps": round(alg / t / 1e9, 1), "frac": round(alg / t / 8e12, 4),
                     "parity_ok": bool(ok), "route_parity_ok": bool(route_ok), "frame_bytes": round(total / n, 1),
                     "index_bytes": nb, "ab_new": spread(t_new), "ab_route": spread(t_route),
                     "new_name": "unpack_requests_mixed",
                     "route_name": f"classify + {K if K > 1 else 0} x gather + {K} x srpc_gpu_unpack"})

    def requests_var_case(name, methods, n, maxlen):
        """Server side with string-bodied methods: a stream of n request frames
        over the methods in a uniformly random order, string lengths uniform in
        0..maxlen, classified and decoded into the methods' columns, chars and
        offsets in arrival order by one srpc_frames_unpack_requests_mixed_var.
        The stream is srpc_frames_pack_requests_mixed_var's (its first 4096
        frames checked against the CPU oracle); the decode is checked against the
        method vector and the columns the frames were packed from.  Algorithmic
        bytes: frames + fields + chars + 8 per string offset + 1 class byte + 4
        offset bytes per frame + the index.  Beside it, timed alternately on
        stream events, the bucket route of batch_server: srpc_frames_classify,
        then per string method srpc_frames_gather_var + srpc_gpu_unpack_var, per
        fixed method srpc_frames_gather + srpc_gpu_unpack (the route's host sync
        for the bucket counts is not in its time)."""
        if args.only not in name:
            return
        from srpc_amd import FrameClassifier, MixedFrames, MixedVarFrames, framed_request_prefix
        STRING = oracle.STRING
        K = len(methods)
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        d_method = torch.randint(0, K, (n,), dtype=torch.uint8, device=dev, generator=gen)
        counts = torch.bincount(d_method.to(torch.int64), minlength=K).cpu().numpy()
        var = [STRING in rq.kinds for _, rq, _ in methods]
        req = [GpuPacker.for_request(rq, m) if v else GpuPacker(rq, framed_request_prefix(rq, m))
               for (m, rq, _), v in zip(methods, var)]
        qcols, qoffs, fixed_part = [], [], []
        for k, (_, rq, _) in enumerate(methods):
            c_k = int(counts[k])
            cs, os_ = [], []
            for kind in rq.kinds:
                if kind == STRING:
                    lens = torch.randint(0, maxlen + 1, (c_k,), dtype=torch.int64, device=dev, generator=gen)
                    o = torch.zeros(c_k + 1, dtype=torch.int64, device=dev)
                    o[1:] = torch.cumsum(lens, 0)
                    cs.append(torch.randint(0, 256, (int(o[c_k]) + 16,), dtype=torch.uint8, device=dev, generator=gen))
                    os_.append(o)
                else:
                    c = torch.randint(0, 256, (c_k * oracle.KIND_SIZE[kind] + 16,), dtype=torch.uint8, device=dev,
                                      generator=gen)
                    cs.append(c & 1 if kind == oracle.BOOL else c)
                    os_.append(None)
            qcols.append(cs)
            qoffs.append(os_ if var[k] else None)
            fixed_part.append((4 if var[k] else 0) + len(req[k].prefix) +
                              sum(8 if kind == STRING else oracle.KIND_SIZE[kind] for kind in rq.kinds))
        chars = sum(int(o[-1]) for os_ in qoffs if os_ for o in os_ if o is not None)
        total = sum(int(c) * f for c, f in zip(counts, fixed_part)) + chars
        assert total < 1 << 32, "the stream must stay under 4 GiB"
        mq = MixedVarFrames(req)
        cap = [int(c) for c in counts]
        nb = MixedFrames.index_bytes(n, K)
        d_index = torch.empty(nb, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(8 * (K + 1), dtype=torch.uint8, device=dev)
        st = torch.zeros(16, dtype=torch.uint8, device=dev)
        assert MixedFrames.index(d_method, n, K, d_index, nb, d_counts, st, stream=s) == 0
        sb = mq.scratch_bytes(n)
        scratch = torch.empty(sb + 16, dtype=torch.uint8, device=dev)
        buf = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        offs = torch.empty(n + 1, dtype=torch.int32, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        assert mq.pack(qcols, qoffs, None, cap, d_method, d_index, n, buf, total, offs, d_total, st, scratch, sb,
                       stream=s) == 0
        torch.cuda.synchronize()
        ok = int(d_total[0]) == total and not bool(st[:4].any())
        # the stream's first 4096 frames against the oracle's, interleaved on the host
        m = min(4096, n)
        hm = d_method[:m].cpu().numpy()
        per = []
        for k, (p, cs) in enumerate(zip(req, qcols)):
            mk = int((hm == k).sum())
            kinds = p.schema.kinds
            hc, ho = [], []
            for c, kind, f in zip(cs, kinds, range(len(kinds))):
                if kind == STRING:
                    o = qoffs[k][f][: mk + 1].cpu().numpy().astype(np.uint64)
                    hc.append(c[: max(int(o[mk]), 1)].cpu().numpy())
                    ho.append(o)
                else:
                    hc.append(c[: max(mk, 1) * oracle.KIND_SIZE[kind]].cpu().numpy().view(oracle.KIND_DTYPE[kind])[:mk])
                    ho.append(None)
            body = len(p.prefix) + sum(8 if kind == STRING else oracle.KIND_SIZE[kind] for kind in kinds)
            rec = np.full(mk, body, np.int64)
            for o in ho:
                if o is not None:
                    rec = rec + np.diff(o.astype(np.int64))
            ends = np.concatenate([[0], np.cumsum(rec)])
            w = oracle.pack(kinds, hc, mk, p.prefix, ho if var[k] else None) if mk else b""
            per.append([(int(e - b).to_bytes(4, "big") if var[k] else b"") + w[int(b):int(e)]
                        for b, e in zip(ends[:-1], ends[1:])])
        seen = [0] * K
        want = []
        for i in range(m):
            want.append(per[hm[i]][seen[hm[i]]])
            seen[hm[i]] += 1
        want = b"".join(want)
        ok = ok and buf[: len(want)].cpu().numpy().tobytes() == want

        back = [[torch.empty(total + 16 if kind == STRING else c.numel(), dtype=torch.uint8, device=dev)
                 for c, kind in zip(cs, p.schema.kinds)] for cs, p in zip(qcols, req)]
        boffs = [[torch.empty(int(counts[k]) + 1, dtype=torch.int64, device=dev) if kind == STRING else None
                  for kind in p.schema.kinds] if var[k] else None for k, p in enumerate(req)]
        scap = [[total if kind == STRING else None for kind in p.schema.kinds] if var[k] else None
                for k, p in enumerate(req)]
        nslots = sum(kind == STRING for p in req for kind in p.schema.kinds)
        ends = torch.empty(8 * max(nslots, 1), dtype=torch.uint8, device=dev)
        cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)

        def clear():
            for k, b in enumerate(back):
                for f, c in enumerate(b):
                    (c[: int(qoffs[k][f][-1]) + 16] if var[k] and qoffs[k][f] is not None else c).fill_(0xA5)
            cls.fill_(0xA5)

        def same():
            good = torch.equal(cls[:n], d_method)
            for k, p in enumerate(req):
                for f, kind in enumerate(p.schema.kinds):
                    if kind == STRING:
                        used = int(qoffs[k][f][-1])
                        good = good and torch.equal(boffs[k][f], qoffs[k][f])
                        good = good and torch.equal(back[k][f][:used], qcols[k][f][:used])
                    else:
                        used = int(counts[k]) * oracle.KIND_SIZE[kind]
                        good = good and torch.equal(qcols[k][f][:used], back[k][f][:used])
            return bool(good)

        def decode():
            assert mq.unpack_requests(buf, total, offs, n, back, boffs, scap, None, cap, cls, d_index, nb, d_counts, ends,
                                      st, scratch, sb, stream=s) == 0

        clear()
        decode()
        torch.cuda.synchronize()
        ok = ok and same() and not bool(st[:4].any())
        ok = ok and np.array_equal(d_counts.cpu().numpy().view(np.uint64), np.append(counts, 0).astype(np.uint64))

        # the bucket route
        fc = FrameClassifier([(p, 0 if v else 23) for p, v in zip(req, var)])
        r_cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        r_idx = torch.empty(4 * K * n + 16, dtype=torch.uint8, device=dev)
        r_counts = torch.empty(8 * (K + 2), dtype=torch.uint8, device=dev)
        r_out_off = torch.empty(8 * (n + 1), dtype=torch.uint8, device=dev)
        csb = fc.scratch_bytes(n)
        cscratch = torch.empty(csb, dtype=torch.uint8, device=dev)
        gathered = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        grec = torch.empty(n + 1, dtype=torch.int64, device=dev)
        payload = [int(counts[k]) * (fixed_part[k] - 4) + sum(int(o[-1]) for o in qoffs[k] if o is not None) if var[k] else 0
                   for k in range(K)]
        vsb = max([p.var_scratch_bytes(int(counts[k]), payload[k]) for k, p in enumerate(req) if var[k]])
        vscratch = torch.empty(vsb + 16, dtype=torch.uint8, device=dev)

        def route():
            fc.classify(buf, total, offs, n, r_cls, r_idx, r_counts, r_out_off, cscratch, csb, stream=s)
            for k, p in enumerate(req):
                c = int(counts[k])
                if not c:
                    continue
                idx = r_idx.data_ptr() + 4 * k * n
                if var[k]:
                    FrameClassifier.gather_var(buf, offs, idx, c, gathered, grec, cscratch, csb, stream=s)
                    p.unpack_var(gathered, payload[k], c, grec, back[k], boffs[k], vscratch, vsb, st, stream=s)
                    continue
                src = buf
                if c != n:
                    FrameClassifier.gather(buf, offs, idx, c, p.record_bytes, gathered, stream=s)
                    src = gathered
                p.unpack(src, c * p.record_bytes, c, back[k], stream=s)

        clear()
        route()
        torch.cuda.synchronize()
        route_ok = torch.equal(r_cls[:n], d_method) and not bool(st[:4].any())
        for k, p in enumerate(req):  # the buckets' order is unspecified: lengths and fixed columns as multisets
            for f, kind in enumerate(p.schema.kinds):
                if kind == STRING:
                    a, b = qoffs[k][f], boffs[k][f]
                    route_ok = route_ok and int(b[-1]) == int(a[-1])
                    route_ok = route_ok and torch.equal((a[1:] - a[:-1]).sort().values, (b[1:] - b[:-1]).sort().values)
                else:
                    used = int(counts[k]) * oracle.KIND_SIZE[kind]
                    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[oracle.KIND_SIZE[kind]]
                    route_ok = route_ok and torch.equal(qcols[k][f][:used].view(dt).sort().values,
                                                        back[k][f][:used].view(dt).sort().values)

        def ev(fn):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / 1e3

        for _ in range(3):
            route()
            decode()
        t_new, t_route = [], []
        for _ in range(args.reps):
            t_new.append(ev(decode))
            t_route.append(ev(route))
        clear()
        t = timeit(decode)
        torch.cuda.synchronize()
        ok = ok and same()
        fields = sum(int(c) * sum(oracle.KIND_SIZE[kind] for kind in p.schema.kinds) for c, p in zip(counts, req))
        nstr_total = sum(int(counts[k]) + 1 for k, p in enumerate(req) for kind in p.schema.kinds if kind == STRING)
        alg = total + fields + chars + 8 * nstr_total + 5 * n + nb
        nv = sum(var)
        rows.append({"case": f"{name}_decode", "mixed": True, "calls": n, "plans": K, "alg_bytes": alg,
                     "us": round(t * 1e6, 2), "GBps": round(alg / t / 1e9, 1), "frac": round(alg / t / 8e12, 4),
                     "parity_ok": bool(ok), "route_parity_ok": bool(route_ok), "frame_bytes": round(total / n, 1),
                     "index_bytes": nb, "ab_new": spread(t_new), "ab_route": spread(t_route),
                     "new_name": "unpack_requests_mixed_var",
                     "route_name": f"classify + {nv} x (gather_var + unpack_var) + {K - nv} x (gather + unpack)"})

    def aos_case(name, sch, n, vptr=True):
        """Records as C-aligned structs behind an 8-byte vtable slot (a C++
        std::vector<T> of srpc messages copied to the device; vptr=False: a
        plain struct): srpc_gpu_pack_aos / unpack_aos.  Algorithmic bytes: the
        whole struct array (read by pack, written by unpack) + the wire."""
        if args.only not in name:
            return
        p = GpuPacker(sch)
        fmts = ([np.uint64] if vptr else []) + [np.dtype(oracle.KIND_DTYPE[k]) for k in sch.kinds]
        dt = np.dtype({"names": (["_v"] if vptr else []) + [f"f{i}" for i in range(len(sch.kinds))], "formats": fmts},
                      align=True)
        rng = np.random.default_rng(3)
        recs = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
        for i, k in enumerate(sch.kinds):
            if k == oracle.BOOL:
                recs[f"f{i}"] &= 1
        offs = [dt.fields[f"f{i}"][1] for i in range(len(sch.kinds))]
        drecs = t_u8(recs)
        back = torch.empty_like(drecs)
        wire = torch.empty(n * p.record_bytes + 16, dtype=torch.uint8, device=dev)
        p.pack_aos(drecs, dt.itemsize, offs, n, wire, stream=s)
        torch.cuda.synchronize()
        m = 4096
        ok = wire[: m * p.record_bytes].cpu().numpy().tobytes() == oracle.pack(
            sch.kinds, [np.ascontiguousarray(recs[f"f{i}"][:m]) for i in range(len(sch.kinds))], m)
        alg = n * dt.itemsize + n * p.record_bytes
        tp = timeit(lambda: p.pack_aos(drecs, dt.itemsize, offs, n, wire, stream=s))
        back.copy_(drecs)
        tu = timeit(lambda: p.unpack_aos(wire, n * p.record_bytes, n, back, dt.itemsize, offs, stream=s))
        ok = ok and torch.equal(back, drecs)
        fill_row = {}
        if hasattr(p, "unpack_aos_fill"):
            # into fresh objects (srpc_gpu_unpack_aos_fill): non-field bytes from
            # record 0's image; the fields must equal the source's
            fill = recs[:1].view(np.uint8).tobytes()
            back.zero_()
            tf = timeit(lambda: p.unpack_aos_fill(wire, n * p.record_bytes, n, back, dt.itemsize, offs, fill, stream=s))
            got = back[: m * dt.itemsize].cpu().numpy().view(dt)
            ok = ok and all(np.array_equal(got[f"f{i}"], recs[f"f{i}"][:m]) for i in range(len(sch.kinds)))
            if vptr:
                ok = ok and bool(np.all(got["_v"] == recs["_v"][0]))
            fill_row = {"unpack_fill_us": round(tf * 1e6, 2), "unpack_fill_frac": round(alg / tf / 8e12, 4)}
        rows.append({"case": name, "path": "aos", "records": n, "record_bytes": p.record_bytes,
                     "struct_bytes": dt.itemsize, "alg_bytes": alg, "pack_us": round(tp * 1e6, 2),
                     "unpack_us": round(tu * 1e6, 2), "pack_GBps": round(alg / tp / 1e9, 1),
                     "unpack_GBps": round(alg / tu / 1e9, 1), "pack_frac": round(alg / tp / 8e12, 4),
                     "unpack_frac": round(alg / tu / 8e12, 4), "parity_ok": bool(ok), **fill_row})

    def var_case(name, kinds, n, maxlen, prefix=b""):
        if args.only not in name:
            return
        sch = Schema("V", tuple((f"f{i}", k) for i, k in enumerate(kinds)))
        p = GpuPacker(sch, prefix)
        rng = np.random.default_rng(2)
        cols, offs = [], []
        for k in kinds:
            if k == oracle.STRING:
                lens = rng.integers(0, maxlen + 1, n).astype(np.uint64)
                o = np.zeros(n + 1, np.uint64)
                o[1:] = np.cumsum(lens)
                cols.append(rng.integers(0, 256, int(o[-1]) + 1, dtype=np.uint8))
                offs.append(o)
            else:
                dt = np.dtype(oracle.KIND_DTYPE[k])
                cols.append(rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt))
                offs.append(None)
        fixed = len(prefix) + sum(8 if k == oracle.STRING else oracle.KIND_SIZE[k] for k in kinds)
        total = n * fixed + int(sum(int(o[-1]) for o in offs if o is not None))
        dcols = [t_u8(c) for c in cols]
        doffs = [t_u8(o) if o is not None else None for o in offs]
        wire = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        rec = torch.empty(8 * (n + 1), dtype=torch.uint8, device=dev)
        sb = p.var_scratch_bytes(n, total)
        scratch = torch.empty(sb + 16, dtype=torch.uint8, device=dev)
        outs = [torch.empty(total + 16 if k == oracle.STRING else n * oracle.KIND_SIZE[k] + 16,
                            dtype=torch.uint8, device=dev) for k in kinds]
        ooffs = [torch.empty(8 * (n + 1), dtype=torch.uint8, device=dev) if k == oracle.STRING else None
                 for k in kinds]
        want = oracle.pack(kinds, cols, n, prefix, list(offs))
        col_bytes = sum(c.nbytes for c, k in zip(cols, kinds) if k != oracle.STRING)
        str_bytes = total - n * fixed
        alg = col_bytes + str_bytes + 8 * (n + 1) * sum(k == oracle.STRING for k in kinds) + total
        if args.var_caps:
            ib, cb = (int(x) for x in args.var_caps.split(":"))
            p.tune(var_image_bytes=ib, var_chars_bytes=cb)
        kernels = [int(k) for k in args.var_kernel.split(",") if k] or [None]
        for vk in kernels:
            label = name if vk is None else f"{name}_k{vk}"
            if vk is not None:
                p.tune(var_kernel=vk)
            wire.fill_(0)
            p.pack_var(dcols, doffs, n, wire, total, rec, scratch, sb, stream=s)
            torch.cuda.synchronize()
            ok = wire[:total].cpu().numpy().tobytes() == want
            tp = timeit(lambda: p.pack_var(dcols, doffs, n, wire, total, rec, scratch, sb, stream=s))
            tu = timeit(lambda: p.unpack_var(wire, total, n, rec, outs, ooffs, scratch, sb, stream=s))
            row = {"case": label, "path": "var", "records": n, "wire_bytes": total, "alg_bytes": alg,
                   "pack_us": round(tp * 1e6, 2), "unpack_us": round(tu * 1e6, 2),
                   "pack_GBps": round(alg / tp / 1e9, 1), "unpack_GBps": round(alg / tu / 1e9, 1),
                   "pack_frac": round(alg / tp / 8e12, 4), "unpack_frac": round(alg / tu / 8e12, 4),
                   "parity_ok": bool(ok)}
            if sum(k == oracle.STRING for k in kinds) > 1:
                # several string fields: the unpack with the batch's tile table
                # (srpc_gpu_unpack_var_tiled, ABI 6; the table from the pack's
                # own input offsets), checked against the look-back unpack
                tw = p.var_tile_table_words(n)
                table = torch.empty(8 * tw + 16, dtype=torch.uint8, device=dev)
                p.var_tile_table(doffs, n, table, stream=s)
                p.unpack_var(wire, total, n, rec, outs, ooffs, scratch, sb, stream=s)
                torch.cuda.synchronize()
                ref = [o.clone() for o in outs], [o.clone() if o is not None else None for o in ooffs]
                for o in outs:
                    o.fill_(0)
                tt = timeit(lambda: p.unpack_var_tiled(wire, total, n, rec, table, outs, ooffs, scratch, sb,
                                                       stream=s))
                torch.cuda.synchronize()
                # the bytes the batch owns (the columns' slack is nobody's)
                same = True
                for k, a_, b_, oa, ob in zip(kinds, outs, ref[0], ooffs, ref[1]):
                    if k == oracle.STRING:
                        same = same and torch.equal(oa, ob)
                        used = int(ob[-8:].cpu().numpy().view(np.uint64)[0]) if n else 0
                    else:
                        used = n * oracle.KIND_SIZE[k]
                    same = same and torch.equal(a_[:used], b_[:used])
                row["tiled_ok"] = bool(same)
                row["parity_ok"] = row["parity_ok"] and same
                row.update({"unpack_tiled_us": round(tt * 1e6, 2), "unpack_tiled_frac": round(alg / tt / 8e12, 4)})
            if args.stream:
                # the same wire decoded with NO record index (srpc_gpu_unpack_var_stream),
                # the index rebuilt on the device and written out (8 B per record more)
                ssb = p.var_stream_scratch_bytes(n, total)
                sscr = torch.empty(ssb + 256, dtype=torch.uint8, device=dev)
                sbase = sscr.data_ptr() + (-sscr.data_ptr()) % 256
                rec2 = torch.empty(8 * (n + 1), dtype=torch.uint8, device=dev)
                ts = timeit(lambda: p.unpack_var_stream(wire, total, n, rec2, outs, ooffs, sbase, ssb, stream=s))
                torch.cuda.synchronize()
                row["stream_ok"] = bool(torch.equal(rec2, rec))
                row["parity_ok"] = row["parity_ok"] and row["stream_ok"]
                salg = alg + 8 * (n + 1)
                row.update({"stream_us": round(ts * 1e6, 2), "stream_frac": round(salg / ts / 8e12, 4)})
            rows.append(row)

    N = 1 << 24
    fixed_case("quad_dword_16M", QUAD, N)
    fixed_case("quad_tile_16M", QUAD, N, path=srpc_amd.SRPC_PATH_TILE)
    fixed_case("number_body_16M", NUMBER, N)
    fixed_case("all_kinds_17B_16M", Schema.of("all_kinds", ("a", "bool"), ("b", "int8"), ("c", "char"),
                                              ("d", "int16"), ("e", "int32"), ("f", "int64")), N)
    fixed_case("square_request_53B_16M", NUMBER, N, srpc_amd.request_prefix(SQUARE_METHOD, "Number"))
    fixed_case("square_response_19B_16M", NUMBER, N, srpc_amd.response_prefix(0, "Number"))
    two = Schema.of("TwoNumbers", ("left", "int32"), ("right", "int32"))
    fixed_case("add_request_58B_16M", two, N, srpc_amd.request_prefix("Calculator_servicer::add", "TwoNumbers"))
    fixed_case("subtract_request_63B_16M", two, N,
               srpc_amd.request_prefix("Calculator_servicer::subtract", "TwoNumbers"))
    fixed_case("two_numbers_response_23B_16M", two, N, srpc_amd.response_prefix(0, "TwoNumbers"))
    replies_case("number_replies_23B_16M", NUMBER, N)
    replies_case("all_kinds_replies_39B_16M", Schema.of("all_kinds", ("a", "bool"), ("b", "int8"), ("c", "char"),
                                                        ("d", "int16"), ("e", "int32"), ("f", "int64")), N)
    NV = args.replies_var_frames
    tag = "16M" if NV == 1 << 24 else str(NV)
    replies_var_case(f"replies_var_text_0-64_{tag}", Schema.of("Text", ("text", "string")), NV, 64)
    replies_var_case(f"replies_var_multiple_primitives_0-40_{tag}",
                     Schema.of("multiple_primitives", ("arg1", "int8"), ("arg2", "char"), ("arg3", "int64"),
                               ("arg4", "string")), NV, 40)
    NM = args.mixed_calls
    mtag = "16M" if NM == 1 << 24 else str(NM)
    svc = "Calculator_servicer::"
    mixed_case(f"mixed_k1_square_{mtag}", [(SQUARE_METHOD, NUMBER, NUMBER)], NM)
    mixed_case(f"mixed_k4_calculator_{mtag}", [(SQUARE_METHOD, NUMBER, NUMBER), (svc + "add", two, NUMBER),
                                               (svc + "subtract", two, NUMBER), (svc + "multiply", two, NUMBER)], NM)
    requests_case(f"requests_k1_square_{mtag}", [(SQUARE_METHOD, NUMBER, NUMBER)], NM)
    requests_case(f"requests_k4_calculator_{mtag}", [(SQUARE_METHOD, NUMBER, NUMBER), (svc + "add", two, NUMBER),
                                                     (svc + "subtract", two, NUMBER), (svc + "multiply", two, NUMBER)], NM)
    mp = Schema.of("multiple_primitives", ("arg1", "int8"), ("arg2", "char"), ("arg3", "int64"), ("arg4", "string"))
    echo = ("Echo_servicer::echo", mp, mp)
    calc = [(SQUARE_METHOD, NUMBER, NUMBER), (svc + "add", two, NUMBER), (svc + "subtract", two, NUMBER),
            (svc + "multiply", two, NUMBER)]
    for maxlen in (16, 300):
        requests_var_case(f"requests_var_k1_echo_0-{maxlen}_{mtag}", [echo], NM, maxlen)
        requests_var_case(f"requests_var_k5_calculator_echo_0-{maxlen}_{mtag}", calc + [echo], NM, maxlen)
    aos_case("quad_aos_16M", QUAD, N)
    aos_case("quad_aos_plain_16M", QUAD, N, vptr=False)
    aos_case("all_kinds_aos_16M", Schema.of("all_kinds", ("a", "bool"), ("b", "int8"), ("c", "char"),
                                            ("d", "int16"), ("e", "int32"), ("f", "int64")), N)
    var_case("multiple_primitives_str0-64_4M", [oracle.INT8, oracle.CHAR, oracle.INT64, oracle.STRING],
             1 << 22, 64)
    var_case("string_0-1024_1M", [oracle.STRING], 1 << 20, 1024)
    var_case("string_0-16_8M", [oracle.STRING], 1 << 23, 16)
    var_case("string_0-32_4M", [oracle.STRING], 1 << 22, 32)
    var_case("two_str_request_0-32_4M", [oracle.STRING, oracle.INT32, oracle.STRING], 1 << 22, 32,
             srpc_amd.request_prefix("Svc_servicer::method", "TwoStr"))
    txt = json.dumps(rows, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)
    for r in rows:
        if r.get("mixed"):
            extra = ""
            if "ab_new" in r:
                extra = (f'  events: {r["new_name"]} {r["ab_new"]["median_us"]:.1f} us [{r["ab_new"]["min_us"]:.1f}, '
                         f'{r["ab_new"]["max_us"]:.1f}]  {r["route_name"]} {r["ab_route"]["median_us"]:.1f} us '
                         f'[{r["ab_route"]["min_us"]:.1f}, {r["ab_route"]["max_us"]:.1f}]')
            print(f'{r["case"]:36s} mixed {r["us"]:9.1f} us {r["GBps"]:7.1f} GB/s ({r["frac"]:.3f})  '
                  f'parity={r["parity_ok"]}{extra}')
            continue
        if r.get("replies"):
            extra = ""
            if "unpack_us" in r:
                extra += (f'  srpc_gpu_unpack {r["unpack_us"]:9.1f} us ({r["unpack_frac"]:.3f})'
                          f'  time/byte vs unpack {r["time_per_byte_vs_unpack"]:.3f}')
            if "ab_new" in r:
                extra += (f'  events: new {r["ab_new"]["median_us"]:.1f} us [{r["ab_new"]["min_us"]:.1f}, '
                          f'{r["ab_new"]["max_us"]:.1f}]  {r.get("route_name", "classify+gather+unpack")} '
                          f'{r["ab_route"]["median_us"]:.1f} us '
                          f'[{r["ab_route"]["min_us"]:.1f}, {r["ab_route"]["max_us"]:.1f}]')
            if "unpack_var_us" in r:
                extra += (f'  route parity={r["route_parity_ok"]}  srpc_gpu_unpack_var alone {r["unpack_var_us"]:.1f} us '
                          f'({r["unpack_var_frac"]:.3f})')
            print(f'{r["case"]:44s} replies {r["us"]:9.1f} us {r["GBps"]:7.1f} GB/s ({r["frac"]:.3f})  '
                  f'parity={r["parity_ok"]}{extra}')
            continue
        extra = f'  stream {r["stream_us"]:8.1f} us ({r["stream_frac"]:.3f})' if "stream_us" in r else ""
        for k in ("tiled_ok", "stream_ok"):
            if k in r and not r[k]:
                extra += f"  {k}=False"
        if "unpack_tiled_us" in r:
            extra += f'  unpack_tiled {r["unpack_tiled_us"]:8.1f} us ({r["unpack_tiled_frac"]:.3f})'
        if "unpack_fill_us" in r:
            extra += f'  unpack_fill {r["unpack_fill_us"]:8.1f} us ({r["unpack_fill_frac"]:.3f})'
        if "generic_pack_frac" in r:
            extra += (f'  generic ({r["generic_pack_frac"]:.3f} / {r["generic_unpack_frac"]:.3f})'
                      f'  rec ({r["rec_pack_frac"]:.3f} / {r["rec_unpack_frac"]:.3f})')
        print(f'{r["case"]:34s} {r["path"]:5s} pack {r["pack_us"]:9.1f} us {r["pack_GBps"]:7.1f} GB/s '
              f'({r["pack_frac"]:.3f})  unpack {r["unpack_us"]:9.1f} us {r["unpack_GBps"]:7.1f} GB/s '
              f'({r["unpack_frac"]:.3f})  parity={r["parity_ok"]}{extra}')


if __name__ == "__main__":
    main()
