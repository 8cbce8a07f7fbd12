#!/usr/bin/env python3
"""A/B sweep of DWORD-path variants on the bench workload (16M Quad records).

Interleaved rounds in ONE process (cdna_hip_programming.md §5.4 rule 24):
every variant is timed once per round, rounds repeat, and the median and min
per variant are reported.  Each pack/unpack is timed on the kernel clock of
srpc_time_next_call (dispatch begin/end); the torch copy by events around it.  "cold" rounds write a 1 GiB scratch buffer before each
timed kernel so the 256 MiB Infinity Cache holds none of its inputs.

Known-good reference on the same device: torch's device-to-device copy of the
same 512 MiB (256 MiB read + 256 MiB write), i.e. the chip's copy ceiling for
this byte count.

    python tools/sweep.py [--records N] [--rounds R] [--out gpurun_out/sweep.json]

Two further modes look at SRPC_TUNE_SWEEP (which way pack and unpack walk the
records), whose gain exists only for the producer/consumer pair:

    python tools/sweep.py --mode pair --schema quad,number,two --records 16777216,67108864
        sweep 0..3 alternated per round; every timed item is `pack; unpack`
        back to back, both calls armed, the pair's time running from pack's
        dispatch begin to unpack's dispatch end; beside it an uninstrumented
        step clock (K steps between two events, bench.py's).
    python tools/sweep.py --mode window
        after a full ascending pack, a descending unpack of only the top
        x MiB of the wire (a pointer-shifted call), warm and after a 512 MiB
        flush, in us per MiB: where the two curves meet is how much of pack's
        tail the Infinity Cache still holds.

Both print their rows and, like the variant sweep, write JSON where --out says.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="variants", choices=["variants", "pair", "window"])
    ap.add_argument("--records", default=str(1 << 24), help="records (pair mode: comma list)")
    ap.add_argument("--rounds", type=int, default=None, help="default 7 (pair and window: 9)")
    ap.add_argument("--schema", default="quad", help="quad, number or two (pair mode: comma list)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="", help="comma list of workgroup caps to sweep (0 = full grid)")
    ap.add_argument("--base", default="1,1,3", help="rpl,iter,nt for the --grids sweep")
    ap.add_argument("--reps", type=int, default=5, help="pair: timed pairs per setting per round")
    ap.add_argument("--steps", type=int, default=20, help="pair: steps of the uninstrumented step clock")
    ap.add_argument("--nontemporal", default="", help="pair, window: comma list of SRPC_TUNE_NONTEMPORAL values "
                                                      "to run beside the plan's default (P:U = pack P, unpack U)")
    ap.add_argument("--slices", default="32,64,96,128,192,256", help="window: MiB of wire below its end")
    args = ap.parse_args()
    schemas = args.schema.split(",")
    records = [int(x) for x in args.records.split(",")]
    if any(x not in SCHEMAS for x in schemas) or (args.mode != "pair" and len(schemas) * len(records) != 1):
        ap.error("--schema: quad, number or two; several values of --schema / --records in pair mode only")
    nts = [None] + [x for x in args.nontemporal.split(",") if x]  # "3", or "2:3" = pack 2, unpack 3
    if args.rounds is None:
        args.rounds = 7 if args.mode == "variants" else 9
    if args.mode == "pair":
        return write(args,
                     {"mode": "pair", "rounds": args.rounds, "reps": args.reps, "steps": args.steps,
                      "cases": [pair_ab(s, n, nt, args) for s in schemas for n in records for nt in nts]})
    if args.mode == "window":
        return write(args,
                     {"mode": "window", "rounds": args.rounds,
                      "cases": [window(schemas[0], records[0], nt, args) for nt in nts]})
    args.schema, args.records = schemas[0], records[0]

    import torch

    import srpc_amd
    from srpc_amd import NUMBER, QUAD, TWO_NUMBERS, GpuPacker

    sch = {"quad": QUAD, "number": NUMBER, "two": TWO_NUMBERS}[args.schema]
    F = len(sch.kinds)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    n = args.records
    cols = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(F)]
    back = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(F)]
    wire = torch.empty(n * 4 * F, dtype=torch.uint8, device=dev)
    srpc_amd.fill_splitmix_i32(cols, n, 0x5EED, 0, s)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    copy_src = torch.empty(n * 4 * F, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    p = GpuPacker(sch)

    if args.grids:
        base = [int(x) for x in args.base.split(",")]
        variants = [("dword", base[0], base[1], base[2], g) for g in [int(x) for x in args.grids.split(",")]]
    else:
        variants = [("dword", rpl, it, nt, 0)
                    for rpl, it, nt in itertools.product((1, 4), (1, 2, 4, 8), (0, 1, 2, 3))]
        variants.append(("tile", 0, 0, 0, 0))
    alg = 2 * 4 * F * n  # bytes per kernel: read F*4 + write F*4 per record

    def timed(fn, cold, hook=True):
        if cold:
            flush.fill_(1)
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(s)
        if hook:  # kernel clock (srpc_time_next_call) restamps a and b
            b.record(s)
            srpc_amd.time_next_call(a, b)
        fn()
        if not hook:
            b.record(s)
        return a, b

    res = {}
    for _ in range(2):  # warm-up every variant
        for v in variants:
            set_variant(p, v, srpc_amd)
            p.pack(cols, n, wire, stream=s)
            p.unpack(wire, wire.numel(), n, back, stream=s)
    torch.cuda.synchronize()
    ok = all(torch.equal(x, y) for x, y in zip(cols, back))
    for rnd in range(args.rounds):
        for cold in (False, True):
            evs = []
            for v in variants:
                set_variant(p, v, srpc_amd)
                evs.append((v, "pack", timed(lambda: p.pack(cols, n, wire, stream=s), cold)))
                evs.append((v, "unpack", timed(lambda: p.unpack(wire, wire.numel(), n, back, stream=s), cold)))
            evs.append((("copy",), "d2d", timed(lambda: copy_dst.copy_(copy_src), cold, hook=False)))
            torch.cuda.synchronize()
            for v, k, (a, b) in evs:
                res.setdefault((v, k, cold), []).append(a.elapsed_time(b))
    out = {"records": n, "schema": sch.name, "alg_bytes_per_kernel": alg, "roundtrip_ok": ok,
           "rows": []}
    for (v, k, cold), ts in sorted(res.items(), key=lambda kv: (kv[0][2], kv[0][1], statistics.median(kv[1]))):
        med, mn = statistics.median(ts), min(ts)
        out["rows"].append({"variant": "/".join(map(str, v)), "kernel": k, "cold": cold,
                            "median_us": round(med * 1e3, 2), "min_us": round(mn * 1e3, 2),
                            "GBps_median": round(alg / (med / 1e3) / 1e9, 1),
                            "frac_of_8TBps": round(alg / (med / 1e3) / 8e12, 4)})
    txt = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)
    for r in out["rows"]:
        print(f'{"cold" if r["cold"] else "warm"} {r["kernel"]:6s} {r["variant"]:16s} '
              f'med {r["median_us"]:8.2f} us  min {r["min_us"]:8.2f} us  {r["GBps_median"]:8.1f} GB/s  '
              f'{r["frac_of_8TBps"]:.3f}')


SCHEMAS = ("quad", "number", "two")


def write(args, out):
    if not args.out:
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


def setup(schema, n):
    """Columns, their unpacked copy, the wire and a plan for n records."""
    import torch

    import srpc_amd
    from srpc_amd import NUMBER, QUAD, TWO_NUMBERS, GpuPacker

    sch = {"quad": QUAD, "number": NUMBER, "two": TWO_NUMBERS}[schema]
    F = len(sch.kinds)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    cols = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(F)]
    back = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(F)]
    wire = torch.empty(n * 4 * F, dtype=torch.uint8, device=dev)
    srpc_amd.fill_splitmix_i32(cols, n, 0x5EED, 0, s)
    return torch, srpc_amd, GpuPacker(sch), F, s, cols, back, wire


def events(torch, s, k):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(k)]
    for e in ev:
        e.record(s)  # torch creates the HIP event on its first record
    return ev


def med_min(ts):
    return {"median_us": round(statistics.median(ts) * 1e3, 2), "min_us": round(min(ts) * 1e3, 2)}


def pair_ab(schema, n, nt, args):
    """sweep 0..3 alternated per round; per setting one untimed pair (the
    caches then hold what the same setting left), `reps` armed pairs and the
    step clock over `steps` unarmed steps."""
    torch, srpc_amd, p, F, s, cols, back, wire = setup(schema, n)
    if nt is not None:
        p.tune(nontemporal=int(nt.split(":")[0]), unpack_nontemporal=int(nt.split(":")[-1]))
    wl = wire.numel()

    def step():
        p.pack(cols, n, wire, stream=s)
        p.unpack(wire, wl, n, back, stream=s)

    for sw in range(4):
        p.tune(sweep=sw)
        step()
    torch.cuda.synchronize()
    ok = all(torch.equal(x, y) for x, y in zip(cols, back))
    res = {sw: {"pair": [], "pack": [], "unpack": [], "step": []} for sw in range(4)}
    for _ in range(args.rounds):
        for sw in range(4):
            p.tune(sweep=sw)
            step()
            ev = [events(torch, s, 4) for _ in range(args.reps)]
            for a, b, c, d in ev:
                srpc_amd.time_next_call(a, b)
                p.pack(cols, n, wire, stream=s)
                srpc_amd.time_next_call(c, d)
                p.unpack(wire, wl, n, back, stream=s)
            t0, t1 = events(torch, s, 2)
            t0.record(s)
            for _ in range(args.steps):
                step()
            t1.record(s)
            torch.cuda.synchronize()
            for a, b, c, d in ev:
                res[sw]["pair"].append(a.elapsed_time(d))
                res[sw]["pack"].append(a.elapsed_time(b))
                res[sw]["unpack"].append(c.elapsed_time(d))
            res[sw]["step"].append(t0.elapsed_time(t1) / args.steps)
    out = {"schema": schema, "records": n, "nontemporal": "default" if nt is None else nt, "roundtrip_ok": ok,
           "wire_MiB": wl / 2**20, "sweep": {str(sw): {k: med_min(v) for k, v in r.items()} for sw, r in res.items()}}
    for sw, r in out["sweep"].items():
        print(f'{schema:6s} n={n} nt={out["nontemporal"]} sweep={sw} ' +
              "  ".join(f'{k} {v["median_us"]:8.2f}/{v["min_us"]:8.2f}' for k, v in r.items()) + "  us (median/min)")
    del cols, back, wire
    torch.cuda.empty_cache()
    return out


def window(schema, n, nt, args):
    """Full ascending pack, then a descending unpack of the top x MiB of the
    wire only: straight after the pack, and with 512 MiB written in between."""
    torch, srpc_amd, p, F, s, cols, back, wire = setup(schema, n)
    if nt is not None:
        p.tune(nontemporal=int(nt.split(":")[0]), unpack_nontemporal=int(nt.split(":")[-1]))
    stride = 4 * F
    wl = wire.numel()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=wire.device)
    slices = [x for x in (int(v) for v in args.slices.split(",")) if (x << 20) <= wl]
    res = {(x, c): [] for x in slices for c in (False, True)}
    for rnd in range(args.rounds + 1):  # round 0 warms up
        evs = []
        for x in slices:
            k = (x << 20) // stride      # records in the slice
            r0 = n - k                   # ... which starts at record r0
            for cold in (False, True):
                a, b = events(torch, s, 2)
                p.tune(sweep=0)
                p.pack(cols, n, wire, stream=s)
                if cold:
                    flush.fill_(rnd & 0xFF)
                p.tune(sweep=2)
                srpc_amd.time_next_call(a, b)
                p.unpack(wire[r0 * stride:], k * stride, k, [c[r0:] for c in back], stream=s)
                evs.append((x, cold, a, b))
        torch.cuda.synchronize()
        if rnd:
            for x, cold, a, b in evs:
                res[(x, cold)].append(a.elapsed_time(b))
    ok = all(torch.equal(c[n - ((slices[-1] << 20) // stride):], b[n - ((slices[-1] << 20) // stride):])
             for c, b in zip(cols, back))
    rows, prev = [], None
    for x in slices:
        w, c = statistics.median(res[(x, False)]) * 1e3, statistics.median(res[(x, True)]) * 1e3
        row = {"slice_MiB": x, "warm_us": round(w, 2), "cold_us": round(c, 2),
               "warm_us_per_MiB": round(w / x, 4), "cold_us_per_MiB": round(c / x, 4),
               "warm_min_us": round(min(res[(x, False)]) * 1e3, 2), "cold_min_us": round(min(res[(x, True)]) * 1e3, 2)}
        if prev:  # the cost of the MiB added since the previous slice
            row["warm_marginal_us_per_MiB"] = round((w - prev[1]) / (x - prev[0]), 4)
            row["cold_marginal_us_per_MiB"] = round((c - prev[2]) / (x - prev[0]), 4)
        prev = (x, w, c)
        rows.append(row)
        print(f'{schema} nt={"default" if nt is None else nt} top {x:4d} MiB: warm {w:7.2f} us  cold {c:7.2f} us  ' +
              f'{row["warm_us_per_MiB"]:.4f} / {row["cold_us_per_MiB"]:.4f} us per MiB' +
              (f'  marginal {row["warm_marginal_us_per_MiB"]:.4f} / {row["cold_marginal_us_per_MiB"]:.4f}'
               if "warm_marginal_us_per_MiB" in row else ""))
    del cols, back, wire, flush
    torch.cuda.empty_cache()
    return {"schema": schema, "records": n, "nontemporal": "default" if nt is None else nt, "slices_ok": ok,
            "wire_MiB": wl / 2**20, "rows": rows}


def set_variant(p, v, srpc_amd):
    if v[0] == "tile":
        p.force_path(srpc_amd.SRPC_PATH_TILE)
    else:
        p.force_path(srpc_amd.SRPC_PATH_DWORD)
        p.tune(v[1], v[2], v[3], grid=v[4])


if __name__ == "__main__":
    main()
