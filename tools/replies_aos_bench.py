"""Kernel-clock time of the reply decode into structs
(srpc_frames_unpack_replies_aos) beside the three calls that bracket it, on one
all-full uniform stream of `--calls` all_kinds replies (39-byte frames) and the
natural 32-byte struct behind a vtable slot:

  (a) srpc_frames_unpack_replies_aos    frames -> structs + codes
  (b) srpc_gpu_unpack_aos_fill          the same plan, bytes in and struct bytes
                                        out; no codes, no per-frame judgement
  (c) srpc_frames_unpack_replies        frames -> columns + codes
  (d) srpc_gpu_unpack                   the same plan -> columns

Every figure is srpc_time_next_call's interval, the four calls interleaved in
each of `--reps` rounds after one warm-up round; medians and every sample are
printed.  (c)/(d) is what judging every frame costs the column form; the
yardstick for (a) is (b) * (c)/(d) * 1.1.  The fraction of 8 TB/s counts the
algorithmic bytes of (a) once each: nframes * (F + stride + 1).

    python tools/replies_aos_bench.py [--calls 4000000] [--reps 10]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from srpc_amd import GpuPacker, Schema, framed_response_prefix, time_next_call  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8e12  # bytes/s, MI355X HBM3E
ALL_KINDS = Schema.of("all_kinds", ("k_bool", "bool"), ("k_i8", "int8"), ("k_char", "char"),
                      ("k_i16", "int16"), ("k_i32", "int32"), ("k_i64", "int64"))
SIZES = [1, 1, 1, 2, 4, 8]
STRIDE, OFFSETS = 32, (8, 9, 10, 12, 16, 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    n = a.calls
    p = GpuPacker(ALL_KINDS, framed_response_prefix(ALL_KINDS, 0))
    F = p.record_bytes
    g = torch.Generator(device=DEV).manual_seed(1)
    src = [torch.randint(0, 2 if i == 0 else 256, (n * s,), dtype=torch.uint8, device=DEV, generator=g)
           for i, s in enumerate(SIZES)]
    buf = torch.zeros(n * F + 16, dtype=torch.uint8, device=DEV)
    p.pack(src, n, buf)
    cols = [torch.zeros(n * s + 16, dtype=torch.uint8, device=DEV) for s in SIZES]
    recs = torch.zeros(n * STRIDE + 16, dtype=torch.uint8, device=DEV)
    codes = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    st = torch.zeros(16, dtype=torch.uint8, device=DEV)
    fill = np.random.default_rng(2).integers(0, 256, STRIDE, dtype=np.uint8).tobytes()
    calls = {
        "a replies_aos": lambda: p.unpack_replies_aos(buf, n * F, None, n, recs, STRIDE, OFFSETS, fill, codes, st),
        "b unpack_aos_fill": lambda: p.unpack_aos_fill(buf, n * F, n, recs, STRIDE, OFFSETS, fill, st),
        "c replies (columns)": lambda: p.unpack_replies(buf, n * F, None, n, cols, codes, st),
        "d unpack (columns)": lambda: p.unpack(buf, n * F, n, cols, st),
    }
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s), e1.record(s)
    torch.cuda.synchronize()
    samples = {k: [] for k in calls}
    for r in range(a.reps + 1):
        for k, fn in calls.items():
            time_next_call(e0, e1)
            rc = fn()
            torch.cuda.synchronize()
            assert rc == 0 and not st[:4].any(), (k, rc)
            if r:
                samples[k].append(e0.elapsed_time(e1) * 1e3)  # us
    # (a) and (b) leave the same structs; (a)'s codes are the frames' (all 0)
    calls["b unpack_aos_fill"]()
    want = recs.clone()
    recs.zero_()
    calls["a replies_aos"]()
    torch.cuda.synchronize()
    assert torch.equal(recs[:n * STRIDE], want[:n * STRIDE]) and not codes[:n].any()
    print(f"calls {n} frame bytes {F} struct bytes {STRIDE} reps {a.reps} frames per tile {p.replies_aos_per_tile(STRIDE)}")
    med = {}
    for k, v in samples.items():
        med[k] = statistics.median(v)
        print(f"{k:22s} median {med[k]:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  samples "
              + " ".join(f"{x:.1f}" for x in v))
    ma, mb, mc, md = (med[k] for k in calls)
    alg = n * (F + STRIDE + 1)
    print(f"(c)/(d) = {mc / md:.3f}   (a)/(b) = {ma / mb:.3f}   yardstick (b)*(c)/(d)*1.1 = {mb * mc / md * 1.1:.1f} us"
          f"   (a) {'within' if ma <= mb * mc / md * 1.1 else 'MISSES'} it")
    print(f"(a) algorithmic bytes {alg} -> {alg / (ma * 1e-6) / 1e12:.2f} TB/s = {alg / (ma * 1e-6) / PEAK:.3f} of 8 TB/s")


if __name__ == "__main__":
    main()
