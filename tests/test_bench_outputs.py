"""bench.py's plain run and `--dump-outputs DIR`: which records a dump keeps
(decided without a GPU), and one real run on cuda:0 whose dumped wire bytes
and columns are checked against the CPU oracle and whose result line holds the
headline and none of the `--full` objects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import oracle  # noqa: E402

FULL_ONLY = ("verify", "kernels_ms", "kernels_ms_cold", "roofline", "strong_scaling", "pcie_inclusive",
             "cpu_baseline", "per_rank")


def test_dump_records_small_batch_keeps_every_record():
    n = 2 * bench.DUMP_EDGE + bench.DUMP_SAMPLE
    assert np.array_equal(bench.dump_records(n), np.arange(n))
    assert bench.dump_records(1).tolist() == [0]


def test_dump_records_large_batch_is_a_fixed_sample_with_both_ends():
    n = 1 << 24
    a, b = bench.dump_records(n), bench.dump_records(n)
    assert np.array_equal(a, b)  # same arguments, same records
    assert a.dtype == np.int64 and np.all(np.diff(a) > 0) and a[0] == 0 and a[-1] == n - 1
    e = bench.DUMP_EDGE
    assert np.array_equal(a[:e], np.arange(e)) and np.array_equal(a[-e:], np.arange(n - e, n))
    assert 2 * e + bench.DUMP_SAMPLE // 2 < a.size <= 2 * e + bench.DUMP_SAMPLE
    # records.npy + wire.npy (float32 x 16) + four float64 columns: within 64 MB
    assert a.size * (8 + 4 * bench.REC_BYTES + 4 * 8) <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_step_computed(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, steps = 100003, 3  # odd, several blocks; small enough that every record is kept
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--records", str(n), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["ms_per_step"] > 0
    # value is the wire GiB/s of one step of ms_per_step (both rounded in the line)
    assert line["value"] == pytest.approx(n * bench.REC_BYTES / 2**30 / (line["ms_per_step"] / 1e3), rel=0.02)
    assert line["full"] is False and not [k for k in FULL_ONLY if k in line]

    files = sorted(os.listdir(out))
    assert files == sorted(line["dumped_outputs"]["files"]) == ["col0.npy", "col1.npy", "col2.npy", "col3.npy",
                                                                "records.npy", "wire.npy"]
    got = {f[:-4]: np.load(out / f) for f in files}
    assert sum(a.nbytes for a in got.values()) == line["dumped_outputs"]["bytes"] <= 64 * 10**6
    assert got["wire"].dtype == np.float32 and got["wire"].shape == (n, bench.REC_BYTES)
    assert np.array_equal(got["records"], np.arange(n, dtype=np.float64))
    cols = oracle.splitmix_columns_i32(4, n)
    want = np.frombuffer(oracle.pack([oracle.INT32] * 4, cols, n), np.uint8).reshape(n, bench.REC_BYTES)
    assert np.array_equal(got["wire"], want.astype(np.float32))
    for f, c in enumerate(cols):
        assert got[f"col{f}"].dtype == np.float64 and np.array_equal(got[f"col{f}"], c.astype(np.float64))
