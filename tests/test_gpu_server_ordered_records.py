"""srpc::gpu::batch_server in ordered records mode (include/srpc/gpu_server.hpp:
set_ordered_records, set_ordered_records_handler): record handlers see their
requests in arrival order across batches, a stateful whole-batch handler over
struct arrays with unknown frames answered by the CPU server in place, the same
reply bytes as the bucket route, mode switches on one server, the refusals:
tests/cpp/gpu_server_ordered_records_test.cpp."""
import os
import subprocess

import pytest

from tests.cpp import build_cpp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cpp_batch_server_ordered_records():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srpc_amd import build
    build.build()
    exe = build_cpp.build_one(os.path.join(HERE, "cpp", "gpu_server_ordered_records_test.cpp"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failed" in out.stdout, out.stdout + out.stderr
