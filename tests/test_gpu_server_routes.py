"""srpc::gpu::batch_server across its routes (include/srpc/gpu_server.hpp): one
server served again after register_* and mode changes, the byte counters and
the warm-up calls of every route, the bucket route's overflow demotion, in
lock-step batches of 16 over a socketpair:
tests/cpp/gpu_server_routes_test.cpp."""
import os
import subprocess

import pytest

from tests.cpp import build_cpp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cpp_batch_server_routes():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srpc_amd import build
    build.build()
    exe = build_cpp.build_one(os.path.join(HERE, "cpp", "gpu_server_routes_test.cpp"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failed" in out.stdout, out.stdout + out.stderr
