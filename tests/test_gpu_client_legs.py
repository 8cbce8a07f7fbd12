"""srpc::gpu::batch_client::call_legs (include/srpc/gpu_client.hpp): column,
record and string-bodied legs in one ordered batch against a
srpc::gpu::batch_server with methods of all three kinds over a socketpair:
tests/cpp/gpu_client_legs_test.cpp."""
import os
import subprocess

import pytest

from tests.cpp import build_cpp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cpp_call_legs():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srpc_amd import build
    build.build()
    exe = build_cpp.build_one(os.path.join(HERE, "cpp", "gpu_client_legs_test.cpp"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failed" in out.stdout, out.stdout + out.stderr
