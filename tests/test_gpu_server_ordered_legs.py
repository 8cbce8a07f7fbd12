"""srpc::gpu::batch_server::set_ordered_legs / set_ordered_legs_handler
(include/srpc/gpu_server.hpp): a column method, a record method and a
string-bodied method served side by side in arrival order, through one
srpc_frames_unpack_requests_mixed_legs and one
srpc_frames_pack_requests_mixed_legs a batch, over a socketpair:
tests/cpp/gpu_server_ordered_legs_test.cpp."""
import os
import subprocess

import pytest

from tests.cpp import build_cpp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cpp_ordered_legs():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srpc_amd import build
    build.build()
    exe = build_cpp.build_one(os.path.join(HERE, "cpp", "gpu_server_ordered_legs_test.cpp"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failed" in out.stdout, out.stdout + out.stderr
