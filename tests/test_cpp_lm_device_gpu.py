"""GPU: the C++ facade's device-side lmpar (BlockDiagonalSparseQR::lmparDevice, include/qrkit/QRKit.hpp) against its lmpar through
tests/cpp/test_lm_device.cpp, run the way test_cpp_lm_gpu.py runs the facade's LM test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_facade_lmpar_device():
    subprocess.check_call(["make", "-C", ROOT, "-s", "cpptest"])
    out = subprocess.run([os.path.join(ROOT, "build", "test_lm_device")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Failed." not in out.stdout and out.stdout.count("Passed.") == 2


def test_cpp_lm_device_compiles():
    """CPU: the test compiles and links against the library (no GPU needed)."""
    subprocess.check_call(["make", "-C", ROOT, "-s", "cpptest"])
    assert os.path.exists(os.path.join(ROOT, "build", "test_lm_device"))
