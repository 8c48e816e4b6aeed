"""GPU: the C++ facade's reduced LM route and qrkit::DenseQlessR (include/qrkit/QRKit.hpp) through
tests/cpp/test_angular_lm_reduced.cpp, run the way test_cpp_angular_lm_gpu.py runs test_angular_lm."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_facade_angular_lm_reduced():
    subprocess.check_call(["make", "-C", ROOT, "-s", "cpptest"])
    out = subprocess.run([os.path.join(ROOT, "build", "test_angular_lm_reduced")], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Failed." not in out.stdout and out.stdout.count("Passed.") == 3


def test_cpp_angular_lm_reduced_compiles():
    """CPU: the test compiles and links against the library (no GPU needed)."""
    subprocess.check_call(["make", "-C", ROOT, "-s", "cpptest"])
    assert os.path.exists(os.path.join(ROOT, "build", "test_angular_lm_reduced"))
