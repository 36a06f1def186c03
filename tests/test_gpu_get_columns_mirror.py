"""C++ mirror of the batched column query: BRWTDevice::get_columns
(csrc/brwt_device.hpp over mbrwt_get_columns) compiled and run from
tests/cpp/get_columns/ against the matrix the context was built from."""
import os
import subprocess

import pytest

from conftest import gpu_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "get_columns")


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a GPU")
def test_cpp_mirror_get_columns():
    subprocess.run(["make", "-s", "-C", CPP, "_build/test_get_columns"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "test_get_columns")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 tests, 0 failed checks" in r.stdout, r.stdout
