"""C++ mirror of the build from sparse columns:
BRWTDevice::build_from_sparse_columns[_greedy] (csrc/brwt_device.hpp) compiled
and run from tests/cpp/from_sparse_columns/ against the oracle."""
import os
import subprocess

import pytest

from conftest import gpu_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "from_sparse_columns")


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a GPU")
def test_cpp_mirror_builds_from_sparse_columns(oracle_mod):
    subprocess.run(["make", "-s", "-C", CPP, "_build/test_from_sparse_columns"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "test_from_sparse_columns")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "4 tests, 0 failed checks" in r.stdout, r.stdout
