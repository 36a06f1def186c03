"""C++ mirror of the tree shape from rows: BRWTDevice::build_from_rows_greedy
(csrc/brwt_device.hpp) compiled and run from tests/cpp/shape_from_rows/
against the oracle."""
import os
import subprocess

import pytest

from conftest import gpu_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "shape_from_rows")


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a GPU")
def test_cpp_mirror_builds_the_greedy_shape_from_rows(oracle_mod):
    subprocess.run(["make", "-s", "-C", CPP], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "test_shape_from_rows")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 tests, 0 failed checks" in r.stdout, r.stdout
