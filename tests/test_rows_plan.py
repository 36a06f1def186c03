"""The row-record build's decisions (csrc/rows_plan.hpp: candidate block
shapes, their cost, the choice, the block override, the row / S magic number,
the record-code rule) as pure host code: tests/cpp/test_rows_plan.cpp, built
without the library and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_rows_plan_host_rules():
    subprocess.run(["make", "-s", "-C", CPP, "rows_plan"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "test_rows_plan")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "11 tests, 0 failed checks" in r.stdout, r.stdout
