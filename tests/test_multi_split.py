"""The read split of the multi-device classify calls (csrc/multi_split.hpp:
validation of the read offsets, the cut rule, its balance bound, where reads
without rows go) as pure host code: tests/cpp/multi/test_multi_split.cpp,
built without the library and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "multi")


def test_multi_split_host_rules():
    subprocess.run(["make", "-s", "-C", CPP, "split"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "test_multi_split")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "9 tests, 0 failed checks" in r.stdout, r.stdout
