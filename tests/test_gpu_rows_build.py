"""The decisions of whole row-record builds (csrc/rows_build.hip rows_build_*:
record code, block shape, tolerance, block override, variable-length records,
the AUTO decline, ranged builds) pinned to recorded values: every case builds
one small image and compares layout() and rows_stats() with
tests/golden/rows_build_decisions.json.

The golden file is this module's own output: `python tests/test_gpu_rows_build.py`
prints every case's record as JSON; with an earlier run's file as argument
it prints only the keys on which the two runs agree (the keys to pin).
Recorded that way on the commit before the build driver was split into steps
(7b41f3b): every key of every case agreed between the two runs, so all are
pinned.  Image bytes are not compared (spill entries are placed by an atomic
counter).

The block override 64,9 never reaches the build: mbrwt_set_build_option
refuses it (MBRWT_ERR_INVALID) and the option keeps its value, which the
cases record as `refused_options`; the build then takes the automatic choice.
The driver's own validity rule (an S that does not divide the alignment) is
covered on the host by tests/cpp/test_rows_plan.cpp.
"""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_build_decisions.json")

COMPACT = ("MBRWT_BUILD_ROWS_FOOTPRINT", 1)  # MBRWT_ROWS_COMPACT


def _code(c):
    return ("MBRWT_BUILD_ROWS_CODE", c)


# name -> (tree, layout, build options); a tree is (kind, args...)
SPARSE = ("dense", 5000, 300, 0.01, 11, "basic", 8, 0)
DENSE = ("dense", 5000, 64, 0.5, 12, "basic", 8, 0)
GREEDY = ("dense", 5000, 300, 0.01, 11, "greedy", 2, 10)
MIXED_BASIC = ("mixed", 5000, 300, 5, "basic", 8, 0)
MIXED_GREEDY = ("mixed", 5000, 300, 5, "greedy", 2, 10)
LONG = ("dense", 5000, 2652, 0.3, 13, "basic", 8, 0)
CASES = {
    # sparse uniform: the AUTO terminal records, the nibble codes, both forced codes
    "sparse_code0": (SPARSE, "rows", [_code(0)]),
    "sparse_code1": (SPARSE, "rows", [_code(1)]),
    "sparse_code2": (SPARSE, "rows", [_code(2)]),
    "sparse_code3": (SPARSE, "rows", [_code(3)]),
    # dense uniform: the compact codes give way to bytes (or not: as recorded)
    "dense_code0": (DENSE, "rows", [_code(0)]),
    "dense_code1": (DENSE, "rows", [_code(1)]),
    # greedy + relax: the non-uniform tolerance; COMPACT there and on a uniform tree
    "greedy_relax": (GREEDY, "rows", []),
    "greedy_relax_compact": (GREEDY, "rows", [COMPACT]),
    "uniform_compact": (SPARSE, "rows", [COMPACT]),
    # rows of very different lengths: spills and long rows in the automatic choice
    "mixed_basic": (MIXED_BASIC, "rows", [_code(3)]),
    "mixed_greedy": (MIXED_GREEDY, "rows", [_code(3)]),
    "mixed_basic_auto_code": (MIXED_BASIC, "rows", []),
    # a block override the rule ignores (64,9): the automatic choice
    "mixed_basic_ignored_override": (MIXED_BASIC, "rows", [_code(3), ("MBRWT_BUILD_ROWS_BLOCK", 64 << 8 | 9)]),
    "mixed_greedy_ignored_override": (MIXED_GREEDY, "rows", [_code(3), ("MBRWT_BUILD_ROWS_BLOCK", 64 << 8 | 9)]),
    # long rows: variable-length records forced, chosen (or not), or the decline to node images
    "long_var_forced": (LONG, "rows", [("MBRWT_BUILD_ROWS_VAR", 1)]),
    "long_rows": (LONG, "rows", []),
    "long_auto": (LONG, "auto", []),
    # a ranged build: three ranges, the decision on the first
    "ranged": (("synthetic", 800000, 300, 0.01, 8, 14), "rows", [("MBRWT_BUILD_ROWS_RANGE", 360360)]),
}
SAME_AS = {"mixed_basic_ignored_override": "mixed_basic", "mixed_greedy_ignored_override": "mixed_greedy"}


@functools.lru_cache(maxsize=None)
def _dense(kind, n, m, *rest):
    if kind == "mixed":  # the matrix of test_gpu_rows.test_every_block_shape: most rows sparse, some dense
        rng = np.random.default_rng(rest[0])
        u = rng.random(n)
        p = np.where(u < 0.005, 1.0, np.where(u < 0.025, 0.5, 0.01))
        return rng.random((n, m)) < p[:, None]
    d, seed = rest
    return np.random.default_rng(seed).random((n, m)) < d


@functools.lru_cache(maxsize=None)
def _export(tree):
    """The oracle's tree of a dense case, built once per module and shared."""
    import oracle as O
    O.build()
    n, m = tree[1], tree[2]
    part, arity, relax = tree[-3:]
    return O.OracleTree.from_dense(_dense(tree[0], n, m, *tree[3:-3]), part, arity, relax).export()


def build_record(name):
    """Build the case's image; its decisions as a dict."""
    from genome_graph_annotation_amd import BRWTDevice, MBRWTError, _lib as L
    from genome_graph_annotation_amd.brwt import build_option
    tree, layout, options = CASES[name]
    refused = []
    with contextlib.ExitStack() as stack:
        for opt, value in options:
            try:
                stack.enter_context(build_option(getattr(L, opt), value))
            except MBRWTError as e:  # (64,9: mbrwt_set_build_option itself refuses it; the option keeps its value)
                assert e.status == L.MBRWT_ERR_INVALID
                refused.append(opt)
        try:
            if tree[0] == "synthetic":
                dev = BRWTDevice.synthetic(*tree[1:], layout=layout)
            else:
                dev = BRWTDevice.from_tree(_export(tree), layout=layout)
        except MBRWTError as e:
            return {"error": e.status, "refused_options": refused}
    rec = {"layout": dev.layout(), "refused_options": refused}
    rec.update(dev.rows_stats() or {})
    dev.close()
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_build_decisions(oracle_mod, golden, name):
    want = golden[name]
    got = build_record(name)
    print(name, json.dumps(got, sort_keys=True))
    assert {k: got.get(k) for k in want} == want
    if name in SAME_AS:  # an ignored override: the automatic choice
        assert got["refused_options"] == ["MBRWT_BUILD_ROWS_BLOCK"]
        auto = dict(golden[SAME_AS[name]], refused_options=got["refused_options"])
        assert want == auto


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)
    for name, want in golden.items():
        assert "layout" in want or "error" in want, name
        if want.get("layout") in ("rows", "both"):
            assert {"block_bytes", "rows_per_block", "nibble_codes", "terminal_records", "variable"} <= set(want), name


if __name__ == "__main__":
    records = {name: build_record(name) for name in CASES}
    if len(sys.argv) > 1:  # an earlier run: keep the keys on which both agree
        with open(sys.argv[1]) as f:
            earlier = json.load(f)
        for name, rec in records.items():
            for k in [k for k in rec if k not in earlier[name] or earlier[name][k] != rec[k]]:
                print(f"{name}: {k} differs between the runs ({earlier[name].get(k)} / {rec[k]})", file=sys.stderr)
                del rec[k]
    print(json.dumps(records, indent=1, sort_keys=True))
