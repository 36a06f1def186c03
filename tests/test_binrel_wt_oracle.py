"""BinRel-WT(sdsl) oracle (oracle/binrel_wt_oracle.cpp) against the reference's
own tests (tests/test_bin_rel_wt_sdsl.cpp:15-176) and the synthetic row spec.
CPU only."""
import numpy as np
import pytest


def _check(O, dense):
    t = O.OracleWT.from_dense(dense)
    n, m = dense.shape
    assert t.num_rows() == n and t.num_columns() == m and t.num_relations() == int(dense.sum())
    for r in range(n):
        assert t.get_row(r) == np.nonzero(dense[r])[0].tolist()
        for c in range(m):
            assert t.get(r, c) == bool(dense[r, c])
    for c in range(m):
        assert t.get_column(c).tolist() == np.nonzero(dense[:, c])[0].tolist()


def test_empty(oracle_mod):
    e = oracle_mod.OracleWT.empty()
    assert e.num_rows() == 0 and e.num_columns() == 0


@pytest.mark.parametrize("kind", ["zero", "one", "mixed"])
def test_reference_grids(oracle_mod, kind):
    hi = 20 if kind == "zero" else 10
    for m in range(1, hi):
        for n in range(1, hi):
            if kind == "zero":
                dense = np.zeros((n, m), dtype=bool)
            elif kind == "one":
                dense = np.ones((n, m), dtype=bool)
            else:  # first and last columns all zero (test_bin_rel_wt_sdsl.cpp:150-153)
                dense = np.zeros((n, m), dtype=bool)
                for j in range(n):
                    for i in range(1, m - 1):
                        dense[j, i] = (i + j) % 2
            _check(oracle_mod, dense)


@pytest.mark.parametrize("n,m,d", [(300, 3173, 0.038), (500, 257, 0.1), (200, 2, 0.5), (100, 1, 0.7)])
def test_random(oracle_mod, n, m, d):
    dense = np.random.default_rng(n + m).random((n, m)) < d
    _check(oracle_mod, dense)


def test_unsorted_and_repeated_ids(oracle_mod):
    """Rows are emitted by generate_rows in any order; interval_symbols still
    returns ascending ids.  A repeated id shows the reference's padding zero
    and repeated row (bin_rel_wt_sdsl.cpp:66-82, :85-96)."""
    O = oracle_mod
    t = O.OracleWT.from_csr(np.array([0, 3, 5], dtype=np.uint64), np.array([5, 1, 3, 2, 2], dtype=np.uint32), 6)
    assert t.get_row(0) == [1, 3, 5]
    assert t.get_row(1) == [2, 0]
    assert t.get_column(2).tolist() == [1, 1]
    assert t.get(1, 2) and not t.get(1, 0)


@pytest.mark.parametrize("m", [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32])
def test_wide_symbols_against_numpy(oracle_mod, m):
    """31-, 32- and 33-level trees (code_length(num_columns) reaches 33 at
    2^32 columns, one more than the 32-bit symbols) on the chunk-per-row / w32
    CSRs of tests/wt_shapes.py, against the numpy reference over the CSR: the
    rows, every present column, present and absent get.  Before the shifts by
    L and by L - 1 - l were guarded, rank() tested `c >> 32` on a u32, and
    get / get_column were wrong at 2^31 and 2^32 - 1 columns."""
    import wt_shapes as S
    off, cols = S.chunk_per_row(m)
    t = oracle_mod.OracleWT.from_csr(off, cols, m)
    n = len(off) - 1
    assert t.num_rows() == n and t.num_columns() == m and t.num_relations() == len(cols)
    rows = np.concatenate([np.arange(n), np.arange(n)[::-1]]).astype(np.uint64)
    r_off, r_cols = S.ref_rows(off, cols, rows)
    o_off, o_cols = t.get_rows(rows)
    np.testing.assert_array_equal(o_off, r_off)
    np.testing.assert_array_equal(o_cols, r_cols)
    for c in np.unique(cols).tolist():
        np.testing.assert_array_equal(t.get_column(c), S.ref_column(off, cols, c), err_msg=f"column {c}")
    for c in S.absent_columns(cols, m):
        assert len(t.get_column(c)) == 0, c
    qr, qc, want = S.point_queries(off, cols, m)
    assert want.any() and not want.all()
    got = np.array([t.get(int(r), int(c)) for r, c in zip(qr, qc)])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(S.ref_get(off, cols, qr, qc), want)
    with pytest.raises(IndexError):
        t.get_column(m)


def _mix64(z):
    M = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_synthetic_row_spec(oracle_mod):
    """wt_synth_row follows DESIGN.md "BinRel-WT" (re-derived here in Python)."""
    O = oracle_mod
    M = (1 << 64) - 1
    m, d, seed = 300, 0.05, 42
    T = int(d * 2.0**64)
    assert O.lib().wt_synth_threshold(d) == T
    off, cols = O.wt_synth_rows(1000, 20, m, d, seed)
    for i in range(20):
        K = _mix64(seed ^ (((1000 + i + 1) * 0x9E3779B97F4A7C15) & M))
        want = [c for c in range(m) if _mix64((K + c * 0xD1B54A32D192ED03) & M) < T]
        assert cols[off[i]:off[i + 1]].tolist() == want
    off, cols = O.wt_synth_rows(0, 20000, 3173, 0.038, 42)
    assert abs(off[-1] / 20000 - 3173 * 0.038) < 1.0
