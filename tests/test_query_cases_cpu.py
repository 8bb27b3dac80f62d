"""The degenerate-input case table (tests/_query_cases.py), validated without
a GPU: every case's precondition holds on the oracle's answer, and the numpy
oracle equals pyarrow Acero on every mutated input (the restatements of
tests/test_oracle_acero.py, called with the mutated tables). The device
pipelines are then compared with this anchored oracle in
tests/test_gpu_query_cases.py."""
import numpy as np
import pytest

import _query_cases as QC
import test_oracle_acero as A


def test_base_answers_nonempty():
    """The SF written into the case module: every table is non-empty and
    every one of the 22 answers on the unmutated data has a row."""
    for kind in ("raw", "exact"):
        d = QC.base(kind)
        for t, cols in d.items():
            if isinstance(cols, dict):
                assert all(len(a) > 0 for a in cols.values()), t
        for i in range(1, 23):
            q = "q%d" % i
            if kind == "exact" and q in QC.RAW_QUERIES:
                continue
            assert QC.n_groups(q, QC.run_oracle(q, d)) > 0, (kind, q)


def test_case_table_covers_every_query():
    by_q = {}
    for q, mut in QC.CASES:
        by_q.setdefault(q, set()).add(mut)
    assert sorted(by_q, key=lambda q: int(q[1:])) == \
        ["q%d" % i for i in range(1, 23)]
    for q, muts in by_q.items():
        assert len(muts) >= 3, q
        assert {"window_miss", "one_survivor"} <= muts, q
    for q in QC.LIMITS:
        assert {"tie_at_limit", "short_result"} <= by_q[q], q


@pytest.mark.parametrize("q,mut", QC.CASES, ids=QC.CASE_IDS)
def test_mutator_rules(q, mut):
    """Row counts, column sets and dtypes unchanged; dense keys still dense;
    the result is read-only and the base was not written."""
    d = QC.build(q, mut)
    sf = QC.SF_Q21_TIE if (q, mut) == ("q21", "tie_at_limit") else QC.SF
    b = QC.base("raw" if q in QC.RAW_QUERIES else "exact", sf)
    for t, cols in b.items():
        if not isinstance(cols, dict):
            continue
        assert set(cols) == set(d[t]), t
        for c, a in cols.items():
            assert d[t][c].dtype == a.dtype and d[t][c].shape == a.shape, c
            assert not d[t][c].flags.writeable and not a.flags.writeable
    for t, k in (("customer", "c_custkey"), ("supplier", "s_suppkey"),
                 ("part", "p_partkey")):
        assert np.array_equal(d[t][k], np.arange(1, len(d[t][k]) + 1))
    assert np.array_equal(d["orders"]["o_orderkey"],
                          b["orders"]["o_orderkey"])


@pytest.mark.parametrize("q,mut", QC.CASES, ids=QC.CASE_IDS)
def test_precondition(q, mut):
    QC.check_precondition(q, mut, QC.build(q, mut))


@pytest.mark.parametrize("q,mut", QC.CASES, ids=QC.CASE_IDS)
def test_oracle_equals_acero(q, mut):
    getattr(A, "test_%s_oracle_equals_acero" % q)(QC.build(q, mut))
