"""The 22 device pipelines on degenerate inputs (tests/_query_cases.py): empty
windows, joins that match nothing, a single survivor, one hot key, sums that
are exactly zero, ties across a LIMIT cut-off and short results. The
expectation is the numpy oracle, itself anchored to pyarrow Acero on the same
mutated inputs by tests/test_query_cases_cpu.py.

Row sets, keys, counts, strings and output order are compared exactly. On
the EXACT base every product and sum is exact in f64, so sums are compared
with array_equal as well: the comparison bodies of test_gpu_q4_q10_q18.py
are called with the mutated tables and their assert_allclose is replaced by
an equality check. Q6 and Q19 need the generator's own discounts and
quantities and keep the tolerance their existing comparison has (rtol 1e-9;
under zero_sum that tolerance still demands exactly 0.0).

Q3Fused finds its groups by a non-zero revenue sum (its documented
precondition; the fix was measured and fell outside the bench gate,
profiles/query_cases.md), so the fused paths are compared with the oracle
restricted to the non-zero groups; only q3-zero_sum has any other group, and
there the generic q3() is held to the full oracle."""
import numpy as np
import pytest

import _query_cases as QC
import test_gpu_q4_q10_q18 as B
from oracle import queries as OQ

pytestmark = pytest.mark.gpu

WRITTEN_OUT = ("q1", "q3", "q5", "q6")
REUSED = [(c, i) for c, i in zip(QC.CASES, QC.CASE_IDS)
          if c[0] not in WRITTEN_OUT]


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _cases(q):
    return pytest.mark.parametrize(
        "mut", [m for qq, m in QC.CASES if qq == q])


def _free(*colsets):
    for cs in colsets:
        for c in cs.values():
            c.free()


# the reused bodies that compare a float column, i.e. call assert_allclose
FLOAT_BODIES = ("q2", "q7", "q8", "q9", "q10", "q11", "q14", "q15", "q17",
                "q18", "q19", "q22")


@pytest.mark.parametrize("case", [c for c, _ in REUSED],
                         ids=[i for _, i in REUSED])
def test_pipeline_vs_oracle(gpu, case, monkeypatch):
    q, mut = case
    d = QC.build(q, mut)
    QC.check_precondition(q, mut, d)
    hits = []

    def exact(actual, desired, rtol=0.0, err_msg="", **kw):
        hits.append(err_msg)
        assert np.array_equal(np.asarray(actual, dtype=np.float64),
                              np.asarray(desired, dtype=np.float64)), \
            "%s: %r != %r" % (err_msg, actual, desired)

    if q not in QC.RAW_QUERIES:
        monkeypatch.setattr(np.testing, "assert_allclose", exact)
    getattr(B, "test_%s_device_vs_oracle" % q)(gpu, d)
    if q in FLOAT_BODIES and q not in QC.RAW_QUERIES:
        # the body really went through the equality check (it would not if
        # it ever bound assert_allclose by another name); a dict-shaped
        # answer with no entry has nothing to compare
        assert hits or QC.n_groups(q, QC.run_oracle(q, d)) == 0, q


@_cases("q1")
def test_q1(gpu, mut):
    from quokka_amd import staging, queries as DQ
    d = QC.build("q1", mut)
    QC.check_precondition("q1", mut, d)
    li = d["lineitem"]
    cols = staging.stage_columns(li, names=[
        "l_shipdate", "l_quantity", "l_extendedprice", "l_discount",
        "l_tax", "l_returnflag", "l_linestatus"])
    try:
        got = DQ.q1(cols)
    finally:
        _free(cols)
    want = OQ.q1(li)
    assert list(got["l_returnflag"]) == list(want["l_returnflag"])
    assert list(got["l_linestatus"]) == list(want["l_linestatus"])
    for c in ("count_order", "sum_qty", "sum_base_price", "sum_disc_price",
              "sum_charge", "avg_qty", "avg_price", "avg_disc"):
        assert np.array_equal(got[c], want[c]), c


@_cases("q6")
def test_q6(gpu, mut):
    from quokka_amd import staging, queries as DQ
    d = QC.build("q6", mut)
    QC.check_precondition("q6", mut, d)
    li = d["lineitem"]
    cols = staging.stage_columns(li, names=[
        "l_shipdate", "l_quantity", "l_extendedprice", "l_discount"])
    try:
        got = DQ.q6(cols)
    finally:
        _free(cols)
    want = OQ.q6(li)
    assert got["rows_passed"] == want["rows_passed"]
    # the tolerance of test_gpu_parity.test_q6_parity; exact when want is 0
    np.testing.assert_allclose(got["revenue"], want["revenue"], rtol=1e-9)


def _by_key(full):
    o = np.argsort(full["l_orderkey"], kind="stable")
    return {c: v[o] for c, v in full.items()}


def _same_groups(got, want, what):
    got, want = _by_key(got), _by_key(want)
    for c in ("l_orderkey", "o_orderdate", "o_shippriority", "revenue"):
        assert np.array_equal(got[c], want[c]), (what, c)


def _same_top(got, want, what):
    assert len(got["l_orderkey"]) == len(want["l_orderkey"]), what
    for c in ("l_orderkey", "o_orderdate", "o_shippriority", "revenue"):
        assert np.array_equal(got[c], want[c]), (what, c)


@_cases("q3")
def test_q3(gpu, mut):
    """Generic q3() against the full oracle; q3_fused, every probe variant
    and extract_top10 against the oracle's non-zero groups."""
    from quokka_amd import staging, queries as DQ
    d = QC.build("q3", mut)
    QC.check_precondition("q3", mut, d)
    li, od, cu = d["lineitem"], d["orders"], d["customer"]
    wfull, wtop = OQ.q3(li, od, cu)
    nz = wfull["revenue"] != 0.0
    assert nz.all() or mut == "zero_sum"
    rfull = {c: v[nz] for c, v in wfull.items()}
    o = np.lexsort((rfull["l_orderkey"], rfull["o_orderdate"],
                    -rfull["revenue"]))[:10]
    rtop = {c: v[o] for c, v in rfull.items()}

    lcols = staging.stage_columns(li, names=["l_orderkey", "l_shipdate",
                                             "l_extendedprice", "l_discount"])
    ocols = staging.stage_columns(od, names=["o_orderkey", "o_custkey",
                                             "o_orderdate", "o_shippriority"])
    ccols = staging.stage_columns(cu, names=["c_custkey", "c_mktsegment"])
    st = None
    try:
        full, top = DQ.q3(lcols, ocols, ccols)
        _same_groups(full, wfull, "q3")
        _same_top(top, wtop, "q3")

        full, top = DQ.q3_fused(lcols, ocols, ccols)
        _same_groups(full, rfull, "q3_fused")
        _same_top(top, rtop, "q3_fused")

        st = DQ.Q3Fused(ocols, ccols)
        for nt in (False, True, 4):
            st.reset_sums()
            st.probe(lcols, nt=nt)
            full, top = st.extract()
            _same_groups(full, rfull, "nt=%r" % nt)
            _same_top(top, rtop, "nt=%r" % nt)
            k, top = st.extract_top10()
            assert k == int(nz.sum()), nt
            _same_top(top, rtop, "extract_top10 nt=%r" % nt)
    finally:
        if st is not None:
            st.free()
        _free(lcols, ocols, ccols)


@_cases("q5")
def test_q5(gpu, mut):
    from quokka_amd import staging, queries as DQ
    d = QC.build("q5", mut)
    QC.check_precondition("q5", mut, d)
    li, od, cu, su = d["lineitem"], d["orders"], d["customer"], d["supplier"]
    want = OQ.q5(li, od, cu, su, d["nation"], d["region"])
    lcols = staging.stage_columns(li, names=["l_orderkey", "l_suppkey",
                                             "l_extendedprice", "l_discount"])
    ocols = staging.stage_columns(od, names=["o_orderkey", "o_custkey",
                                             "o_orderdate"])
    ccols = staging.stage_columns(cu, names=["c_custkey", "c_nationkey"])
    scols = staging.stage_columns(su, names=["s_suppkey", "s_nationkey"])
    st = None
    try:
        results = [("q5_fused", DQ.q5_fused(lcols, ocols, ccols, scols))]
        st = DQ.Q5Fused(ocols, ccols, scols)
        for nt in (False, True):
            st.reset_sums()
            st.probe(lcols, nt=nt)
            results.append(("nt=%r" % nt, st.result()))
    finally:
        if st is not None:
            st.free()
        _free(lcols, ocols, ccols, scols)
    for what, got in results:
        assert [n for n, _ in got] == [n for n, _ in want], what
        assert np.array_equal([v for _, v in got], [v for _, v in want]), what
