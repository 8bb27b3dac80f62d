"""The join-payload cases pinned without a GPU: on every executor case and
every `how` the plain-Python model of tests/_join_payload_cases.py (left
probe + optional take) gives exactly pyarrow Acero's join, NULLs, NaN and
-0.0 included; and the case tables hold what the GPU tests rely on."""
import numpy as np
import pytest

import _join_payload_cases as C

pa = pytest.importorskip("pyarrow")


@pytest.mark.parametrize("how", C.HOWS)
@pytest.mark.parametrize("name", sorted(C.EXECUTOR_CASES))
def test_model_equals_acero(name, how):
    c = C.executor_case(pa, name)
    args = (c["probe"], c["build"], how, c["left_on"], c["right_on"],
            c["key_to_keep"])
    C.assert_tables_equal(C.model_join(*args), C.acero_join(*args),
                          ["pid", "bid"])


@pytest.mark.parametrize("name", sorted(C.EXECUTOR_CASES))
def test_executor_cases_hold_their_edges(name):
    c = C.executor_case(pa, name)
    probe, build = c["probe"], c["build"]
    for t, p in ((probe, "p_"), (build, "b_")):
        i64 = t.column(p + "i64").to_pylist()
        for v in (2 ** 53 + 1, C.I64_MIN, C.I64_MAX, None):
            assert v in i64, (p, v)
        f64 = t.column(p + "f64").to_pylist()
        assert None in f64 and any(v is not None and v != v for v in f64)
        assert any(v == 0 and np.signbit(v) for v in f64 if v is not None)
        s = t.column(p + "str").to_pylist()
        assert "" in s and None in s
        assert None in t.column(p + "d32").to_pylist()
        assert None in t.column(p + "bool").to_pylist()
        assert t.schema.field(p + "d32").type == pa.date32()
        assert t.schema.field(p + "i32").type == pa.int32()
    # hits, misses and chains all occur
    bk = build.column(c["right_on"]).to_pylist()
    pk = probe.column(c["left_on"]).to_pylist()
    present = {k for k in bk if k is not None}
    hits = sum(k in present for k in pk)
    assert 0.25 * len(pk) < hits < 0.75 * len(pk)
    assert len(present) < sum(k is not None for k in bk), "no chains"
    assert C.I64_MIN not in bk
    assert (None in bk and None in pk) == c["null_keys"]
    assert sum(len(b) for b in c["build_batches"]) == len(build)
    if len(c["build_batches"]) == 2:
        first, second = c["build_batches"]
        assert not any(first.column(n).null_count
                       for n in first.column_names)
        assert all(second.column("b_" + k).null_count
                   for k in ("i64", "d32", "bool", "f64", "str"))


def test_probe_model_rules():
    """The left probe on a hand-written case: chains emit every pair, a
    miss and a NULL key one NO_ROW pair, the value under a null is not
    looked at."""
    build, bvalid = [5, 7, 5, 9, 7, 5], [True, True, True, False, True, True]
    pk, pvalid = [5, 6, 7, 9, 5], [True, True, True, True, False]
    N = C.NO_ROW
    assert C.probe(build, bvalid, pk, pvalid, 3) == [
        (0, 0), (0, 2), (0, 5), (1, N), (2, 1), (2, 4), (3, N), (4, N)]
    assert C.probe(build, bvalid, pk, pvalid, 0) == [
        (0, 0), (0, 2), (0, 5), (2, 1), (2, 4)]
    assert C.probe(build, bvalid, pk, pvalid, 1) == [0, 2]
    assert C.probe(build, bvalid, pk, pvalid, 2) == [1, 3, 4]
    assert C.probe([], None, pk, None, 3) == [(i, N) for i in range(5)]


def test_take_model_rules():
    vals, mask = [10, 20, 30], [True, False, True]
    assert C.take_opt(vals, mask, [2, C.NO_ROW, 1, 0]) == \
        ([30, 0, 0, 10], [True, False, False, True], 2)
    assert C.take_opt(vals, None, [1, C.NO_ROW]) == \
        ([20, 0], [True, False], 1)
    assert C.take_opt(vals, mask, []) == ([], [], 0)


def test_take_case_table():
    rng = np.random.default_rng(0)
    sizes = C.take_sizes(256, 2048)
    assert len(set(sizes)) == len(sizes) == 12
    assert sizes[-1] > 256 * 2048          # a second grid-stride round
    for n in (1, 64, 129):
        for pattern in C.TAKE_PATTERNS:
            idx = C.take_idx(n, pattern, rng)
            no = idx == C.NO_ROW
            assert (idx[~no] < C.TAKE_N_SRC).all()
            want = {"none": 0, "all": n, "lane0": (n + 63) // 64,
                    "lane63": n // 64, "last": 1,
                    "alternating": n // 2}[pattern]
            assert int(no.sum()) == want, (n, pattern)
            for dt in C.TAKE_DTYPES:
                vals, mask = C.take_source(dt, "gathered rows all null",
                                           idx, rng)
                assert not mask[idx[~no]].any()
                assert (vals[~mask] == C.JUNK[dt]).all()


def test_probe_case_table():
    rng = np.random.default_rng(0)
    for kind in ("unique", "chains", "empty"):
        build, keys, mask = C.probe_case(kind, 2000, rng)
        assert C.I64_MIN not in build
        assert (keys[mask] == C.I64_MIN).any() and not mask.all()
        if kind == "chains":
            counts = np.unique(np.unique(build, return_counts=True)[1])
            assert counts.tolist() == [1, 2, 7]
        pairs = C.probe(build.tolist(), None, keys.tolist(), mask.tolist(), 3)
        assert {p for p, _ in pairs} == set(range(2000))
        if kind != "empty":
            assert any(b == C.NO_ROW for _, b in pairs)
            assert any(b != C.NO_ROW for _, b in pairs)
