"""Null values in the aggregate without a GPU (DESIGN.md §3a''''): the
numpy model of tests/_null_value_cases.py against pyarrow Acero, the
independent oracle (sum / min / max skip nulls and, at min_count=1, give
NULL for a group without a value), and the host half of
GPUAggExecutor(null_values=True): what the constructor refuses, and the
final-expression step over host arrays."""
import pickle

import numpy as np
import pytest

import _null_value_cases as C

pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")


def _acero(codes, vals, masks, ops, ngroups):
    """-> (acc, valid) as the model gives them, from Table.group_by; a
    group that has no row at all is the identity and invalid in both."""
    cols = {"g": pa.array(np.asarray(codes, dtype=np.int64))}
    for c, (v, m) in enumerate(zip(vals, masks)):
        cols["v%d" % c] = pa.array(v) if m is None else pa.array(v, mask=~m)
    opt = pc.ScalarAggregateOptions(skip_nulls=True, min_count=1)
    out = pa.table(cols).group_by(["g"], use_threads=False).aggregate(
        [("v%d" % c, C.ACERO_FN[op], opt) for c, op in enumerate(ops)])
    g = np.asarray(out.column("g"))
    acc = np.array([[C.AGG_INIT[op]] * ngroups for op in ops])
    valid = np.zeros((len(ops), ngroups), dtype=bool)
    for c, op in enumerate(ops):
        col = out.column("v%d_%s" % (c, C.ACERO_FN[op])).combine_chunks()
        ok = np.asarray(col.is_valid())
        valid[c, g[ok]] = True
        acc[c, g[ok]] = np.asarray(col.fill_null(0.0))[ok]
    return acc, valid


def _same(got, want):
    (acc, valid), (wacc, wvalid) = got, want
    assert np.array_equal(valid, wvalid)
    assert np.array_equal(acc, wacc)    # small integers: exact, inf included


@pytest.mark.parametrize("nvals", C.KERNEL_NVALS)
@pytest.mark.parametrize("n", C.KERNEL_N + [C.GRID_ROWS + 65])
def test_model_aggregates_like_acero(n, nvals):
    case = C.kernel_case(n, nvals)
    codes, vals, masks, ops, ngroups = case
    got = C.aggregate(*case)
    _same(got, _acero(*case))
    # the case holds what it promises
    assert any(m is not None and not m.all() for m in masks)
    if nvals > 1:
        assert any(m is None for m in masks)
    assert not got[1][0, min(1, ngroups - 1)], "an all-NULL group"
    for v, m in zip(vals, masks):
        if m is not None and not m.all():
            junk = v[~m]
            assert (np.isnan(junk) | (np.abs(junk) > 1e299)).all()


def test_model_identity_is_not_null_like_acero():
    case = C.identity_case()
    acc, valid = C.aggregate(*case)
    _same((acc, valid), _acero(*case))
    assert valid[:, 0].all() and acc[:, 0].tolist() == [0.0, np.inf, -np.inf]
    assert not valid[:, 1].any()
    assert acc[:, 1].tolist() == [0.0, np.inf, -np.inf], "identity under NULL"
    assert valid[0, 2] and acc[0, 2] == 0.0
    assert acc[:, 3].tolist() == [9.0, 4.0, 5.0]


def test_model_batches_like_acero():
    batches, ops = C.batch_case()
    keys = np.concatenate([k for k, _, _ in batches])
    uniq, codes = np.unique(keys, return_inverse=True)
    vals = [np.concatenate([v[c] for _, v, _ in batches]) for c in range(3)]
    masks = [np.concatenate([m[c] for _, _, m in batches]) for c in range(3)]
    got = C.aggregate(codes, vals, masks, ops, len(uniq))
    _same(got, _acero(codes, vals, masks, ops, len(uniq)))
    for key in (C.LATE, C.EARLY):
        assert got[1][:, np.searchsorted(uniq, key)].all(), "one value each"
    first = batches[0]
    assert not any(m[first[0] == C.LATE].any() for m in first[2])


# ---- GPUAggExecutor(null_values=True): host only -------------------------
def test_null_values_constructor():
    from quokka_amd.executors import GPUAggExecutor
    with pytest.raises(ValueError, match="device_keys"):
        GPUAggExecutor(["g"], None, "sum(x) as sx", null_values=True)
    grand = GPUAggExecutor([], None, "sum(x) as sx", null_values=True)
    keyed = GPUAggExecutor(["g"], None, C.AGG_SQL, device_keys=True,
                           null_keys=True, null_values=True)
    for ex in (grand, keyed):
        twin = pickle.loads(pickle.dumps(ex))
        assert twin.null_values and twin.sum_cols == ex.sum_cols
    assert not GPUAggExecutor(["g"], None, "sum(x) as sx").null_values
    wide = ", ".join("sum(c%d) as s%d" % (i, i) for i in range(65))
    with pytest.raises(ValueError, match="64"):
        GPUAggExecutor([], None, wide, null_values=True)
    GPUAggExecutor([], None, wide)


def _final(sql, order, s, valid, keys=None):
    from quokka_amd.executors import GPUAggExecutor, _to_table
    ex = GPUAggExecutor(["g"], order, sql, device_keys=True,
                        null_values=True)
    out, _ = ex._final_columns(dict(keys or {}), s, valid)
    return _to_table(out)


def test_final_expressions_propagate_null():
    t, f = True, False
    s = {"a": np.array([6.0, 0.0, 8.0, 0.0]),
         "b": np.array([3.0, 2.0, 0.0, 0.0]),         # identities under NULL
         "c": np.array([1.0, np.inf, 5.0, 7.0])}
    valid = {"a": np.array([t, f, t, f]), "b": np.array([t, t, f, f]),
             "c": np.array([t, f, t, t])}
    with np.errstate(all="raise"):      # 8 / 0 and 0 / 0 stay silent
        out = _final("sum(a)/sum(b) as r, min(c) as lo, sum(b) as sb", None,
                     s, valid)
    assert out.column("r").type == pa.float64()
    assert out.column("r").to_pylist() == [2.0, None, None, None]
    assert out.column("lo").to_pylist() == [1.0, None, 5.0, 7.0]
    assert out.column("sb").to_pylist() == [3.0, 2.0, None, None]


def test_final_alias_without_null_is_a_plain_column():
    s = {"a": np.array([6.0, 1.0]), "b": np.array([3.0, 0.0])}
    valid = {"a": np.array([True, True]), "b": np.array([True, False])}
    out = _final("sum(a) as sa, sum(a) + sum(b) as ab", None, s, valid)
    sa = out.column("sa")
    assert sa.null_count == 0 and sa.type == pa.float64()
    assert sa.to_pylist() == [6.0, 1.0]
    assert out.column("ab").to_pylist() == [9.0, None]
    # and it is what the default gives for the same sums
    from quokka_amd.executors import GPUAggExecutor, _to_table
    ex = GPUAggExecutor(["g"], None, "sum(a) as sa", device_keys=True)
    plain, _ = ex._final_columns({}, s)
    assert _to_table(plain).column("sa").equals(sa)


@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_final_order_by_puts_null_aliases_last(direction):
    """Against pyarrow's sort_by, which places nulls at the end either
    way. The slots under the NULLs hold what would sort first."""
    g = np.arange(6, dtype=np.int64)
    s = {"a": np.array([3.0, -np.inf, 1.0, np.inf, 2.0, np.nan])}
    valid = {"a": np.array([True, False, True, False, True, False])}
    out = _final("sum(a) as sa", [("sa", direction), ("g", "asc")], s,
                 valid, keys={"g": g})
    want = pa.table({"g": g, "sa": pa.array(s["a"], mask=~valid["a"])}
                    ).sort_by([("sa", direction + "ending"),
                               ("g", "ascending")])
    assert out.column("sa").to_pylist() == want.column("sa").to_pylist()
    assert out.column("g").to_pylist() == want.column("g").to_pylist()
    assert out.column("sa").to_pylist()[-3:] == [None] * 3
