"""The float-edge case tables of tests/_float_agg_cases.py against pyarrow
Acero (the engine the queries are anchored to), the facts about the case
data that the GPU tests lean on, and the host ends of the executors
(GPUAggExecutor._final_columns / _order_by, GPUTopKExecutor.done) over
NaN beside NULL. No device."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _float_agg_cases as C

pa = pytest.importorskip("pyarrow")

CASES = C.all_cases()


def _quieted(col):
    """The column with the quiet bit set on every NaN, sign and payload
    kept. Acero folds MIN/MAX with fmin/fmax, which the C library lets
    return NaN for a SIGNALLING NaN operand ({-inf, sNaN} -> NaN, seen
    with pyarrow 25): an artefact of the host libm, not a rule. The
    project's rule is one rule for every NaN, so Acero is asked about the
    quiet twin and the kernels get the signalling pattern itself."""
    v = np.array(col, dtype=np.float64)
    bits = v.view(np.uint64)
    bits[np.isnan(v)] |= np.uint64(0x0008000000000000)
    return v


def test_quieting_changes_only_signalling_nans():
    v = np.array(C.NANS + [1.0, C.INF, -0.0, C.TINY])
    q = _quieted(v)
    changed = v.view(np.uint64) != q.view(np.uint64)
    assert changed.tolist() == [False, False, True, False, False] + [False] * 4
    assert np.isnan(q[:5]).all()


def test_acero_on_a_signalling_nan_as_observed():
    """What _quieted works round, pinned as seen (pyarrow 25): beside a
    signalling NaN that follows -inf Acero's MIN/MAX give NaN (in the
    other order, {sNaN, 3.0}, they gave 3.0), beside its quiet twin they
    skip it. If an upgrade changes the first line, _quieted can go and the
    cross-check can feed Acero the raw patterns."""
    snan = C.f64(0x7FF0000000000001)
    for vals, quiet in (([-C.INF, snan], False),
                        (_quieted([-C.INF, snan]).tolist(), True)):
        t = pa.table({"g": pa.array([0, 0], type=pa.int64()),
                      "v": pa.array(np.array(vals, dtype=np.float64))})
        out = t.group_by("g").aggregate([("v", "min"), ("v", "max")])
        lo = out.column("v_min").to_pylist()[0]
        hi = out.column("v_max").to_pylist()[0]
        if quiet:
            assert lo == -C.INF and hi == -C.INF
        else:
            assert math.isnan(lo) and math.isnan(hi), (vals, lo, hi)


def _acero(case, c):
    """-> {op: list [ngroups]} of Acero's min / max / sum over column c."""
    t = pa.table({"g": pa.array(case.gids, type=pa.int64()),
                  "v": pa.array(_quieted(case.cols[c]))})
    out = t.group_by("g").aggregate([("v", "min"), ("v", "max"),
                                     ("v", "sum")])
    by = {g: i for i, g in enumerate(out.column("g").to_pylist())}
    res = {}
    for op in (C.SUM, C.MIN, C.MAX):
        col = out.column("v_" + C.OP_NAMES[op]).to_pylist()
        res[op] = [col[by[g]] for g in range(case.ngroups)]
    return res


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_agrees_with_acero(case):
    for c in range(len(case.cols)):
        got = _acero(case, c)
        rows = C.group_rows(case.gids, case.cols[c], case.ngroups)
        for op in (C.SUM, C.MIN, C.MAX):
            want = C.reference(case.gids, case.cols[c], case.ngroups, op)
            for g in range(case.ngroups):
                # Acero's own sum is one more summation order: it is held
                # to the same bound as the kernels wherever fsum is not
                # exact, and to equality where it is
                bound = C.case_bound(case, c, rows[g], op)
                assert C.same(got[op][g], want[g], bound), (
                    case.name, c, C.OP_NAMES[op], g, got[op][g], want[g])


def test_null_beside_nan_like_acero():
    gids, col, mask, ngroups = C.null_nan_case()
    t = pa.table({"g": pa.array(gids, type=pa.int64()),
                  "v": pa.array(np.array(col), mask=~np.array(mask))})
    out = t.group_by("g").aggregate([("v", "min"), ("v", "max"),
                                     ("v", "sum")])
    by = {g: i for i, g in enumerate(out.column("g").to_pylist())}
    for op in (C.SUM, C.MIN, C.MAX):
        want = C.reference(gids, col, ngroups, op, mask, null_values=True)
        got = out.column("v_" + C.OP_NAMES[op]).to_pylist()
        for g in range(4):                   # group 4 has no row at all
            assert C.same(got[by[g]], want[g]), (op, g, got[by[g]], want[g])
        assert want[4] is None
    mn = C.reference(gids, col, ngroups, C.MIN, mask, null_values=True)
    assert math.isnan(mn[0]) and mn[1] is None and mn[2] == 2.0 \
        and mn[3] is None


def test_reference_rules():
    nan, inf = C.NAN, C.INF
    assert math.isnan(C.ref_sum([1.0, nan]))
    assert math.isnan(C.ref_sum([inf, -inf]))
    assert C.ref_sum([inf, 1.0, inf]) == inf and C.ref_sum([-inf]) == -inf
    assert C.ref_sum([]) == 0.0
    assert C.ref_min([nan, 1.0]) == 1.0 and C.ref_max([nan, 1.0]) == 1.0
    assert math.isnan(C.ref_min([nan, nan])) and math.isnan(C.ref_max([nan]))
    assert C.ref_min([]) == inf and C.ref_max([]) == -inf
    assert C.ref_min([nan, inf]) == inf and C.ref_max([-inf, nan]) == -inf
    assert len(C.NANS) == 5 and all(x != x for x in C.NANS)
    assert C.same(-0.0, 0.0) and not C.same(1.0, nan) and C.same(nan, nan)
    assert not C.same(None, 0.0) and C.same(None, None)


# ---- facts about the case data -----------------------------------------------
def test_exact_family_is_exact_in_any_order():
    """Every value is an integer multiple of 0.25 and the magnitudes of a
    whole table sum below 2**53 quarter-units: every partial sum in any
    order is representable, so a dropped or doubled row changes the bits."""
    tables = [(c, None) for c in C.exact_cases()]
    tables += [(c, 0) for c in C.hot_cases() if c.name == "hot_exact"]
    for case, only in tables:       # of hot_exact, the hot group's rows
        for col in case.cols:
            rows = [x for g, x in zip(case.gids, col) if only in (None, g)]
            assert len(rows) >= 1000
            assert all(x * 4 == int(x * 4) for x in rows)
            assert sum(abs(int(x * 4)) for x in rows) < 2 ** 53


def test_q1_q6_products_are_exact():
    t = C.q1_case(1500, 512)
    for i in range(1500):
        p, d, x = (t["l_extendedprice"][i], t["l_discount"][i],
                   t["l_tax"][i])
        if not math.isfinite(p):
            continue
        dp = p * (1.0 - d)
        assert Fraction(dp) == Fraction(p) * (1 - Fraction(d))
        assert Fraction(dp * (1.0 + x)) == Fraction(dp) * (1 + Fraction(x))
    want = C.q1_reference(t)
    assert all(math.isnan(want[1][j]) for j in (1, 2, 3))
    assert all(math.isfinite(v) for v in want[2]) and want[2][5] > 0
    assert want[3][:4] == [0.0] * 4 and want[3][5] == 1.0
    assert all(math.isnan(want[4][j]) for j in (1, 2, 3)) and want[4][5] == 2
    assert want[5] == [0.0] * 6
    assert any(x != x for i, x in enumerate(t["l_extendedprice"])
               if t["l_returnflag"][i] * 2 + t["l_linestatus"][i] == 2)
    for kind, nan in (("exact", False), ("nan_pass", True),
                      ("nan_fail", False), ("inf_pair", True),
                      ("nzero", False)):
        q = C.q6_case(257, kind)
        rev, cnt = C.q6_reference(q)
        assert math.isnan(rev) == nan and cnt > 0, kind
    assert any(x != x for x in C.q6_case(257, "nan_fail")["l_extendedprice"])
    assert C.q6_reference(C.q6_case(257, "nzero"))[0] == 0.0


def test_cancel_bound_sees_one_row_and_an_fp32_accumulate():
    (case,) = C.cancel_cases()
    for c, col in enumerate(case.cols):
        for rows in C.group_rows(case.gids, col, case.ngroups):
            n = len(rows)
            assert 8 <= n <= 4096
            assert all(1.0 <= abs(x) <= 2.0 ** 20 for x in rows)
            bound = C.sum_bound(rows)
            mag = math.fsum(abs(x) for x in rows)
            # below the smallest |x|: one lost or doubled row fails it
            assert bound < min(abs(x) for x in rows)
            # 2**13 times tighter than one fp32 rounding of the magnitude
            # an fp32 accumulate carries (u32 = 2**-24)
            assert bound * 2 ** 13 <= 2.0 ** -24 * mag
            if c == 0:
                assert abs(math.fsum(rows)) <= 2.0, "the true sum is near 0"
    # Q1's charge: price*(1-disc)*(1+tax) holds at most 4 roundings
    assert C.gamma(4095 + 4) * 4096 * 2.0 ** 20 < 1.0


def test_subnormal_family_is_exact():
    (case,) = C.subnormal_cases()
    for col in case.cols:
        for rows in C.group_rows(case.gids, col, case.ngroups):
            assert Fraction(math.fsum(rows)) == sum(Fraction(x) for x in rows)
            assert any(0 < abs(x) < 2.2250738585072014e-308 for x in rows)
    want = C.reference(case.gids, case.cols[0], case.ngroups, C.SUM)
    assert want[:3] == [C.TINY, 16 * C.TINY, 1024 * C.TINY]
    assert all(w != 0.0 for w in want[:3])


def test_hot_family_shape():
    for case in C.hot_cases():
        sizes = [len(r) for r in C.group_rows(case.gids, case.cols[0],
                                              case.ngroups)]
        assert sizes == [C.HOT_ROWS] + [1] * C.HOT_OTHERS
    want = {c.name: C.reference(c.gids, c.cols[0], c.ngroups, C.MIN)[0]
            for c in C.hot_cases()}
    assert math.isnan(want["hot_all_nan"])
    assert math.isfinite(want["hot_nan_mixed"])


# ---- host ends: NaN beside NULL in the order-by -----------------------------
def _sorted_like_acero(vals, valid, direction):
    g = np.arange(len(vals), dtype=np.int64)
    t = pa.table({"g": g, "a": pa.array(vals, mask=~valid)})
    return t.sort_by([("a", direction + "ending"), ("g", "ascending")])


NAN_NULL_VALS = np.array([C.NAN, 2.0, 7.0, C.NAN, -1.0, C.INF, -C.INF, 0.0])
NAN_NULL_VALID = np.array([True, True, False, True, True, True, True, False])


@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_agg_final_columns_order_nan_then_null(direction):
    """A MIN alias holding NaN (an all-NaN group), finite values and NULL:
    numbers, then NaN, then NULL, in both directions, as Acero's sort_by
    with nulls at the end."""
    from quokka_amd.executors import GPUAggExecutor, _to_table
    ex = GPUAggExecutor(["g"], [("lo", direction), ("g", "asc")],
                        "min(a) as lo", device_keys=True, null_values=True)
    g = np.arange(len(NAN_NULL_VALS), dtype=np.int64)
    out, _ = ex._final_columns({"g": g}, {"a": NAN_NULL_VALS.copy()},
                               {"a": NAN_NULL_VALID})
    got = _to_table(out)
    want = _sorted_like_acero(NAN_NULL_VALS, NAN_NULL_VALID, direction)
    assert got.column("g").to_pylist() == want.column("g").to_pylist()
    lo = got.column("lo").to_pylist()
    assert lo[-2:] == [None, None] and all(math.isnan(x) for x in lo[-4:-2])


@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_agg_order_by_nan_without_masks(direction):
    """The default path has no NULLs: NaN sorts last both ways."""
    from quokka_amd.executors import GPUAggExecutor
    ex = GPUAggExecutor(["g"], [("lo", direction), ("g", "asc")],
                        "min(a) as lo")
    g = np.arange(len(NAN_NULL_VALS), dtype=np.int64)
    order = ex._order_by({"g": g, "lo": NAN_NULL_VALS})
    allv = np.ones(len(g), dtype=bool)
    want = _sorted_like_acero(NAN_NULL_VALS, allv, direction)
    assert g[order].tolist() == want.column("g").to_pylist()


@pytest.mark.parametrize("direction", ["asc", "desc"])
@pytest.mark.parametrize("k", [3, 6, 8])
def test_topk_orders_nan_before_null(direction, k):
    from quokka_amd.executors import GPUTopKExecutor
    g = np.arange(len(NAN_NULL_VALS), dtype=np.int64)
    t = pa.table({"g": g, "a": pa.array(NAN_NULL_VALS,
                                        mask=~NAN_NULL_VALID)})
    ex = GPUTopKExecutor(["a", "g"], k, [direction == "desc", False])
    ex.execute([t.slice(0, 3), t.slice(3)], 0, 0)
    got = ex.done(0)
    want = _sorted_like_acero(NAN_NULL_VALS, NAN_NULL_VALID,
                              direction).slice(0, k)
    assert got.column("g").to_pylist() == want.column("g").to_pylist()
