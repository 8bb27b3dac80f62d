"""Float edge values through every aggregate path on the device, against
the plain-Python reference of tests/_float_agg_cases.py (math.fsum; the
rules of pyarrow Acero, cross-checked in test_float_agg_cases_cpu.py):
SUM with a NaN is NaN, inf + -inf is NaN, MIN/MAX skip NaN beside other
values and an all-NaN MIN/MAX is NaN; exact families bit for bit, the
cancelling sums within gamma(n-1+k) * sum|term|, subnormals never flushed.

Paths: k_groupby_sum (ops.GroupByI64: one update, uneven updates, across a
growth), both twins of k_groupby_dense_acc (ops.DenseAcc / GroupByKeys),
the HAVING extract, the JIT aggregate (grouped and grand, column and
product), qk_q1_agg (streaming and row-pair kernels), qk_q6_agg, the fused
Q3/Q5 probe-aggregates, and GPUAggExecutor end to end against Acero."""
import ctypes
import math

import numpy as np
import pytest

import _float_agg_cases as C

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu

OPS3 = [C.SUM, C.MIN, C.MAX]
CASES = C.all_cases()
CASE_IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _dev(shim, values, dtype=np.float64):
    return shim.DevColumn.from_numpy(np.array(values, dtype=dtype))


def _free(*cols):
    for c in cols:
        if isinstance(c, dict):
            c = list(c.values())
        for d in (c if isinstance(c, (list, tuple)) else [c]):
            d.free()


def _want(case, c, null_values=False, mask=None):
    """-> ({op: list [ngroups]}, {op: bounds [ngroups]}) for column c."""
    rows = C.group_rows(case.gids, case.cols[c], case.ngroups, mask)
    want = {op: C.reference(case.gids, case.cols[c], case.ngroups, op, mask,
                            null_values) for op in OPS3}
    bound = {op: [C.case_bound(case, c, r, op) for r in rows] for op in OPS3}
    return want, bound


def _assert_case(case, got, what):
    """got[c][op] -> sequence [ngroups] of floats (or None)."""
    bad = []
    for c in range(len(case.cols)):
        want, bound = _want(case, c)
        for op in OPS3:
            for g in range(case.ngroups):
                if not C.same(got[c][op][g], want[op][g], bound[op][g]):
                    bad.append((c, C.OP_NAMES[op], g, got[c][op][g],
                                want[op][g]))
    assert not bad, (what, case.name, bad[:8], len(bad))


# ---- 1. k_groupby_sum through ops.GroupByI64 --------------------------------
def _groupby_i64(shim, case, splits, expected_groups):
    """SUM/MIN/MAX of every column in ONE record (nvals = 3 * ncols), the
    rows fed in the given row splits. Keys are 7 * gid - 11."""
    from quokka_amd import ops
    ncols = len(case.cols)
    gb = ops.GroupByI64(expected_groups, 3 * ncols, agg_ops=OPS3 * ncols)
    cap0 = gb.cap
    lo = 0
    for hi in list(splits) + [len(case.gids)]:
        k = _dev(shim, [7 * g - 11 for g in case.gids[lo:hi]], np.int64)
        vs = [_dev(shim, col[lo:hi]) for col in case.cols]
        gb.update(k, [v for v in vs for _ in OPS3], hi - lo)
        _free(k, vs)
        lo = hi
    keys, sums = gb.extract()
    grew = gb.cap > cap0
    gb.free()
    assert sorted(keys.tolist()) == [7 * g - 11 for g in range(case.ngroups)]
    at = {int(k): j for j, k in enumerate(keys.tolist())}
    got = [{op: [sums[3 * c + i][at[7 * g - 11]]
                 for g in range(case.ngroups)]
            for i, op in enumerate(OPS3)} for c in range(ncols)]
    return got, sums[:, [at[7 * g - 11] for g in range(case.ngroups)]], grew


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_groupby_i64_families(gpu, case):
    got, _, _ = _groupby_i64(gpu, case, [], 8192)
    _assert_case(case, got, "GroupByI64")


@pytest.mark.parametrize("case", C.exact_cases() + C.special_cases()
                         + C.hot_cases(), ids=lambda c: c.name)
def test_groupby_i64_updates_and_growth_agree(gpu, case):
    """One update, three uneven updates (one of them empty) and a run that
    crosses a _grow give the same bits under `exact` and the same answer
    under the contract everywhere."""
    n = len(case.gids)
    one, raw1, g1 = _groupby_i64(gpu, case, [], 8192)
    three, raw3, g3 = _groupby_i64(gpu, case, [n // 7, n // 7, n - 5], 8192)
    grown, rawg, gg = _groupby_i64(gpu, case, [3, n // 2], 2)
    assert not g1 and not g3 and gg, "only the last run grows its table"
    for got, what in ((three, "3 updates"), (grown, "across _grow")):
        _assert_case(case, got, what)
    if case.family == "exact" or case.name == "hot_exact":
        hot = slice(0, 1) if case.family == "hot" else slice(None)
        assert raw1[:, hot].tobytes() == raw3[:, hot].tobytes() \
            == rawg[:, hot].tobytes()


# ---- 2. k_groupby_dense_acc, both twins -------------------------------------
def _dense(shim, case, nullable, masks=None, capacity=4):
    """ops.DenseAcc over the group ids as codes -> (got, valid or None).
    capacity 4 makes every multi-group case cross _grow_acc."""
    from quokka_amd import ops
    ncols = len(case.cols)
    acc = ops.DenseAcc(3 * ncols, OPS3 * ncols, capacity=capacity,
                       nullable_vals=nullable)
    codes = _dev(shim, case.gids, np.uint32)
    vs = [_dev(shim, col) for col in case.cols]
    kw = {}
    if masks is not None:
        kw["val_valid"] = [np.array(m, dtype=bool) for m in masks
                           for _ in OPS3]
    acc.accumulate(codes, case.ngroups, [v for v in vs for _ in OPS3],
                   len(case.gids), **kw)
    sums = acc.extract(case.ngroups)
    valid = acc.extract_valid(case.ngroups) if nullable else None
    acc.free()
    _free(codes, vs)
    got = [{op: sums[3 * c + i].tolist() for i, op in enumerate(OPS3)}
           for c in range(ncols)]
    return got, valid


@pytest.mark.parametrize("nullable", [False, True], ids=["plain", "valid"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dense_acc_families(gpu, case, nullable):
    got, valid = _dense(gpu, case, nullable)
    _assert_case(case, got, "DenseAcc nullable=%r" % nullable)
    if nullable:
        assert valid.all(), "every group met a value in every column"


def test_dense_acc_null_beside_nan(gpu):
    """{NULL, NaN}: MIN/MAX NaN and not NULL. {NULL}: NULL, identity under
    it. A NaN under a 0 validity bit is never read. A code without rows
    keeps the identities."""
    gids, col, mask, ngroups = C.null_nan_case()
    case = C.Case("null_nan", "special", gids, [col], ngroups, None)
    got, valid = _dense(gpu, case, True, masks=[mask])
    want, _ = _want(case, 0, null_values=True, mask=mask)
    ident = {C.SUM: 0.0, C.MIN: C.INF, C.MAX: -C.INF}
    for i, op in enumerate(OPS3):
        for g in range(ngroups):
            w = want[op][g]
            assert bool(valid[i][g]) == (w is not None), (op, g)
            have = got[0][op][g]
            assert C.same(have, ident[op] if w is None else w), (op, g, have)
    assert math.isnan(got[0][C.MIN][0]) and valid[1][0]
    assert got[0][C.MIN][1] == C.INF and not valid[1][1]


def test_groupby_keys_special_and_hot(gpu):
    """ops.GroupByKeys (dictionary codes, then the dense accumulate) over
    three uneven updates, nullable_vals off and on."""
    from quokka_amd import ops
    for case in C.special_cases() + C.hot_cases():
        n = len(case.gids)
        for nullable in (False, True):
            gb = ops.GroupByKeys(1, 3, agg_ops=OPS3, expected_groups=4,
                                 nullable_vals=nullable)
            for lo, hi in ((0, 5), (5, 5), (5, n // 2), (n // 2, n)):
                k = _dev(gpu, [1000 - g for g in case.gids[lo:hi]], np.int64)
                v = _dev(gpu, case.cols[0][lo:hi])
                gb.update([k], [v, v, v], hi - lo)
                _free(k, v)
            (keys,), sums = gb.extract()
            if nullable:
                assert gb.extract_vals_valid().all()
            gb.free()
            at = {int(k): j for j, k in enumerate(keys.tolist())}
            got = {op: [sums[i][at[1000 - g]] for g in range(case.ngroups)]
                   for i, op in enumerate(OPS3)}
            one = C.Case(case.name, case.family, case.gids, case.cols[:1],
                         case.ngroups, None)
            _assert_case(one, [got], "GroupByKeys nullable=%r" % nullable)


# ---- 3. HAVING: extract_where_gt --------------------------------------------
def test_extract_where_gt_nan_inf_zero(gpu):
    """A group qualifies exactly where Python's v > t is true: never with
    a NaN on either side, and -0.0 > 0.0 is false."""
    from quokka_amd import ops
    vals = C.GT_VALUES
    gb = ops.GroupByI64(64, 2, agg_ops=[C.SUM, C.MAX])
    k = _dev(gpu, list(range(len(vals))), np.int64)
    v = _dev(gpu, vals)
    gb.update(k, [v, v], len(vals))
    _free(k, v)
    for col in (0, 1):
        for t in C.GT_THRESHOLDS:
            keys, sums = gb.extract_where_gt(col, t)
            want = sorted(i for i, x in enumerate(vals) if x > t)
            assert sorted(keys.tolist()) == want, (col, t)
            for j, key in enumerate(keys.tolist()):
                assert sums[col][j] == vals[key]
    gb.free()


# ---- 4. the JIT aggregate ---------------------------------------------------
JIT_AGGS = ["sum(x) as s", "min(x) as lo", "max(x) as hi", "count(*) as n",
            "sum(x * f) as sp", "min(x * f) as lp", "max(x * f) as hp"]


@pytest.fixture(scope="module")
def jit_programs(gpu):
    """Two compiled programs for the whole file: grouped and grand, both
    with the predicate `keep > 0`."""
    from quokka_amd import jit
    schema = {"g": np.dtype(np.uint8), "x": np.dtype(np.float64),
              "f": np.dtype(np.float64), "keep": np.dtype(np.int32)}
    grouped = jit.JitAggregate(schema, [("g", 16)], JIT_AGGS[:4],
                               predicate="keep > 0")
    grand = jit.JitAggregate(schema, [], JIT_AGGS, predicate="keep > 0")
    yield grouped, grand
    grouped.free()
    grand.free()


def _jit_run(shim, agg, g, x, f, keep):
    cols = {"g": _dev(shim, g, np.uint8), "x": _dev(shim, x),
            "f": _dev(shim, f), "keep": _dev(shim, keep, np.int32)}
    acc = agg.make_acc()
    agg.run({c: cols[c] for c in agg.cols}, acc)
    shim.call("qk_stream_sync", None)
    got = agg.read(acc)
    acc.free()
    _free(cols)
    return got


@pytest.mark.parametrize("case", [c for c in CASES if c.ngroups <= 14],
                         ids=lambda c: c.name)
def test_jit_grouped(gpu, jit_programs, case):
    """Group ngroups holds rows the predicate removes, every one of them a
    NaN or an infinity: it reads back untouched, 0 / +inf / -inf / 0.
    Group 15 has no row at all."""
    grouped, _ = jit_programs
    dead = case.ngroups
    extra = [C.NAN, C.INF, -C.INF] * 100
    g = list(case.gids) + [dead] * len(extra)
    x = list(case.cols[0]) + extra
    keep = [1] * len(case.gids) + [0] * len(extra)
    got = _jit_run(gpu, grouped, g, x, [1.0] * len(g), keep)
    one = C.Case(case.name, case.family, case.gids, case.cols[:1],
                 case.ngroups, None)
    _assert_case(one, [{op: got[:, i].tolist() for i, op in
                        enumerate(OPS3)}], "JitAggregate grouped")
    counts = [len(r) for r in C.group_rows(case.gids, case.cols[0],
                                           case.ngroups)]
    assert got[:case.ngroups, 3].tolist() == counts
    for gid in (dead, 15):
        assert got[gid].tolist() == [0.0, C.INF, -C.INF, 0.0], gid


def _grand_tables():
    """(name, x, f): one group each, the product x * f exact (f from
    {0.25, 0.5}; 0 is left to `zero_factor`, where NaN * 0 is NaN)."""
    out = []
    for case in C.exact_cases() + C.subnormal_cases():
        out.append((case.name, case.cols[0], None))
    for name, vals in C.special_groups():
        out.append((name, vals, None))
    hot = C.hot_cases()[1]
    out.append((hot.name, hot.cols[0], None))
    out.append(("zero_factor", [C.NAN, 1.0, 2.0], [0.0, 0.0, 0.5]))
    return out


@pytest.mark.parametrize("name,x,f", _grand_tables(),
                         ids=[t[0] for t in _grand_tables()])
def test_jit_grand(gpu, jit_programs, name, x, f):
    _, grand = jit_programs
    if f is None:
        f = [(0.25, 0.5)[i % 2] for i in range(len(x))]
    if name == "subnormal":
        f = [1.0] * len(x)        # 5e-324 * 0.25 rounds; keep products exact
    # removed rows: specials the predicate must keep out
    xs = list(x) + [C.NAN, C.INF, -C.INF]
    fs = list(f) + [1.0, 1.0, 1.0]
    keep = [1] * len(x) + [0, 0, 0]
    got = _jit_run(gpu, grand, [0] * len(xs), xs, fs, keep)[0]
    prod = [a * b for a, b in zip(x, f)]
    want = [C.ref_sum(x), C.ref_min(x), C.ref_max(x), float(len(x)),
            C.ref_sum(prod), C.ref_min(prod), C.ref_max(prod)]
    for j, w in enumerate(want):
        assert C.same(got[j], w), (name, JIT_AGGS[j], got[j], w)


def test_jit_grand_removes_every_row(gpu, jit_programs):
    _, grand = jit_programs
    got = _jit_run(gpu, grand, [0] * 5, [C.NAN, 1.0, C.INF, -C.INF, 2.0],
                   [1.0] * 5, [0] * 5)[0]
    assert got.tolist() == [0.0, C.INF, -C.INF, 0.0, 0.0, C.INF, -C.INF]


def test_jit_null_beside_nan(gpu):
    """The nullable= path (third compiled program): a NULL input is spelt
    as the no-input pattern inside the kernel. {NULL, NaN}: MIN/MAX NaN.
    {NULL}: the identity, COUNT(x) 0. {NULL, NaN, 2.0}: 2.0. A group whose
    only row is NULL, and one without rows, read the identity."""
    from quokka_amd import jit, ops
    gids, col, mask, ngroups = C.null_nan_case()
    schema = {"g": np.dtype(np.uint8), "x": np.dtype(np.float64)}
    agg = jit.JitAggregate(schema, [("g", 8)],
                           ["sum(x) as s", "min(x) as lo", "max(x) as hi",
                            "count(x) as n", "min(x * 2) as lp"],
                           nullable=["x"])
    cols = {"g": _dev(gpu, gids, np.uint8),
            "x": ops.NullableColumn.from_numpy(np.array(col), mask)}
    acc = agg.make_acc()
    agg.run(cols, acc)
    gpu.call("qk_stream_sync", None)
    got = agg.read(acc)
    acc.free()
    cols["g"].free()
    cols["x"].free()
    agg.free()
    ident = {C.SUM: 0.0, C.MIN: C.INF, C.MAX: -C.INF}
    for j, op in enumerate(OPS3):
        want = C.reference(gids, col, ngroups, op, mask, null_values=True)
        for g in range(8):
            w = want[g] if g < ngroups else None
            assert C.same(got[g][j], ident[op] if w is None else w), \
                (C.OP_NAMES[op], g, got[g][j], w)
    rows = C.group_rows(gids, col, ngroups, mask)
    assert got[:ngroups, 3].tolist() == [float(len(r)) for r in rows]
    assert math.isnan(got[0][1]) and math.isnan(got[0][2]) \
        and math.isnan(got[0][4])
    assert got[1][1] == C.INF and got[2][4] == 4.0


# ---- 5. Q1 and Q6 -----------------------------------------------------------
Q1_COLS = [("l_shipdate", np.int32), ("l_quantity", np.float64),
           ("l_extendedprice", np.float64), ("l_discount", np.float64),
           ("l_tax", np.float64), ("l_returnflag", np.uint8),
           ("l_linestatus", np.uint8)]


def _addr(col):
    p = col.ptr
    return int(getattr(p, "value", p) or 0)


def _q1_shape():
    from test_gpu_q1_stream import _shape
    return _shape()


@pytest.mark.parametrize("size", ["T+1", "G+1"])
@pytest.mark.parametrize("path", ["stream", "rowpair"])
def test_q1_float_edges(gpu, size, path):
    """Exact data on all six accumulators: counts and every finite sum bit
    for bit. The row-pair kernel is reached with a misaligned view of rows
    1.. of a table that holds one junk row in front."""
    from quokka_amd import ops, queries
    T, G = _q1_shape()
    n = T + 1 if size == "T+1" else G + 1
    t = C.q1_case(n, T)
    want = C.q1_reference(t)
    off = 1 if path == "rowpair" else 0
    dev = {k: _dev(gpu, [t[k][0]] * off + t[k], dt) for k, dt in Q1_COLS}
    cols = {k: d.view(off, n) for k, d in dev.items()}
    # qk_q1_agg's own dispatch test: any f64 pointer off 16 B, shipdate off
    # 8 B or a flag pointer off 2 B takes k_q1_agg_rowpair
    f64_names = ("l_quantity", "l_extendedprice", "l_discount", "l_tax")
    mis = any(_addr(cols[k]) & 15 for k in f64_names) \
        or _addr(cols["l_shipdate"]) & 7 \
        or any(_addr(cols[k]) & 1 for k in ("l_returnflag", "l_linestatus"))
    assert bool(mis) == (path == "rowpair"), "the view reaches the other kernel"
    # where +inf (row 0) and -inf (row T) meet: at T+1 inside one block
    # (stream: block 0's tile and its tail row; row-pair: pair 0 and the odd
    # tail of thread 0). At G+1 in two blocks: the streaming grid is G / T
    # resident blocks with tile b in block b, the row-pair grid gives pair
    # 256 = rows T, T+1 to block 1.
    if size == "G+1":
        assert G // T >= 2 and G % T == 0
        assert T // 2 == int(gpu._lib.qk_block_threads())
        assert min(int(gpu._lib.qk_max_blocks()), (n // 2) // (T // 2)) >= 2
    else:
        assert n // T == 1 and (n // 2) // (T // 2) == 1
    acc = queries.q1_partials_device(cols, cutoff=C.Q1_CUTOFF)
    got = ops.q1_read_partials(acc)
    acc.free()
    _free(dev)
    bad = [(g, j, got[g][j], want[g][j]) for g in range(6) for j in range(6)
           if not C.same(got[g][j], want[g][j])]
    assert not bad, bad
    assert math.isnan(got[1][1]) and math.isfinite(got[2][1])
    assert math.isnan(got[4][1]) and got[3][5] == 1.0 and got[3][1] == 0.0


@pytest.mark.parametrize("kind", ["exact", "nan_pass", "nan_fail",
                                  "inf_pair", "nzero"])
def test_q6_float_edges(gpu, kind):
    from quokka_amd import ops
    n = int(gpu._lib.qk_block_threads()) + 1
    t = C.q6_case(n, kind)
    dev = {"l_shipdate": _dev(gpu, t["l_shipdate"], np.int32),
           "l_quantity": _dev(gpu, t["l_quantity"]),
           "l_extendedprice": _dev(gpu, t["l_extendedprice"]),
           "l_discount": _dev(gpu, t["l_discount"])}
    out = _dev(gpu, [0.0, 0.0])
    q = C.Q6
    ops.q6_agg(n, dev["l_shipdate"], dev["l_quantity"],
               dev["l_extendedprice"], dev["l_discount"], q["date_lo"],
               q["date_hi"], q["disc_lo"], q["disc_hi"], q["qty_hi"], out)
    gpu.call("qk_stream_sync", None)
    rev, cnt = out.to_numpy(2).tolist()
    _free(dev, out)
    wrev, wcnt = C.q6_reference(t)
    assert cnt == wcnt and C.same(rev, wrev), (kind, rev, wrev, cnt, wcnt)


# ---- 6. fused Q3 / Q5 probe-aggregates --------------------------------------
@pytest.fixture(scope="module")
def probe_world(gpu):
    """The tables of test_gpu_probe_variants.py, 300 lineitem rows, with a
    NaN price in one row that matches both builds and in one that matches
    neither."""
    import test_gpu_probe_variants as PV
    from quokka_amd import staging, queries as DQ
    cust, orders, supp, li = PV._tables()
    n = 300
    li = {k: v[:n].copy() for k, v in li.items()}
    building = set(cust["c_custkey"][cust["c_mktsegment"] == DQ.MKT_BUILDING])
    cnat = dict(zip(cust["c_custkey"], cust["c_nationkey"]))
    snat = dict(zip(supp["s_suppkey"], supp["s_nationkey"]))
    both = [i for i in range(64)
            if orders["o_custkey"][i] in building
            and orders["o_orderdate"][i] < DQ.Q3_DATE
            and DQ.Q5_LO <= orders["o_orderdate"][i] < DQ.Q5_HI
            and cnat[orders["o_custkey"][i]] in PV.ASIA]
    hit = both[0]
    hit_key = orders["o_orderkey"][hit]
    hit_supp = [k for k, v in snat.items()
                if v == cnat[orders["o_custkey"][hit]]][0]
    PV._force_head_rows(li, hit_key, hit_supp, hit_key + 1, DQ.Q3_DATE)
    li["l_extendedprice"][4] = C.NANS[1]      # row 4 hits both builds
    li["l_extendedprice"][2] = C.NANS[2]      # row 2 misses both
    q3_build = {k for k, c, d in zip(orders["o_orderkey"],
                                     orders["o_custkey"],
                                     orders["o_orderdate"])
                if c in building and d < DQ.Q3_DATE}
    q5_build = {k: cnat[c] for k, c, d in zip(orders["o_orderkey"],
                                              orders["o_custkey"],
                                              orders["o_orderdate"])
                if cnat[c] in PV.ASIA and DQ.Q5_LO <= d < DQ.Q5_HI}
    rev = [p * (1.0 - d) for p, d in zip(li["l_extendedprice"].tolist(),
                                         li["l_discount"].tolist())]
    q3_want, q5_want = {}, {}
    for i in range(n):
        k, s = int(li["l_orderkey"][i]), int(li["l_suppkey"][i])
        if k in q3_build and li["l_shipdate"][i] > DQ.Q3_DATE:
            q3_want.setdefault(k, []).append(rev[i])
        if q5_build.get(k, -1) == snat[s]:
            q5_want.setdefault(int(snat[s]), []).append(rev[i])
    ocols, ccols, scols = (staging.stage_columns(t)
                           for t in (orders, cust, supp))
    q3, q5 = DQ.Q3Fused(ocols, ccols), DQ.Q5Fused(ocols, ccols, scols)
    yield {"li": li, "q3": q3, "q5": q5, "hit_key": int(hit_key),
           "hit_nat": int(cnat[orders["o_custkey"][hit]]),
           "q3_want": {k: C.ref_sum(v) for k, v in q3_want.items()},
           "q5_want": {k: C.ref_sum(v) for k, v in q5_want.items()}}
    q3.free()
    q5.free()
    _free(ocols, ccols, scols)


def test_q3_probe_twins_nan(gpu, probe_world):
    from quokka_amd import ops, staging
    w = probe_world
    assert math.isnan(w["q3_want"][w["hit_key"]])
    assert sum(1 for v in w["q3_want"].values() if v != v) == 1
    raw = []
    for nt in (False, True, 4):
        lcols = staging.stage_columns({k: w["li"][k] for k in (
            "l_orderkey", "l_shipdate", "l_extendedprice", "l_discount")})
        mc = ops._count_buf()
        w["q3"].reset_sums()
        w["q3"].probe(lcols, mc, nt=nt)
        full, _ = w["q3"].extract()
        mc.free()
        _free(lcols)
        got = dict(zip(full["l_orderkey"].tolist(), full["revenue"].tolist()))
        assert set(got) == set(w["q3_want"]), nt
        bad = [(k, got[k], v) for k, v in w["q3_want"].items()
               if not C.same(got[k], v)]
        assert not bad, (nt, bad)
        order = np.argsort(full["l_orderkey"])
        finite = np.isfinite(full["revenue"][order])
        raw.append(full["revenue"][order][finite].tobytes())
    assert raw[0] == raw[1] == raw[2], "the twins agree bit for bit"


def test_q5_probe_twins_nan(gpu, probe_world):
    from quokka_amd import ops, staging
    w = probe_world
    assert math.isnan(w["q5_want"][w["hit_nat"]])
    assert any(v == v for v in w["q5_want"].values())
    raw = []
    for nt in (False, True):
        lcols = staging.stage_columns({k: w["li"][k] for k in (
            "l_orderkey", "l_suppkey", "l_extendedprice", "l_discount")})
        mc = ops._count_buf()
        got = np.zeros(32)
        w["q5"].reset_sums()
        w["q5"].probe(lcols, mc, nt=nt)
        gpu.call("qk_d2h", got.ctypes.data_as(ctypes.c_void_p),
                 w["q5"].out25.ptr, ctypes.c_uint64(32 * 8))
        mc.free()
        _free(lcols)
        for nat in range(32):
            assert C.same(got[nat], w["q5_want"].get(nat, 0.0)), (nt, nat)
        raw.append(got[np.isfinite(got)].tobytes())
    assert raw[0] == raw[1], "the twins agree bit for bit"


# ---- 7. GPUAggExecutor against Acero ----------------------------------------
EXEC_CASES = C.special_cases() + C.hot_cases()
EXEC_PATHS = {"default": {}, "device_keys": {"device_keys": True},
              "null_values": {"device_keys": True, "null_values": True}}


def _exec_table(case):
    """Columns a, b, c are the same values: the default executor takes
    one function per column."""
    v = np.array(case.cols[0], dtype=np.float64)
    return pa.table({"g": pa.array(case.gids, type=pa.int64()),
                     "a": v, "b": v.copy(), "c": v.copy()})


@pytest.mark.parametrize("direction", ["asc", "desc"])
@pytest.mark.parametrize("path", list(EXEC_PATHS))
@pytest.mark.parametrize("case", EXEC_CASES, ids=lambda c: c.name)
def test_agg_executor_vs_acero(gpu, case, path, direction):
    """Values against the reference (which the CPU test holds to Acero),
    row order against Acero's sort_by on the MIN alias: numbers, then NaN
    groups, ties by key."""
    from quokka_amd.executors import GPUAggExecutor
    t = _exec_table(case)
    n = t.num_rows
    ex = GPUAggExecutor(["g"], [("lo", direction), ("g", "asc")],
                        "sum(a) as sa, min(b) as lo, max(c) as hi",
                        **EXEC_PATHS[path])
    for lo, hi in ((0, n // 3), (n // 3, n)):
        ex.execute([t.slice(lo, hi - lo)], 0, 0)
    out = ex.done(0)
    want = {op: C.reference(case.gids, case.cols[0], case.ngroups, op)
            for op in OPS3}
    gcol = out.column("g").to_pylist()
    assert sorted(gcol) == list(range(case.ngroups))
    for alias, op in (("sa", C.SUM), ("lo", C.MIN), ("hi", C.MAX)):
        col = out.column(alias).to_pylist()
        assert None not in col, "NaN is a value, not NULL"
        bad = [(g, v, want[op][g]) for g, v in zip(gcol, col)
               if not C.same(v, want[op][g])]
        assert not bad, (alias, bad[:6])
    order = pa.table({"g": pa.array(range(case.ngroups), type=pa.int64()),
                      "lo": pa.array(want[C.MIN], type=pa.float64())}
                     ).sort_by([("lo", direction + "ending"),
                                ("g", "ascending")])
    assert gcol == order.column("g").to_pylist()


@pytest.mark.parametrize("null_values", [False, True])
@pytest.mark.parametrize("case", EXEC_CASES, ids=lambda c: c.name)
def test_grand_aggregate_vs_reference(gpu, case, null_values):
    """Every group of the case as one grand aggregate of its own."""
    from quokka_amd.executors import GPUAggExecutor
    rows = C.group_rows(case.gids, case.cols[0], case.ngroups)
    for g in sorted({0, 1, 2, 3, 7, case.ngroups - 1}):
        if g >= case.ngroups:
            continue
        v = np.array(rows[g], dtype=np.float64)
        ex = GPUAggExecutor([], None,
                            "sum(a) as sa, min(b) as lo, max(c) as hi",
                            null_values=null_values)
        ex.execute([pa.table({"a": v, "b": v.copy(), "c": v.copy()})], 0, 0)
        out = ex.done(0)
        assert out.num_rows == 1
        for alias, op in (("sa", C.SUM), ("lo", C.MIN), ("hi", C.MAX)):
            got = out.column(alias).to_pylist()[0]
            assert C.same(got, C.REF[op](rows[g])), (g, alias, got)
