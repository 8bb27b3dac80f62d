"""GPU tier of the JIT semantics table (tests/_jit_cases.py) and the shape
edges of the generated kernels.

Table cases run through JitFilter / JitMap / JitAggregate and must give
the table's expected result (from the case's AST, never from the
translator). Shape tests sit where the generated kernels change path:
n = 0/1/2, the wave and block edges, 2048 * 256 = 524288 rows (the last
n with chunk = 256 in the filter grid; one more row steps chunk to 512
and leaves a ragged last block; the map and aggregate grids cap at 2048
blocks there, so 524288 + 257 rows take a second grid-stride trip).

Every program is built once per test function and reused across shapes."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jit_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 524288, 524289,
          524288 + 257]
AGG_SHAPES = [0, 1, 2, 3, 511, 512, 513, 524288 + 1]
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


@pytest.fixture(scope="module")
def table():
    by = {}
    for c in T.all_cases():
        if c.gpu:
            by.setdefault((c.family, c.kind), []).append(c)
    return by


def upload(cols):
    from quokka_amd.shim import DevColumn
    return {k: DevColumn.from_numpy(v) for k, v in cols.items()}


def free(cols):
    for c in cols.values():
        c.free()


def tiled(case, n):
    """The case's rows repeated to n rows: the expected result of a
    row-wise expression repeats with them."""
    return ({k: np.resize(v, n) for k, v in case.cols.items()},
            np.resize(case.expected, n))


def run_filter(f, dev, n):
    """Direct qk_jit_filter_run into a sentinel-filled index buffer ->
    (count, whole buffer)."""
    from quokka_amd import ops, shim
    from quokka_amd.shim import DevColumn, c_u64, c_vp
    idx = DevColumn.from_numpy(np.full(n + 8, SENTINEL, dtype=np.uint32))
    cnt = ops._count_buf()
    ptrs = (c_vp * len(f.cols))(*[dev[c].ptr for c in f.cols])
    lib = shim._lib
    lib.qk_jit_filter_run.argtypes = [c_vp, c_vp, c_u64,
                                      ctypes.POINTER(c_vp), c_vp, c_vp]
    rc = lib.qk_jit_filter_run(f.prog, None, c_u64(n), ptrs, idx.ptr,
                               cnt.ptr)
    assert rc == 0, lib.qk_jit_last_error().decode()
    k = ops._read_u64(cnt)
    got = idx.to_numpy(n + 8)
    cnt.free()
    idx.free()
    return k, got


def check_filter(f, dev, n, expected, what):
    k, buf = run_filter(f, dev, n)
    want = np.nonzero(expected)[0].astype(np.uint32)
    assert k == len(want), (what, k, len(want))
    assert np.array_equal(buf[:k], want), what          # order included
    assert (buf[k:] == SENTINEL).all(), what            # nothing past count


# ---- the table through JitFilter and JitMap -------------------------------

FILTER_FAMILIES = ["division", "width", "literal_edges", "precedence",
                   "contraction", "nan", "generated"]
MAP_FAMILIES = ["division", "width", "contraction", "generated"]


@pytest.mark.parametrize("family", FILTER_FAMILIES)
def test_table_filters(gpu, table, family):
    from quokka_amd import jit
    cases = table[(family, "filter")]
    assert cases
    for c in cases:
        f = jit.JitFilter(c.sql, c.schema)
        for n in (len(c.expected), 513):
            cols, want = tiled(c, n)
            dev = upload({k: cols[k] for k in f.cols})
            check_filter(f, dev, n, want, (c.name, c.sql, f.expr, n))
            free(dev)
        f.free()


@pytest.mark.parametrize("family", MAP_FAMILIES)
def test_table_maps(gpu, table, family):
    from quokka_amd import jit
    cases = table[(family, "map")]
    assert cases
    for c in cases:
        m = jit.JitMap(c.sql, c.schema)
        for n in (len(c.expected), 257):
            cols, want = tiled(c, n)
            dev = upload({k: cols[k] for k in m.cols})
            out = m.run(dev)
            got = out.to_numpy(n)
            assert T.canon(got).tobytes() == T.canon(want).tobytes(), \
                (c.name, c.sql, m.expr, n)
            out.free()
            free(dev)
        m.free()


# ---- filter shapes ---------------------------------------------------------

def selectivity_patterns(n, rng):
    i = np.arange(n)
    pats = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool),
            "first": i == 0, "last": i == n - 1, "every64": i % 64 == 0,
            "waves": (i // 64) % 2 == 0, "random": rng.random(n) < 0.5}
    return pats


def test_filter_shapes(gpu):
    """count + scan + scatter at every n where the grid changes, under
    seven selectivity patterns, for a u8/i32 and an f64/i64 program."""
    from quokka_amd import jit
    f1 = jit.JitFilter("s = 1 and a >= 0",
                       {"s": T.U8, "a": T.I32})
    f2 = jit.JitFilter("b > 0.5 or k + 1 < 0", {"b": T.F64, "k": T.I64})
    rng = np.random.default_rng(17)
    for n in SHAPES:
        a = upload({"a": np.arange(n, dtype=np.int32),
                    "k": np.zeros(n, dtype=np.int64)})
        for name, pat in selectivity_patterns(n, rng).items():
            d = upload({"s": pat.astype(np.uint8),
                        "b": pat.astype(np.float64)})
            check_filter(f1, {"s": d["s"], "a": a["a"]}, n, pat,
                         ("u8/i32", n, name))
            check_filter(f2, {"b": d["b"], "k": a["k"]}, n, pat,
                         ("f64/i64", n, name))
            free(d)
        free(a)
    f1.free()
    f2.free()


def test_filter_run_wrapper_shapes(gpu):
    """JitFilter.run (the public path) at the degenerate sizes."""
    from quokka_amd import jit
    f = jit.JitFilter("a * 2 >= 2", {"a": T.I32})
    for n in (0, 1, 2, 257):
        d = upload({"a": np.arange(n, dtype=np.int32)})
        idx, k = f.run(d)
        assert k == max(0, n - 1)
        assert np.array_equal(idx.to_numpy(k), np.arange(1, n))
        idx.free()
        free(d)
    f.free()


# ---- map shapes ------------------------------------------------------------

def test_map_shapes(gpu, table):
    """Bit-exact map output at every n; 524288 + 257 rows take a second
    trip through the grid-stride loop."""
    from quokka_amd import jit
    cases = [table[("contraction", "map")][0], table[("division", "map")][1],
             table[("width", "map")][0]]
    for c in cases:
        m = jit.JitMap(c.sql, c.schema)
        for n in SHAPES:
            cols, want = tiled(c, n)
            dev = upload({k: cols[k] for k in m.cols})
            out = m.run(dev)
            got = out.to_numpy(n)
            assert T.canon(got).tobytes() == T.canon(want).tobytes(), \
                (c.sql, n)
            out.free()
            free(dev)
        m.free()


# ---- aggregates ------------------------------------------------------------

AGG_SCHEMA = {"g": T.U8, "h": T.U8, "a": T.I32, "k": T.I64, "x": T.F64,
              "y": T.F64}
PERIOD = 1021
_c, _l = T.C, T.L
AGG_PRED = ("and", T.cmp(_c("x"), ">", _l(-30)), T.cmp(_c("k"), "<>", _l(5)))
# (function, AST): inputs are small integers and multiples of 1/8, so
# every partial sum of these is exact in any order -> bit-exact; SUM(y)
# alone has rounding and is held to rtol 1e-9 against math.fsum
AGGS = [("sum", ("*", _c("x"), _c("a"))),
        ("min", ("-", _c("k"), _c("a"))),
        ("max", _c("x")),
        ("count", None),
        ("sum", ("/", _c("a"), _l(2))),
        ("sum", ("+", ("*", _c("a"), _l(100000)), _c("k"))),
        ("max", ("+", _c("a"), _c("g"))),
        ("sum", _c("y"))]
INEXACT = {7}


def agg_sql(fn, ast):
    return "count(*)" if fn == "count" else "%s(%s)" % (fn, T.sql_of(ast))


@pytest.fixture(scope="module")
def agg_ref():
    """Base rows (one period) with the predicate and every aggregate
    input evaluated by the table's reference evaluator."""
    rng = np.random.default_rng(23)
    p = PERIOD
    base = {"g": rng.choice(np.array([0, 1, 2, 4, 255], dtype=np.uint8), p,
                            p=[0.3, 0.3, 0.3, 0.05, 0.05]),
            "h": rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), p,
                            p=[0.45, 0.45, 0.05, 0.05]),
            "a": rng.integers(-40, 41, p).astype(np.int32),
            "k": rng.integers(-9, 10, p).astype(np.int64),
            "x": rng.integers(-320, 321, p) / 8.0,
            "y": np.round(rng.uniform(1, 2, p), 3)}
    rows = T.rows_of(base)
    keep = np.array([T.evb(AGG_PRED, r) for r in rows])
    vals = [np.ones(p) if ast is None else
            np.array([float(T.ev(ast, r)) for r in rows]) for _, ast in AGGS]
    return base, keep, vals


def agg_expected(base, keep, vals, idx, gid, ngroups, aggs):
    """idx: base-row index of every input row; gid: base row -> group id
    or -1. -> (ngroups, naggs) via math.fsum / min / max."""
    out = np.zeros((ngroups, len(aggs)))
    sel_gid = np.where(keep, gid, -1)[idx]
    for g in range(ngroups):
        rows = idx[sel_gid == g]
        for j, a in enumerate(aggs):
            v = vals[a][rows]
            fn = AGGS[a][0]
            if fn in ("sum", "count"):
                out[g, j] = math.fsum(v.tolist())
            elif fn == "min":
                out[g, j] = v.min() if len(v) else np.inf
            else:
                out[g, j] = v.max() if len(v) else -np.inf
    return out


def check_agg(got, want, aggs, what):
    for j, a in enumerate(aggs):
        if a in INEXACT:
            np.testing.assert_allclose(got[:, j], want[:, j], rtol=1e-9,
                                       err_msg=str((what, AGGS[a])))
        else:
            assert got[:, j].tobytes() == want[:, j].tobytes(), \
                (what, AGGS[a], got[:, j], want[:, j])


def test_aggregate_shapes(gpu, agg_ref):
    """u8 + i32 + i64 + f64 inputs, SUM / MIN / MAX / COUNT side by side,
    one key (20 accumulators) and two keys (4 * 2 * 8 = 64, the limit),
    at the pair-path / odd-tail sizes. Group 3 of key g is never reached
    and keeps its identities. Rows with g = 4 (its cardinality), g = 255,
    h = 2 or h = 255 reach no group."""
    from quokka_amd import jit
    base, keep, vals = agg_ref
    one = [0, 1, 2, 3, 7]
    two = list(range(8))
    pred = T.sql_of(AGG_PRED)
    agg1 = jit.JitAggregate(AGG_SCHEMA, [("g", 4)],
                            [agg_sql(*AGGS[a]) for a in one], predicate=pred)
    agg2 = jit.JitAggregate(AGG_SCHEMA, [("g", 4), ("h", 2)],
                            [agg_sql(*AGGS[a]) for a in two], predicate=pred)
    assert agg2.ngroups * agg2.naggs == 64
    g, h = base["g"].astype(int), base["h"].astype(int)
    gid1 = np.where(g < 4, g, -1)
    gid2 = np.where((g < 4) & (h < 2), g * 2 + h, -1)
    assert (gid2 == -1).sum() > 50 and ((g == 4) & (h < 2)).any()
    nmax = max(AGG_SHAPES)
    idx_all = np.arange(nmax) % PERIOD
    dev = upload({c: v[idx_all] for c, v in base.items()})
    for n in AGG_SHAPES:
        idx = idx_all[:n]
        view = {c: d.view(0, n) for c, d in dev.items()}
        for agg, gid, aggs in ((agg1, gid1, one), (agg2, gid2, two)):
            acc = agg.make_acc()
            agg.run(view, acc)
            got = agg.read(acc)
            want = agg_expected(base, keep, vals, idx, gid, agg.ngroups, aggs)
            check_agg(got, want, aggs, (n, agg.ngroups))
            if agg is agg1:             # the group no row reaches
                assert got[3].tolist() == [0.0, np.inf, -np.inf, 0.0, 0.0]
            acc.free()
    # two run() calls accumulate into one acc (even split: the pair loads
    # of the second half stay aligned)
    n = 524288 + 1
    half = 262144 + 2
    acc = agg2.make_acc()
    agg2.run({c: d.view(0, half) for c, d in dev.items()}, acc)
    agg2.run({c: d.view(half, n - half) for c, d in dev.items()}, acc)
    want = agg_expected(base, keep, vals, idx_all[:n], gid2, 8, two)
    check_agg(agg2.read(acc), want, two, "two runs")
    acc.free()
    free(dev)
    agg1.free()
    agg2.free()


def test_aggregate_rejecting_predicate_and_contraction(gpu):
    from quokka_amd import jit
    # a predicate no row passes leaves every identity in place
    schema = {"g": T.U8, "x": T.F64}
    agg = jit.JitAggregate(schema, [("g", 2)],
                           ["sum(x)", "min(x)", "max(x)", "count(*)"],
                           predicate="x > 1000")
    for n in (1, 2, 513):
        dev = upload({"g": (np.arange(n) % 2).astype(np.uint8),
                      "x": np.arange(n, dtype=np.float64)})
        acc = agg.make_acc()
        agg.run(dev, acc)
        assert agg.read(acc).tolist() == [[0.0, np.inf, -np.inf, 0.0]] * 2
        acc.free()
        free(dev)
    agg.free()
    # SUM(b * c + d): unfused, every contraction triple contributes
    # exactly 0 and the rest are small dyadic terms, so the sum is exact
    # in any order; a fused multiply-add leaves 2**-60-sized errors in it
    schema = {"b": T.F64, "c": T.F64, "d": T.F64}
    agg = jit.JitAggregate(schema, [], ["sum(b * c + d)", "count(*)"])
    for n in (3, 513, 524288 + 1):
        cols = T.contraction_sum_data(n)
        terms = [b * c + d for b, c, d in zip(cols["b"].tolist(),
                                              cols["c"].tolist(),
                                              cols["d"].tolist())]
        want = math.fsum(terms)
        assert want == sum(terms)                   # exact in this order too
        dev = upload(cols)
        acc = agg.make_acc()
        agg.run(dev, acc)
        got = agg.read(acc)
        assert got[0, 1] == n
        assert got[0, 0].tobytes() == np.float64(want).tobytes(), \
            (n, got[0, 0], want)
        acc.free()
        free(dev)
    agg.free()


# ---- BETWEEN with nullable bounds -------------------------------------------

@pytest.mark.parametrize("n", [257, 513])
def test_nullable_between_bounds(gpu, n):
    """Against the pyarrow Kleene result; the bitmap's last word is
    partial at both sizes."""
    pytest.importorskip("pyarrow")
    from quokka_amd import jit, ops
    from quokka_amd.shim import DevColumn
    cases = T.nullable_cases(n)
    c0 = cases[0]
    dev = {}
    for name, v in c0.cols.items():
        if name in c0.valid:
            dev[name] = ops.NullableColumn.from_numpy(v, c0.valid[name])
        else:
            dev[name] = DevColumn.from_numpy(v)
    for c in cases:
        f = jit.JitFilter(c.sql, c.schema, nullable=c.nullable)
        idx, k = f.run(dev)
        want = np.nonzero(c.expected)[0]
        assert k == len(want), (c.sql, f.expr)
        assert np.array_equal(idx.to_numpy(k), want), (c.sql, f.expr)
        idx.free()
        f.free()
    free(dev)
