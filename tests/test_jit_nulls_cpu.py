"""CPU tests of SQL three-valued logic in the predicate translator and of
the host half of stage_columns' mask mode.

Random predicates with IS [NOT] NULL leaves over two nullable and two
non-null columns are translated with `nullable=`, the emitted C
expression is evaluated through numpy (validity flags as u8 inputs, null
slots holding 0 as on the device) and compared with a direct Kleene
evaluation that carries an explicit unknown state. WHERE keeps the rows
that are TRUE."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from quokka_amd import jit

SCHEMA = {
    "a": np.dtype(np.int32),        # nullable
    "b": np.dtype(np.float64),      # nullable
    "c": np.dtype(np.float64),
    "k": np.dtype(np.int64),
}
NULLABLE = ("a", "b")

_num = st.one_of(
    st.integers(min_value=-20, max_value=20),
    st.floats(min_value=-20, max_value=20, allow_nan=False,
              allow_infinity=False).map(lambda x: round(x, 1)),
)
_col = st.sampled_from(list(SCHEMA))
_cmp = st.sampled_from(["<", "<=", ">", ">=", "=", "<>"])


@st.composite
def leaf(draw, with_is=True):
    col = draw(_col)
    kind = draw(st.integers(0, 5 if with_is else 4))
    if kind == 0:
        return ("cmp", col, draw(_cmp), draw(_num))
    if kind == 1:
        lo, hi = sorted([draw(_num), draw(_num)])
        return ("between", col, lo, hi)
    if kind == 2:
        return ("in", col, draw(st.lists(_num, min_size=1, max_size=4)))
    if kind == 3:
        return ("notin", col, draw(st.lists(_num, min_size=1, max_size=4)))
    if kind == 4:
        if draw(st.booleans()):
            # BETWEEN whose low bound, high bound or both are columns
            # (nullable ones included): the Kleene AND of two comparisons
            lo = draw(st.one_of(_num, _col))
            hi = draw(_col if not isinstance(lo, str)
                      else st.one_of(_num, _col))
            return ("between2", col, lo, hi)
        return ("cmp2", col, draw(_cmp), draw(_col))
    return ("isnull" if draw(st.booleans()) else "notnull", col)


@st.composite
def predicate(draw, depth=0, with_is=True):
    if depth >= 3 or draw(st.integers(0, 2)) == 0:
        return draw(leaf(with_is=with_is))
    kind = draw(st.sampled_from(["and", "or", "not"]))
    if kind == "not":
        return ("not", draw(predicate(depth=depth + 1, with_is=with_is)))
    return (kind, draw(predicate(depth=depth + 1, with_is=with_is)),
            draw(predicate(depth=depth + 1, with_is=with_is)))


def to_sql(p):
    k = p[0]
    if k == "cmp":
        return "%s %s %r" % (p[1], p[2], p[3])
    if k == "cmp2":
        return "%s %s %s" % (p[1], p[2], p[3])
    if k == "between":
        return "%s between %r and %r" % (p[1], p[2], p[3])
    if k == "between2":
        return "%s between %s and %s" % (
            p[1], *[b if isinstance(b, str) else repr(b) for b in p[2:]])
    if k in ("in", "notin"):
        return "%s %sin (%s)" % (p[1], "not " if k == "notin" else "",
                                 ", ".join(repr(e) for e in p[2]))
    if k == "isnull":
        return "%s is null" % p[1]
    if k == "notnull":
        return "%s IS NOT NULL" % p[1]
    if k == "not":
        return "not (%s)" % to_sql(p[1])
    return "(%s) %s (%s)" % (to_sql(p[1]), k, to_sql(p[2]))


# Kleene evaluation: a pair of bool arrays (true, false); a row where
# neither holds is UNKNOWN
def kleene(p, vals, valid):
    k = p[0]
    n = len(vals["a"])
    known = np.ones(n, dtype=bool)
    if k in ("isnull", "notnull"):
        isn = ~valid[p[1]]
        return (isn, ~isn) if k == "isnull" else (~isn, isn)
    if k == "between2":
        return kleene(("and", ("cmp2" if isinstance(p[2], str) else "cmp",
                               p[1], ">=", p[2]),
                       ("cmp2" if isinstance(p[3], str) else "cmp",
                        p[1], "<=", p[3])), vals, valid)
    if k in ("cmp", "cmp2", "between", "in", "notin"):
        v = vals[p[1]]
        known = valid[p[1]].copy()
        if k == "cmp" or k == "cmp2":
            rhs = p[3]
            if k == "cmp2":
                known &= valid[p[3]]
                rhs = vals[p[3]]
            r = {"<": v < rhs, "<=": v <= rhs, ">": v > rhs,
                 ">=": v >= rhs, "=": v == rhs, "<>": v != rhs}[p[2]]
        elif k == "between":
            r = (v >= p[2]) & (v <= p[3])
        else:
            r = np.zeros(n, dtype=bool)
            for e in p[2]:
                r |= v == e
            if k == "notin":
                r = ~r
        return known & r, known & ~r
    if k == "not":
        t, f = kleene(p[1], vals, valid)
        return f, t
    (ta, fa), (tb, fb) = kleene(p[1], vals, valid), kleene(p[2], vals, valid)
    if k == "and":
        return ta & tb, fa | fb
    return ta | tb, fa & fb


def c_eval(expr, order, env_cols, n):
    env = {"v%d" % i: env_cols[name] for i, name in enumerate(order)}
    # C's ! is logical (the translator folds IS NULL on a non-null column
    # to the int constants (0) / (1)), so it maps to logical_not, not ~
    py = expr.replace("&&", "&").replace("||", "|").replace("!(", "_not(")
    env["_not"] = np.logical_not
    return np.broadcast_to(eval(py, {"np": np}, env) != 0, (n,))


def make_data(seed, n=400):
    rng = np.random.default_rng(seed)
    vals = {
        "a": rng.integers(-25, 25, n).astype(np.int32),
        "b": np.round(rng.uniform(-25, 25, n), 1),
        "c": np.round(rng.uniform(-25, 25, n), 1),
        "k": rng.integers(-25, 25, n).astype(np.int64),
    }
    valid = {c: np.ones(n, dtype=bool) for c in vals}
    for c in NULLABLE:
        valid[c] = rng.random(n) > 0.4
        vals[c] = np.where(valid[c], vals[c], 0).astype(vals[c].dtype)
    return vals, valid


@settings(max_examples=300, deadline=None)
@given(predicate())
def test_three_valued_translate_matches_kleene(p):
    sql = to_sql(p)
    tr = jit.Translator(SCHEMA, nullable=NULLABLE)
    expr = tr.translate(sql)
    vals, valid = make_data(abs(hash(sql)) % (2 ** 32))
    env = dict(vals)
    for flag, col in tr.valid_terms:
        assert flag == "__valid_" + col and col in NULLABLE
        assert tr.dtype_of(flag) == np.dtype(np.uint8)
        env[flag] = valid[col].astype(np.uint8)
    got = c_eval(expr, tr.cols, env, len(vals["a"]))
    want, _ = kleene(p, vals, valid)
    assert np.array_equal(got, want), (sql, expr)


@settings(max_examples=200, deadline=None)
@given(predicate(with_is=False))
def test_empty_nullable_emits_the_two_valued_string(p):
    """nullable=() is the existing path: same string, same columns, no
    validity inputs."""
    sql = to_sql(p)
    want_expr, want_cols = jit.translate(sql, SCHEMA)
    tr = jit.Translator(SCHEMA, None, nullable=())
    assert tr.translate(sql) == want_expr
    assert tr.cols == want_cols and tr.valid_terms == []
    expr, cols = jit.translate(sql, SCHEMA, nullable=())
    assert (expr, cols) == (want_expr, want_cols)


def test_or_with_null_side_is_true():
    """The case a plain AND of all validities gets wrong: a > 5 OR b < 3
    with a NULL and b = 1 is TRUE."""
    tr = jit.Translator(SCHEMA, nullable=NULLABLE)
    expr = tr.translate("a > 5 OR b < 3")
    env = {"a": np.array([0, 9, 0], dtype=np.int32),
           "b": np.array([1.0, 0.0, 7.0]),
           "__valid_a": np.array([0, 1, 0], dtype=np.uint8),
           "__valid_b": np.array([1, 0, 1], dtype=np.uint8)}
    got = c_eval(expr, tr.cols, env, 3)
    assert got.tolist() == [True, True, False]
    # NOT of an unknown stays unknown, so the row is dropped
    tr = jit.Translator(SCHEMA, nullable=NULLABLE)
    expr = tr.translate("NOT (a > 5)")
    got = c_eval(expr, tr.cols, env, 3)
    assert got.tolist() == [False, False, False]


def test_nullable_validation():
    with pytest.raises(ValueError, match="unknown nullable"):
        jit.Translator(SCHEMA, nullable=("zz",))
    schema = dict(SCHEMA, s=jit.RAW_STRING)
    with pytest.raises(ValueError, match="null strings"):
        jit.Translator(schema, nullable=("s",)).translate("s LIKE 'x%'")
    # a non-null raw string beside a nullable number still works
    tr = jit.Translator(schema, nullable=("a",))
    tr.translate("s LIKE 'x%' AND a IS NOT NULL")
    assert [t[1] for t in tr.str_terms] == ["s"]
    assert [t[1] for t in tr.valid_terms] == ["a"]


def test_is_null_without_nullable_columns_folds():
    assert jit.translate("a IS NULL", SCHEMA)[0] == "(0)"
    assert jit.translate("a IS NOT NULL", SCHEMA)[0] == "(1)"


# ---- staging mask mode, host half ---------------------------------------

pa = pytest.importorskip("pyarrow")


@pytest.mark.parametrize("offset", [0, 1, 3, 8, 13])
@pytest.mark.parametrize("typ", ["int64", "float64", "int32", "date32"])
def test_split_nulls_offsets(offset, typ):
    from quokka_amd import staging
    from quokka_amd.ops import pack_valid, valid_nbytes
    rng = np.random.default_rng(offset)
    n = 201
    mask = rng.random(n) > 0.3
    raw = rng.integers(1, 1 << 40 if typ == "int64" else 30000, n)
    arr = pa.array(raw, mask=~mask, type=pa.int64())
    if typ != "int64":
        arr = arr.cast({"float64": pa.float64(), "int32": pa.int32(),
                        "date32": pa.int32()}[typ])
        if typ == "date32":
            arr = arr.cast(pa.date32())
    sl = arr.slice(offset)
    assert sl.offset == offset
    filled, m = staging.split_nulls(sl)
    assert filled.null_count == 0
    assert np.array_equal(m, mask[offset:])
    vals = staging.column_to_numpy(filled)
    want_dt = {"int64": np.int64, "float64": np.float64, "int32": np.int32,
               "date32": np.int32}[typ]
    assert vals.dtype == want_dt          # an int column stays an int
    want = np.where(mask, raw, 0)[offset:].astype(want_dt)
    assert np.array_equal(vals, want)
    bits = pack_valid(m)
    assert len(bits) == valid_nbytes(len(m)) and len(bits) % 8 == 0
    assert np.array_equal(
        np.unpackbits(bits, bitorder="little")[:len(m)].astype(bool), m)
    assert not np.unpackbits(bits, bitorder="little")[len(m):].any()
