"""CPU tier of the JIT semantics table (tests/_jit_cases.py): every
case's SQL is translated, the emitted C is compiled and run as C on the
host (tests/_c_expr_host.py, one compiler invocation per test function)
and compared with the table's expected result, which comes from the
case's AST alone. Row sets are compared exactly, arithmetic outputs bit
for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jit_cases as T  # noqa: E402
from _c_expr_host import CExprLib  # noqa: E402
from quokka_amd import jit  # noqa: E402


def _translate(case):
    tr = jit.Translator(case.schema, nullable=case.nullable)
    if case.kind == "map":
        expr, _ = jit.translate_arith(case.sql, case.schema, tr)
    else:
        expr = tr.translate(case.sql)
    return expr, tr


def _run_family(cases, tmp_path):
    """Translate all, compile once, compare each; report every miss."""
    built = []
    for c in cases:
        expr, tr = _translate(c)
        assert tr.cols, c                   # a constant needs no kernel
        built.append((expr, [tr.dtype_of(n) for n in tr.cols],
                      "pred" if c.kind == "filter" else "arith", tr))
    lib = CExprLib([b[:3] for b in built], tmp_path)
    bad = []
    for i, (c, (expr, _, _, tr)) in enumerate(zip(cases, built)):
        env = dict(c.cols)
        for flag, col in tr.valid_terms:
            env[flag] = c.valid[col].astype(np.uint8)
        got = lib.run(i, [env[n] for n in tr.cols])
        if c.kind == "filter":
            ok = np.array_equal(np.nonzero(got)[0],
                                np.nonzero(c.expected)[0])
        else:
            ok = T.canon(got).tobytes() == T.canon(c.expected).tobytes()
        if not ok:
            bad.append("%s: %s -> %s\n  got  %s\n  want %s" % (
                c.name, c.sql, expr, got[:16], c.expected[:16]))
    assert not bad, "%d of %d cases differ:\n%s" % (
        len(bad), len(cases), "\n".join(bad[:12]))


def test_division_is_true_division(tmp_path):
    cases = T.division_cases()
    # the table itself: a = 7 keeps the row under a / 2 > 3
    c0 = cases[0]
    assert c0.sql == "(a / 2) > 3" and c0.cols["a"][0] == 7
    assert c0.expected[0]
    _run_family(cases, tmp_path)


def test_integer_arithmetic_is_64_bit(tmp_path):
    cases = T.width_cases()
    by = {c.name: c for c in cases}
    assert by["width/map_mul"].expected[0] == 214748364700000.0
    assert by["width/map_u8_sub"].expected[0] == -200.0
    _run_family(cases, tmp_path)


def test_literal_edges(tmp_path):
    cases = T.literal_edge_cases()
    by = {c.sql: c for c in cases}
    # k = [MIN, -1, 0, 1, MAX, MIN+1, MAX-1]
    assert not by["k > 9223372036854775808"].expected.any()
    assert by["k > -9223372036854775808"].expected.tolist() == \
        [False, True, True, True, True, True, True]
    assert by["k >= -9223372036854775809"].expected.all()
    assert len(cases) >= 4 * 6 + 10
    _run_family(cases, tmp_path)


def test_literal_edges_never_emit_an_unsigned_constant():
    for c in T.literal_edge_cases():
        expr, _ = _translate(c)
        assert "9223372036854775808" not in expr, (c.sql, expr)
        assert "9223372036854775809" not in expr, (c.sql, expr)


def test_precedence_and_parsing(tmp_path):
    _run_family(T.precedence_cases(), tmp_path)


def test_contraction_free_on_host(tmp_path):
    """The host build uses -ffp-contract=off like the kernels: the C text
    itself must not hide a fused form (e.g. through fma())."""
    _run_family(T.contraction_cases(), tmp_path)


def test_nan_and_infinities_follow_ieee(tmp_path):
    cases = T.nan_cases()
    b = cases[0].cols["b"]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(cases[0].expected, b > 0)        # numpy agrees
        assert np.array_equal(cases[1].expected, ~(b > 0))
        assert np.array_equal(cases[3].expected, b != b)
    _run_family(cases, tmp_path)


def test_generated_arithmetic_batch(tmp_path):
    cases = T.generated_cases()
    assert sum(c.kind == "filter" for c in cases) >= 150
    assert sum(c.kind == "map" for c in cases) >= 50
    _run_family(cases, tmp_path)


@pytest.mark.parametrize("sql,schema", T.reject_cases(),
                         ids=[r[0] for r in T.reject_cases()])
def test_rejects_raise_value_error(sql, schema):
    with pytest.raises(ValueError):
        jit.translate(sql, schema)
    with pytest.raises(ValueError):
        jit.translate(sql, schema, nullable=("a", "b"))


def test_nullable_between_bounds(tmp_path):
    pytest.importorskip("pyarrow")
    cases = T.nullable_cases(257) + T.nullable_cases(64)
    c0 = cases[0]
    assert c0.sql == "not (b between lo and 5)"
    # lo NULL and b > 5: BETWEEN is FALSE, its negation keeps the row
    hit = ~c0.valid["lo"] & c0.valid["b"] & (c0.cols["b"] > 5)
    assert hit.any() and c0.expected[hit].all()
    _run_family(cases, tmp_path)


def test_no_text_change_without_integer_arithmetic():
    """Predicates with no integer arithmetic, no nullable BETWEEN bound
    and no out-of-range literal translate to the text they always had."""
    schema = {"l_shipdate": np.dtype(np.int32),
              "l_discount": np.dtype(np.float64),
              "l_quantity": np.dtype(np.float64),
              "l_extendedprice": np.dtype(np.float64),
              "l_tax": np.dtype(np.float64), "k": np.dtype(np.int64)}
    q6 = ("l_shipdate >= date '1994-01-01' and l_shipdate < "
          "date '1994-01-01' + interval '1' year and l_discount "
          "between 0.06 - 0.01 and 0.06 + 0.01 and l_quantity < 24")
    assert jit.translate(q6, schema)[0] == (
        "((((v0) >= (8766)) && ((v0) < (9131))) && ((((v1) >= "
        "(0.049999999999999996)) && ((v1) <= (0.06999999999999999))))) "
        "&& ((v2) < (24))")
    assert jit.translate_arith(
        "l_extendedprice * (1 - l_discount) * (1 + l_tax) / l_quantity",
        schema)[0] == ("(((v0) * (((1) - (v1)))) * (((1) + (v2)))) / (v3)")
    assert jit.translate("k + 1 > k * 2 - (3)", schema)[0] == \
        "((v0) + (1)) > (((v0) * (2)) - ((3)))"
    assert jit.Translator(schema, nullable=("k",)).translate(
        "not (k between 1 and 5)") == \
        "((((v1) != 0)) && !((((v0) >= (1)) && ((v0) <= (5)))))"


def test_group_id_rejects_out_of_range_keys(tmp_path):
    """Two keys: the generated group id is -1 when either key is outside
    [0, cardinality); the id text is run as C."""
    schema = {"g": np.dtype(np.uint8), "h": np.dtype(np.int32),
              "x": np.dtype(np.float64)}
    # hiprtc is a pure compiler: building needs no GPU
    agg = jit.JitAggregate(schema, [("g", 3), ("h", 2)], ["sum(x)"])
    cols, gexpr = agg.cols, agg.group_expr
    agg.free()
    g = np.array([0, 1, 2, 3, 255, 2, 0, 1], dtype=np.uint8)
    h = np.array([0, 1, 1, 0, 1, 2, -1, 255], dtype=np.int32)
    want = np.array([0, 3, 5, -1, -1, -1, -1, -1], dtype=np.float64)
    lib = CExprLib([(gexpr,
                     [schema[c] for c in cols if c in ("g", "h")], "arith")],
                   tmp_path)
    assert cols[:2] == ["g", "h"]
    got = lib.run(0, [g, h])
    assert got.tolist() == want.tolist(), gexpr
