"""Shared case table for the expression JIT: SQL text, schema, column
data and the expected result, used by the CPU tier (translated C run as
C on the host) and the GPU tier (the hiprtc kernels).

The expected result of every case comes from the case's own AST through
an evaluator in this file, never from the translator or a kernel:

* non-null cases: `ev` / `evb`, row by row in Python. Integers stay
  exact Python ints. `/` converts both sides to f64 and divides in IEEE
  (x / 0 is +-inf or NaN). Once a float is involved every operation is
  one IEEE double operation in the written order: Python floats never
  fuse. An int compared with a float is converted to f64 first. Wherever
  arithmetic produces an int or an int meets a float its magnitude must
  stay below 2**53 (`Unsafe` otherwise), so this reference, C and any SQL
  engine agree.
* nullable cases: pyarrow.compute over the same AST (and_kleene,
  or_kleene, invert, is_null); WHERE keeps the rows that are TRUE.

AST: ("col", name) ("lit", v) ("date", y, m, d, [(sign, n, unit)..])
("neg", x) (op, x, y) for op in + - * /; booleans ("cmp", op, x, y)
("between", x, lo, hi) ("in", x, [v..]) ("notin", x, [v..])
("isnull", x) ("notnull", x) ("not", p) ("and", p, q) ("or", p, q)."""
import datetime
import math
import random
from fractions import Fraction

import numpy as np

I32, F64, U8, I64 = (np.dtype(np.int32), np.dtype(np.float64),
                     np.dtype(np.uint8), np.dtype(np.int64))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
LIMIT = 1 << 53
CMP_OPS = ["<", "<=", ">", ">=", "=", "<>"]


class Unsafe(Exception):
    """An integer left the range in which all evaluators agree."""


class Case:
    def __init__(self, name, family, sql, schema, cols, kind, expected,
                 ast=None, gpu=False, nullable=(), valid=None):
        self.name, self.family, self.sql = name, family, sql
        self.schema, self.cols, self.kind = schema, cols, kind
        self.expected, self.ast, self.gpu = expected, ast, gpu
        self.nullable, self.valid = tuple(nullable), valid

    def __repr__(self):
        return "Case(%s: %s)" % (self.name, self.sql)


# ---- SQL text ------------------------------------------------------------

def _lit_sql(v):
    s = repr(v)
    assert "e" not in s and "n" not in s, s     # no exponent / inf / nan
    return s


def sql_of(x):
    k = x[0]
    if k == "col":
        return x[1]
    if k == "lit":
        return _lit_sql(x[1])
    if k == "date":
        s = "date '%04d-%02d-%02d'" % x[1:4]
        for sign, n, unit in x[4]:
            s += " %s interval '%d' %s" % (sign, n, unit)
        return s
    if k == "neg":
        return "(-%s)" % sql_of(x[1])
    if k in "+-*/":
        return "(%s %s %s)" % (sql_of(x[1]), k, sql_of(x[2]))
    if k == "cmp":
        return "%s %s %s" % (sql_of(x[2]), x[1], sql_of(x[3]))
    if k == "between":
        return "%s between %s and %s" % tuple(sql_of(y) for y in x[1:])
    if k in ("in", "notin"):
        return "%s %sin (%s)" % (sql_of(x[1]), "not " if k == "notin" else "",
                                 ", ".join(_lit_sql(v) for v in x[2]))
    if k == "isnull":
        return "%s is null" % sql_of(x[1])
    if k == "notnull":
        return "%s is not null" % sql_of(x[1])
    if k == "not":
        return "not (%s)" % sql_of(x[1])
    assert k in ("and", "or"), k
    return "(%s) %s (%s)" % (sql_of(x[1]), k, sql_of(x[2]))


# ---- reference evaluator, non-null ---------------------------------------

def _int_result(v):
    if abs(v) >= LIMIT:
        raise Unsafe(v)
    return v


def _f(v):
    if isinstance(v, int):
        if abs(v) > LIMIT:
            raise Unsafe(v)
        return float(v)
    return v


def _div(x, y):
    if y == 0.0:
        if x == 0.0 or x != x:
            return math.nan
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def _date_days(y, m, d, chain):
    cur = datetime.date(y, m, d)
    for sign, n, unit in chain:
        n = n if sign == "+" else -n
        if unit == "day":
            cur += datetime.timedelta(days=n)
            continue
        mo = cur.month - 1 + (n if unit == "month" else 12 * n)
        yy, mm = cur.year + mo // 12, mo % 12 + 1
        last = ((datetime.date(yy + mm // 12, mm % 12 + 1, 1)
                 - datetime.timedelta(days=1)).day)
        cur = datetime.date(yy, mm, min(cur.day, last))
    return (cur - datetime.date(1970, 1, 1)).days


def ev(x, row):
    """Arithmetic AST -> exact Python int or IEEE float."""
    k = x[0]
    if k == "col":
        return row[x[1]]
    if k == "lit":
        return x[1]
    if k == "date":
        return _date_days(x[1], x[2], x[3], x[4])
    if k == "neg":
        v = ev(x[1], row)
        return _int_result(-v) if isinstance(v, int) else -v
    l, r = ev(x[1], row), ev(x[2], row)
    if k == "/":
        if r == 0 and not _has_col(x):
            raise Unsafe("a literal x / 0 is rejected, not evaluated")
        return _div(_f(l), _f(r))
    if isinstance(l, int) and isinstance(r, int):
        return _int_result(l + r if k == "+" else l - r if k == "-"
                           else l * r)
    l, r = _f(l), _f(r)
    return l + r if k == "+" else l - r if k == "-" else l * r


def _cmp(op, l, r):
    if not (isinstance(l, int) and isinstance(r, int)):
        l, r = _f(l), _f(r)
    return {"<": l < r, "<=": l <= r, ">": l > r, ">=": l >= r,
            "=": l == r, "<>": l != r}[op]


def evb(p, row):
    """Boolean AST -> bool (no NULLs)."""
    k = p[0]
    if k == "cmp":
        return _cmp(p[1], ev(p[2], row), ev(p[3], row))
    if k == "between":
        v = ev(p[1], row)
        return _cmp(">=", v, ev(p[2], row)) and _cmp("<=", v, ev(p[3], row))
    if k in ("in", "notin"):
        v = ev(p[1], row)
        hit = any(_cmp("=", v, e) for e in p[2])
        return hit != (k == "notin")
    if k == "not":
        return not evb(p[1], row)
    if k == "and":
        a, b = evb(p[1], row), evb(p[2], row)
        return a and b
    assert k == "or", k
    a, b = evb(p[1], row), evb(p[2], row)
    return a or b


def rows_of(cols):
    names = list(cols)
    lists = [cols[c].tolist() for c in names]      # Python ints / floats
    return [dict(zip(names, vals)) for vals in zip(*lists)]


def expect_filter(ast, cols):
    return np.array([evb(ast, r) for r in rows_of(cols)], dtype=bool)


def expect_map(ast, cols):
    return np.array([float(_f(ev(ast, r))) for r in rows_of(cols)],
                    dtype=np.float64)


def canon(a):
    """f64 array with every NaN replaced by one NaN: IEEE leaves the sign
    and payload of an invalid operation's NaN to the implementation, so a
    bit-for-bit comparison is made after this."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


# ---- reference evaluator, nullable (pyarrow Kleene) -----------------------

def pa_expected(p, cols, valid):
    import pyarrow as pa
    import pyarrow.compute as pc
    arrays = {c: pa.array(v, mask=None if c not in valid else ~valid[c])
              for c, v in cols.items()}

    def operand(x):
        if x[0] == "col":
            return arrays[x[1]]
        assert x[0] == "lit", x
        return pa.scalar(x[1])

    cmp_fn = {"<": pc.less, "<=": pc.less_equal, ">": pc.greater,
              ">=": pc.greater_equal, "=": pc.equal, "<>": pc.not_equal}

    def go(q):
        k = q[0]
        if k == "cmp":
            return cmp_fn[q[1]](operand(q[2]), operand(q[3]))
        if k == "between":
            v = operand(q[1])
            return pc.and_kleene(pc.greater_equal(v, operand(q[2])),
                                 pc.less_equal(v, operand(q[3])))
        if k in ("in", "notin"):
            v, acc = operand(q[1]), None
            for e in q[2]:
                t = pc.equal(v, pa.scalar(e))
                acc = t if acc is None else pc.or_kleene(acc, t)
            return pc.invert(acc) if k == "notin" else acc
        if k == "isnull":
            return pc.is_null(operand(q[1]))
        if k == "notnull":
            return pc.is_valid(operand(q[1]))
        if k == "not":
            return pc.invert(go(q[1]))
        fn = pc.and_kleene if k == "and" else pc.or_kleene
        return fn(go(q[1]), go(q[2]))

    res = pc.fill_null(go(p), False)
    return np.asarray(res.to_numpy(zero_copy_only=False), dtype=bool)


# ---- helpers to write ASTs ------------------------------------------------

def C(n):
    return ("col", n)


def L(v):
    return ("lit", v)


def cmp(l, op, r):
    return ("cmp", op, l, r)


def _case(name, family, ast, schema, cols, kind, gpu=False, sql=None):
    used = {c: cols[c] for c in cols}
    exp = (expect_filter if kind == "filter" else expect_map)(ast, used)
    return Case(name, family, sql or sql_of(ast), schema, used, kind, exp,
                ast=ast, gpu=gpu)


# ---- family: integer division ---------------------------------------------

def _div_data():
    a = [7, -7, 1, -1, 0, 3, 8, -8, I32_MAX, I32_MIN, 9, -9, 5, 6, 100, -3]
    e = [2, 2, 3, -3, 0, 0, 3, 3, 2, 2, -2, 4, 0, 4, 7, 2]
    k = [7, -7, (1 << 40) + 1, -(1 << 40) - 1, 0, 5, -5, 9, 11, -11, 1, -1,
         0, 13, 1000001, -15]
    u = [0, 1, 7, 255, 200, 3, 5, 9, 11, 13, 15, 17, 2, 4, 6, 8]
    return ({"a": I32, "e": I32, "k": I64, "u": U8},
            {"a": np.array(a, dtype=I32), "e": np.array(e, dtype=I32),
             "k": np.array(k, dtype=I64), "u": np.array(u, dtype=U8)})


def division_cases():
    schema, cols = _div_data()
    a, e, k, u = C("a"), C("e"), C("k"), C("u")
    filt = [
        ("i32_lit_gt", cmp(("/", a, L(2)), ">", L(3)), True),
        ("i32_lit_eq_half", cmp(("/", a, L(2)), "=", L(3.5)), True),
        ("i32_lit_neg", cmp(("/", ("neg", a), L(2)), "<=", L(-3.5)), False),
        ("i32_lit_roundtrip", cmp(("*", ("/", a, L(2)), L(2)), "=", a),
         False),
        ("i32_i32_zero_divisor", cmp(("/", a, e), ">=", L(1.5)), True),
        ("i32_i32_nan_ne", cmp(("/", a, e), "<>", ("/", a, e)), False),
        ("i64_i32", cmp(("/", k, e), "<", L(-0.5)), True),
        ("u8_lit", cmp(("/", u, L(2)), ">", L(3)), True),
        ("u8_lit_ne", cmp(("/", u, L(4)), "<>", L(1)), False),
        ("sum_then_div", cmp(("/", ("+", a, L(1)), L(2)), "<", L(4.5)),
         False),
        ("div_in_between", ("between", ("/", a, L(2)), L(0.5), L(3.5)),
         False),
        ("div_left_of_in", ("in", ("/", u, L(2)), [0.5, 3.5, 100]), False),
    ]
    maps = [("map_i32_lit", ("/", a, L(2)), True),
            ("map_i32_i32", ("/", a, e), True),
            ("map_i64_i32", ("/", k, e), False),
            ("map_u8_lit", ("/", u, L(8)), False),
            ("map_lit_i32", ("/", L(1), e), False)]
    out = [_case("div/" + n, "division", ast, schema, cols, "filter", True)
           for n, ast, _ in filt]
    out += [_case("div/" + n, "division", ast, schema, cols, "map", True)
            for n, ast, _ in maps]
    return out


# ---- family: integer width ------------------------------------------------

def width_cases():
    schema = {"a": I32, "e": I32, "u": U8}
    cols = {"a": np.array([I32_MAX, I32_MIN, 30000, -30000, 21475, 21474,
                           0, 1, -1, 2], dtype=I32),
            "e": np.array([I32_MIN, I32_MAX, 1, -1, 0, 5, I32_MAX, I32_MIN,
                           I32_MIN, 7], dtype=I32),
            "u": np.array([0, 199, 200, 201, 255, 1, 100, 250, 2, 3],
                          dtype=U8)}
    a, e, u = C("a"), C("e"), C("u")
    filt = [
        ("mul_leaves_i32", cmp(("*", a, L(100000)), ">", L(2147483647))),
        ("add_leaves_i32", cmp(("+", a, L(2147483647)), ">",
                               L(2147483647))),
        ("u8_goes_negative", cmp(("-", u, L(200)), "<", L(0))),
        ("neg_int32_min", cmp(("neg", a), ">", L(2147483647))),
        ("sub_cols", cmp(("-", a, e), ">", L(4294967294))),
        ("mul_cols_vs_i64", cmp(("*", a, L(3)), "<", ("-", e, L(10)))),
    ]
    maps = [("map_mul", ("*", a, L(100000))),
            ("map_add", ("+", a, L(2147483647))),
            ("map_u8_sub", ("-", u, L(200))),
            ("map_neg", ("neg", a)),
            ("map_sub_cols", ("-", a, e))]
    out = [_case("width/" + n, "width", ast, schema, cols, "filter", True)
           for n, ast in filt]
    out += [_case("width/" + n, "width", ast, schema, cols, "map", True)
            for n, ast in maps]
    return out


# ---- family: literal edges -------------------------------------------------

EDGE_LITS = [9223372036854775807, 9223372036854775808,
             -9223372036854775808, -9223372036854775809]


def literal_edge_cases():
    schema = {"k": I64}
    cols = {"k": np.array([I64_MIN, -1, 0, 1, I64_MAX, I64_MIN + 1,
                           I64_MAX - 1], dtype=I64)}
    k = C("k")
    out = []
    for lit in EDGE_LITS:
        for op in CMP_OPS:
            out.append(_case("edge/k %s %d" % (op, lit), "literal_edges",
                             cmp(k, op, L(lit)), schema, cols, "filter",
                             gpu=True))
    extra = [
        cmp(L(9223372036854775808), ">", k),
        cmp(L(-9223372036854775808), "<", k),
        cmp(L(-9223372036854775809), ">=", k),
        ("in", k, [9223372036854775807, 9223372036854775808]),
        ("in", k, [-9223372036854775808, -9223372036854775809]),
        ("in", k, [9223372036854775808, -9223372036854775809]),
        ("notin", k, [9223372036854775808]),
        ("notin", k, [-9223372036854775808, 0]),
        ("between", k, L(-9223372036854775809), L(9223372036854775808)),
        ("between", k, L(-9223372036854775808), L(9223372036854775807)),
        ("between", k, L(1), L(9223372036854775808)),
        ("between", k, L(-9223372036854775809), L(-1)),
        ("between", k, L(9223372036854775807), L(9223372036854775808)),
        ("between", k, L(9223372036854775808), L(9223372036854775808)),
        ("not", ("between", k, L(-9223372036854775808), L(0))),
    ]
    for ast in extra:
        out.append(_case("edge/" + sql_of(ast), "literal_edges", ast,
                         schema, cols, "filter", gpu=True))
    return out


# ---- family: precedence and parsing ---------------------------------------

def precedence_cases():
    schema = {"a": I32, "b": F64, "k": I64, "d": I32}
    rnd = random.Random(11)
    n = 96
    d0 = _date_days(1994, 1, 1, [])
    cols = {"a": np.array([rnd.randint(-4, 4) for _ in range(n)], dtype=I32),
            "b": np.array([rnd.randint(-16, 16) / 4.0 for _ in range(n)]),
            "k": np.array([rnd.randint(-6, 6) for _ in range(n)], dtype=I64),
            "d": np.array([d0 + rnd.randint(-800, 1200) for _ in range(n)],
                          dtype=I32)}
    a, b, k, d = C("a"), C("b"), C("k"), C("d")
    eq = lambda x, v: cmp(x, "=", L(v))                     # noqa: E731
    table = [
        ("NOT a = 1 AND b = 2", ("and", ("not", eq(a, 1)), eq(b, 2))),
        ("a = 1 OR a = 2 AND b < 3",
         ("or", eq(a, 1), ("and", eq(a, 2), cmp(b, "<", L(3))))),
        ("(a) BETWEEN 1 AND 2", ("between", a, L(1), L(2))),
        ("((a > 1))", cmp(a, ">", L(1))),
        ("(a + 1) * 2 > b AND (b < 2 OR a = 1)",
         ("and", cmp(("*", ("+", a, L(1)), L(2)), ">", b),
          ("or", cmp(b, "<", L(2)), eq(a, 1)))),
        ("a - -3 > 0", cmp(("-", a, L(-3)), ">", L(0))),
        ("- a < 3", cmp(("neg", a), "<", L(3))),
        ("2 - 3 - 4 < a", cmp(("-", ("-", L(2), L(3)), L(4)), "<", a)),
        ("8 / 4 / 2 < b", cmp(("/", ("/", L(8), L(4)), L(2)), "<", b)),
        ("a - (k - a) > 0", cmp(("-", a, ("-", k, a)), ">", L(0))),
        ("a + k * 2 - 1 >= b", cmp(("-", ("+", a, ("*", k, L(2))), L(1)),
                                  ">=", b)),
        ("a * 2 + 1 <> k - 1 - 1",
         cmp(("+", ("*", a, L(2)), L(1)), "<>",
             ("-", ("-", k, L(1)), L(1)))),
        ("not not a > 0 or not (b <= 1 and k <> 2)",
         ("or", ("not", ("not", cmp(a, ">", L(0)))),
          ("not", ("and", cmp(b, "<=", L(1)), cmp(k, "<>", L(2)))))),
        ("d between date '1994-01-01' and date '1994-01-01' + interval "
         "'1' year - interval '1' day",
         ("between", d, ("date", 1994, 1, 1, []),
          ("date", 1994, 1, 1, [("+", 1, "year"), ("-", 1, "day")]))),
        ("d between date '1996-02-29' - interval '1' year and date "
         "'1996-01-31' + interval '1' month + interval '3' day",
         ("between", d, ("date", 1996, 2, 29, [("-", 1, "year")]),
          ("date", 1996, 1, 31, [("+", 1, "month"), ("+", 3, "day")]))),
        ("d >= date '1995-03-31' - interval '13' month and d < date "
         "'1995-03-31' + interval '90' day",
         ("and", cmp(d, ">=", ("date", 1995, 3, 31, [("-", 13, "month")])),
          cmp(d, "<", ("date", 1995, 3, 31, [("+", 90, "day")])))),
    ]
    return [_case("prec/" + sql, "precedence", ast, schema, cols, "filter",
                  gpu=True, sql=sql) for sql, ast in table]


# ---- family: rejects -------------------------------------------------------

def reject_cases():
    schema = {"a": I32, "b": F64, "k": I64}
    return [(sql, schema) for sql in [
        "b > 1 / 0", "b > 1.5 / (2 - 2)", "b > 1e5", "a in ()", "(a > 1",
        "a > 1)", "((a > 1) and b < 2", "a >", "a + > 1", "a > 1 and",
        "or a > 1", "a = 'it''s'", "b = 'x'", "a + interval '1' day > 3",
        "zz > 1", "a > zz + 1", "a between 1", "a in (1, zz)",
        "k + 9223372036854775808 > 0",
    ]]


# ---- family: contraction ---------------------------------------------------

def contraction_data(count=256, seed=3):
    """(b, c, d) with fl(fl(b*c)+d) == 0 exactly while the exact b*c+d
    (what a fused multiply-add rounds) is > 0 for the first half of the
    rows and < 0 for the second half. Row 0 is b = c = 1 + 2**-30,
    d = -(1 + 2**-29)."""
    rnd = random.Random(seed)
    pos = [(1 + 2.0 ** -30, 1 + 2.0 ** -30, -(1 + 2.0 ** -29))]
    neg = []
    while len(pos) < count // 2 or len(neg) < count // 2:
        b = 1.0 + rnd.getrandbits(52) * 2.0 ** -52
        c = 1.0 + rnd.getrandbits(52) * 2.0 ** -52
        p = b * c
        err = Fraction(b) * Fraction(c) - Fraction(p)
        if err > 0 and len(pos) < count // 2:
            pos.append((b, c, -p))
        elif err < 0 and len(neg) < count // 2:
            neg.append((b, c, -p))
    for b, c, d in pos + neg:
        exact = Fraction(b) * Fraction(c) + Fraction(d)
        assert b * c + d == 0.0 and exact != 0
        assert float(exact) != 0.0              # the fused result
    rows = pos + neg
    return {"b": np.array([r[0] for r in rows]),
            "c": np.array([r[1] for r in rows]),
            "d": np.array([r[2] for r in rows])}, len(pos)


def contraction_cases():
    schema = {"b": F64, "c": F64, "d": F64}
    cols, npos = contraction_data()
    e = ("+", ("*", C("b"), C("c")), C("d"))
    out = [
        _case("contract/gt0", "contraction", cmp(e, ">", L(0)), schema,
              cols, "filter", True, sql="b * c + d > 0"),
        _case("contract/lt0", "contraction", cmp(e, "<", L(0)), schema,
              cols, "filter", True, sql="b * c + d < 0"),
        _case("contract/eq0", "contraction", cmp(e, "=", L(0)), schema,
              cols, "filter", True, sql="b * c + d = 0"),
        _case("contract/sub", "contraction",
              cmp(("-", ("*", C("b"), C("c")), ("neg", C("d"))), "<>", L(0)),
              schema, cols, "filter", True, sql="b * c - (-d) <> 0"),
        _case("contract/map", "contraction", e, schema, cols, "map", True,
              sql="b * c + d"),
    ]
    assert not out[0].expected.any() and out[2].expected.all()
    return out


def contraction_sum_data(n):
    """Rows for SUM(b * c + d) whose every partial sum, in any order, is
    exactly representable: contraction triples (each term exactly 0
    unfused, a nonzero 2**-60-sized error fused) interleaved with rows of
    small integers and dyadic fractions (terms are multiples of 1/8 below
    2**12, so sums of up to 2**20 of them stay exact)."""
    tri, _ = contraction_data()
    m = len(tri["b"])
    i = np.arange(n)
    use_tri = i % 3 != 0
    b = np.where(use_tri, tri["b"][i % m], (i % 7).astype(np.float64))
    c = np.where(use_tri, tri["c"][i % m], (i % 5).astype(np.float64))
    d = np.where(use_tri, tri["d"][i % m], (i % 11) / 8.0 - 0.5)
    return {"b": b, "c": c, "d": d}


# ---- family: NaN and infinities --------------------------------------------

def nan_cases():
    schema = {"b": F64, "c": F64}
    vals = [math.nan, math.inf, -math.inf, 0.0, -0.0, 1.5, -1.5]
    cols = {"b": np.array([x for x in vals for _ in vals]),
            "c": np.array([y for _ in vals for y in vals])}
    b, c = C("b"), C("c")
    table = [
        cmp(b, ">", L(0)), ("not", cmp(b, ">", L(0))),
        cmp(b, "=", b), cmp(b, "<>", b),
        cmp(b, "<=", c), ("not", cmp(b, "<=", c)),
        ("between", b, L(-1), L(1)), ("not", ("between", b, L(-1), L(1))),
        ("in", b, [0, 1.5]), ("notin", b, [0, 1.5]),
        cmp(("+", b, c), ">", L(0)), cmp(("*", b, L(0)), "=", L(0)),
        cmp(("-", b, b), "=", L(0)), cmp(("/", b, c), ">=", L(1)),
        ("or", cmp(b, "<", c), cmp(b, ">=", c)),
    ]
    return [_case("nan/" + sql_of(ast), "nan", ast, schema, cols, "filter",
                  gpu=True) for ast in table]


# ---- family: generated arithmetic grammar ----------------------------------

GEN_SCHEMA = {"a": I32, "b": F64, "c": F64, "k": I64, "u": U8}


def gen_data(seed, n=64):
    rnd = random.Random(seed)
    return {"a": np.array([rnd.randint(-40, 40) for _ in range(n)],
                          dtype=I32),
            "b": np.array([rnd.randint(-4000, 4000) / 64.0
                           for _ in range(n)]),
            "c": np.array([round(rnd.uniform(-9, 9), 3) for _ in range(n)]),
            "k": np.array([rnd.randint(-60, 60) for _ in range(n)],
                          dtype=I64),
            "u": np.array([rnd.randint(0, 50) for _ in range(n)], dtype=U8)}


def gen_lit(rnd):
    if rnd.random() < 0.6:
        return L(rnd.randint(-20, 20))
    return L(round(rnd.uniform(-20, 20), 2))


def gen_arith(rnd, depth):
    """Random arithmetic AST of nesting depth <= `depth`."""
    if depth == 0 or rnd.random() < 0.2:
        if rnd.random() < 0.7:
            return C(rnd.choice(list(GEN_SCHEMA)))
        return gen_lit(rnd)
    if rnd.random() < 0.12:
        return ("neg", gen_arith(rnd, depth - 1))
    return (rnd.choice("+-*/"), gen_arith(rnd, depth - 1),
            gen_arith(rnd, depth - 1))


def _has_col(x):
    if x[0] == "col":
        return True
    return any(_has_col(y) for y in x[1:] if isinstance(y, tuple))


def gen_pred(rnd):
    """Arithmetic on either side of a comparison, inside BETWEEN bounds,
    on the left of IN; sometimes two of them under AND / OR / NOT."""
    def leaf():
        kind = rnd.randint(0, 3)
        x = gen_arith(rnd, rnd.randint(1, 3))
        if kind == 0:
            return cmp(x, rnd.choice(CMP_OPS), gen_arith(rnd, 1))
        if kind == 1:
            return cmp(gen_arith(rnd, 1), rnd.choice(CMP_OPS), x)
        if kind == 2:
            return ("between", gen_arith(rnd, 1), gen_arith(rnd, 2), x)
        if x[0] == "col":               # a bare u8 column's IN is the
            x = ("+", x, L(0))          # dictionary-code form: not this
        return (rnd.choice(["in", "notin"]), x,
                [gen_lit(rnd)[1] for _ in range(rnd.randint(1, 4))])
    r = rnd.random()
    if r < 0.6:
        return leaf()
    if r < 0.7:
        return ("not", leaf())
    return (rnd.choice(["and", "or"]), leaf(), leaf())


def generated_cases(count=160, nmaps=60, seed=2024):
    """The fixed seeded batch (compiled once by each tier)."""
    rnd = random.Random(seed)
    cols = gen_data(seed)
    out = []
    while len(out) < count + nmaps:
        kind = "filter" if len(out) < count else "map"
        ast = gen_pred(rnd) if kind == "filter" else \
            gen_arith(rnd, rnd.randint(1, 3))
        if not _has_col(ast):
            continue
        try:
            i = len(out)
            out.append(_case("gen/%03d" % i, "generated", ast, GEN_SCHEMA,
                             cols, kind, gpu=i % 5 == 0))
        except Unsafe:
            continue
    return out


# ---- family: nullable BETWEEN bounds ---------------------------------------

NULL_SCHEMA = {"b": F64, "lo": F64, "hi": F64, "a": I64, "c": I64}
NULL_COLS = ("b", "lo", "hi", "a")


def nullable_data(n, seed=9):
    rng = np.random.default_rng(seed)
    cols = {"b": rng.integers(0, 10, n).astype(np.float64),
            "lo": rng.integers(0, 6, n).astype(np.float64),
            "hi": rng.integers(4, 10, n).astype(np.float64),
            "a": rng.integers(0, 10, n).astype(np.int64),
            "c": rng.integers(0, 10, n).astype(np.int64)}
    valid = {c: rng.random(n) > 0.35 for c in NULL_COLS}
    for c in NULL_COLS:                 # null slots hold 0, as on device
        cols[c] = np.where(valid[c], cols[c], 0).astype(cols[c].dtype)
    return cols, valid


def nullable_asts():
    b, lo, hi, a, c = C("b"), C("lo"), C("hi"), C("a"), C("c")
    return [
        ("not", ("between", b, lo, L(5))),
        ("between", b, lo, L(5)),
        ("not", ("between", b, L(2), hi)),
        ("not", ("between", b, lo, hi)),
        ("between", b, lo, hi),
        ("not", ("between", c, a, L(5))),
        ("not", ("between", c, L(3), a)),
        ("or", ("between", b, lo, hi), cmp(a, ">", L(7))),
        ("or", ("not", ("between", c, lo, hi)), ("isnull", a)),
        ("and", ("not", ("between", a, lo, hi)), ("notnull", b)),
        ("not", ("or", ("between", b, lo, L(7)), ("between", a, L(1), hi))),
        ("not", ("between", b, L(2), L(5))),
    ]


def nullable_cases(n):
    cols, valid = nullable_data(n)
    out = []
    for ast in nullable_asts():
        out.append(Case("null/%d/%s" % (n, sql_of(ast)), "nullable_between",
                        sql_of(ast), NULL_SCHEMA, cols, "filter",
                        pa_expected(ast, cols, valid), ast=ast, gpu=True,
                        nullable=NULL_COLS, valid=valid))
    return out


def all_cases():
    """Every non-null table case (the nullable family needs pyarrow and
    is built by nullable_cases)."""
    return (division_cases() + width_cases() + literal_edge_cases()
            + precedence_cases() + contraction_cases() + nan_cases()
            + generated_cases())
