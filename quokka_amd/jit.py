"""SQL-predicate -> JIT-fused filter kernels (hiprtc).

The reference's partition_fn accepts arbitrary predicates: polars
expressions compiled by sql_utils.evaluate (:86-223) or raw DuckDB SQL
(core.py:157-163). This module covers the same predicate grammar the
reference's TPC-H workload uses (apps/tpc-h/tpch.py filter_sql calls):

  comparisons  = == != <> < <= > >=
  connectives  AND OR NOT, parentheses
  BETWEEN x AND y (inclusive, as DuckDB)
  expr IN (v1, v2, ...) / expr NOT IN (...) — numeric lists, or string
  lists on dict-coded columns (each element resolved through the
  column's StringDict; absent values never match)
  col LIKE 'pat' / NOT LIKE — dict-coded columns only: the SQL pattern
  (% = any run, _ = any char) is matched against the dictionary VALUES
  host-side and becomes a code-set test (no per-row string work on
  device — low-cardinality dictionaries make LIKE a set membership)
  col LIKE 'pat' / NOT LIKE / = 'lit' / <> 'lit' / != 'lit' on a RAW
  string column (schema dtype object, cols entry an ops.StringColumn):
  each distinct (column, pattern, exact) becomes a string term that
  ops.like evaluates on device into a u8 flag column; the predicate sees
  it as one more input, `(vK) != 0` (or `== 0` for the negated forms), so
  AND/OR/NOT and numeric terms compose around it unchanged. IN lists on
  raw string columns are not supported.
  arithmetic   + - * / and unary minus on columns and literals: `/` is
               always f64 division (7 / 2 is 3.5, as Polars and DuckDB
               divide), integer + - * are carried in long long (exact
               whenever the true result fits in int64)
  literals     ints, floats, date 'YYYY-MM-DD' (+/- interval 'N'
               day/month/year, evaluated host-side to date32 days),
               single-quoted strings (equality on dictionary-coded
               columns via the caller's StringDict)

translate() lowers a predicate to a C expression over typed per-row
values v0..vN; JitFilter compiles it with hiprtc into a fused
count+scan+scatter kernel triple for gfx950 (csrc/qk_jit.cpp) and runs
it like ops.filter_col. Literal arithmetic is evaluated in f64 exactly
as the reference SQL evaluates it (e.g. 0.06 - 0.01), preserving the
bit-level comparison semantics.
"""
import ctypes
import datetime
import re

import numpy as np

from . import shim
from .shim import DevColumn, c_u64, c_vp

_EPOCH = datetime.date(1970, 1, 1)
_TYPE_CODE = {np.dtype(np.int32): 0, np.dtype(np.float64): 1,
              np.dtype(np.uint8): 2, np.dtype(np.int64): 3}
RAW_STRING = np.dtype(object)   # schema marker: free-text string column

_TOKEN = re.compile(r"""
    \s*(?:
      (?P<date>date\s*'(\d{4})-(\d{2})-(\d{2})')
    | (?P<interval>interval\s*'(\d+)'\s*(day|month|year)s?)
    | (?P<num>\d+\.\d+|\.\d+|\d+)
    | (?P<str>'[^']*')
    | (?P<op><>|!=|>=|<=|==|=|<|>|\+|-|\*|/|\(|\)|,)
    | (?P<word>[A-Za-z_][A-Za-z0-9_]*)
    )""", re.X | re.I)


def _days(y, m, d):
    return (datetime.date(y, m, d) - _EPOCH).days


class _Tok:
    def __init__(self, kind, val):
        self.kind = kind
        self.val = val

    def __repr__(self):
        return "%s(%r)" % (self.kind, self.val)


def _tokenize(s):
    out, pos = [], 0
    while pos < len(s):
        m = _TOKEN.match(s, pos)
        if not m or m.end() == pos:
            if s[pos:].strip() == "":
                break
            raise ValueError("cannot tokenize %r" % s[pos:pos + 20])
        pos = m.end()
        if m.group("date"):
            out.append(_Tok("date", _days(int(m.group(2)), int(m.group(3)),
                                          int(m.group(4)))))
        elif m.group("interval"):
            n = int(m.group(6))
            unit = m.group(7).lower()
            out.append(_Tok("interval", (n, unit)))
        elif m.group("num"):
            t = m.group("num")
            out.append(_Tok("num", float(t) if "." in t else int(t)))
        elif m.group("str"):
            out.append(_Tok("str", m.group("str")[1:-1]))
        elif m.group("op"):
            out.append(_Tok("op", m.group("op")))
        else:
            w = m.group("word").upper()
            if w in ("AND", "OR", "NOT", "BETWEEN", "IN", "LIKE", "IS",
                     "NULL"):
                out.append(_Tok(w, w))
            else:
                out.append(_Tok("ident", m.group("word")))
    return out


def _last_dom(y, m):
    if m == 12:
        return 31
    return (datetime.date(y, m + 1, 1) - datetime.timedelta(days=1)).day


def _date_add(days, n, unit):
    d = _EPOCH + datetime.timedelta(days=days)
    if unit == "day":
        d = d + datetime.timedelta(days=n)
    else:
        months = n if unit == "month" else 12 * n
        mo = d.month - 1 + months
        y, m = d.year + mo // 12, mo % 12 + 1
        # SQL interval semantics: clamp the day to the target month's end
        d = datetime.date(y, m, min(d.day, _last_dom(y, m)))
    return (d - _EPOCH).days


_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1
_PY_CMP = {"<": lambda x, y: x < y, "<=": lambda x, y: x <= y,
           ">": lambda x, y: x > y, ">=": lambda x, y: x >= y,
           "==": lambda x, y: x == y, "!=": lambda x, y: x != y}


def _lit_val(text):
    """Python value of a literal's text (a repr, maybe parenthesized)."""
    return eval(text, {"__builtins__": {}})


def _lit_text(v):
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            raise ValueError("literal arithmetic leaves the f64 range")
        return repr(v)
    return repr(v)


def _fits_i64(v):
    return isinstance(v, float) or _I64_MIN <= v <= _I64_MAX


def _c_lit(text, as_double=False):
    """C text of a literal. Any int inside int64 but INT64_MIN is its own
    text (C types it int, long or long long: signed). INT64_MIN is spelt
    without the unsigned constant 9223372036854775808; an integer outside
    int64 is only ever emitted as the double it converts to."""
    v = _lit_val(text)
    if isinstance(v, float) or _I64_MIN < v <= _I64_MAX:
        return text
    if v == _I64_MIN:
        return "(-9223372036854775807LL - 1)"
    if as_double:
        try:
            return _lit_text(float(v))
        except OverflowError:
            raise ValueError("integer literal leaves the f64 range")
    raise ValueError("integer literal %d is outside int64 in integer "
                     "arithmetic" % v)


class Translator:
    """Recursive-descent predicate -> C expression over v0..vN.

    With `nullable` (names of columns that may hold NULL) the predicate
    follows SQL three-valued logic: every boolean node is lowered to a
    pair (T = definitely true, F = definitely false) and the emitted
    expression is the root's T, as WHERE keeps only rows that are true.
    A nullable column's validity arrives as a synthetic u8 input
    `__valid_<name>` (self.valid_terms), one more vK like the raw-string
    flag columns. With no nullable column the output is the two-valued
    string, unchanged."""

    def __init__(self, schema, string_dicts=None, nullable=()):
        self.schema = schema            # name -> np dtype
        self.string_dicts = string_dicts or {}
        self.cols = []                  # referenced column names, in order
        # raw-string terms: (flag column name, column, pattern, exact);
        # each flag column is a synthetic u8 entry of self.cols
        self.str_terms = []
        self.nullable = frozenset(nullable or ())
        for name in self.nullable:
            if name not in schema:
                raise ValueError("unknown nullable column %r" % name)
        # validity terms: (flag column name, column)
        self.valid_terms = []
        # nullable columns referenced since the innermost comparison began
        self._touched = []

    def dtype_of(self, name):
        """dtype of a self.cols entry (string-term and validity flag
        columns are u8)."""
        if any(t[0] == name for t in self.str_terms) or \
                any(t[0] == name for t in self.valid_terms):
            return np.dtype(np.uint8)
        return np.dtype(self.schema[name])

    def valid_ref(self, col):
        """-> 'vK' of the validity flag column of nullable column `col`."""
        for name, c in self.valid_terms:
            if c == col:
                return "v%d" % self.cols.index(name)
        name = "__valid_" + col
        while name in self.schema:
            name += "_"
        self.valid_terms.append((name, col))
        self.cols.append(name)
        return "v%d" % self.cols.index(name)

    def _valid_expr(self, touched):
        """V: AND of the validity flags of the nullable columns in
        `touched` ('' when there are none)."""
        seen = []
        for c in touched:
            if c not in seen:
                seen.append(c)
        return " && ".join("((%s) != 0)" % self.valid_ref(c) for c in seen)

    def _leaf3(self, cmp, touched):
        """Two-valued comparison string -> (T, F)."""
        v = self._valid_expr(touched)
        if not v:
            return cmp, "!(%s)" % cmp
        return "(%s) && (%s)" % (v, cmp), "(%s) && !(%s)" % (v, cmp)

    def str_term_ref(self, col, pattern, exact):
        """-> 'vK' of the flag column for this term; identical terms share
        one."""
        for name, c, p, e in self.str_terms:
            if (c, p, e) == (col, pattern, exact):
                return "v%d" % self.cols.index(name)
        name = "__qk_like%d" % len(self.str_terms)
        while name in self.schema:
            name += "_"
        self.str_terms.append((name, col, pattern, exact))
        self.cols.append(name)
        return "v%d" % self.cols.index(name)

    def _p_raw_string(self, col):
        """Comparison of a raw string column, after its identifier."""
        t = self.peek()
        neg = False
        if t and t.kind == "NOT":
            self.take()
            neg = True
            t = self.peek()
        if t and t.kind == "LIKE":
            self.take()
            pat, exact = self.take("str").val, False
        elif t and t.kind == "IN":
            raise ValueError("IN list on raw string column %r is not "
                             "supported" % col)
        elif t and not neg and t.kind == "op" and \
                t.val in ("=", "==", "!=", "<>"):
            self.take()
            neg = t.val in ("!=", "<>")
            pat, exact = self.take("str").val, True
        else:
            raise ValueError("raw string column %r supports only LIKE, "
                             "NOT LIKE, =, <> and != with a string "
                             "literal" % col)
        ref = self.str_term_ref(col, pat, exact)
        raise _Folded("(%s) %s 0" % (ref, "==" if neg else "!="))

    def col_ref(self, name):
        if name not in self.schema:
            raise ValueError("unknown column %r" % name)
        if name not in self.cols:
            self.cols.append(name)
        if name in self.nullable:
            self._touched.append(name)
        return "v%d" % self.cols.index(name), self.schema[name]

    def translate(self, s):
        self.toks = _tokenize(s)
        self.i = 0
        expr = self.p_or()
        if self.i != len(self.toks):
            raise ValueError("trailing tokens: %r" % self.toks[self.i:])
        if self.nullable:
            return expr[0]              # WHERE keeps the definitely-true
        return expr

    def peek(self):
        return self.toks[self.i] if self.i < len(self.toks) else None

    def take(self, kind=None):
        t = self.peek()
        if t is None or (kind and t.kind != kind):
            raise ValueError("expected %s at %r" % (kind, t))
        self.i += 1
        return t

    def p_or(self):
        left = self.p_and()
        while self.peek() and self.peek().kind == "OR":
            self.take()
            right = self.p_and()
            if self.nullable:           # (T, F) pairs
                left = ("(%s) || (%s)" % (left[0], right[0]),
                        "(%s) && (%s)" % (left[1], right[1]))
            else:
                left = "(%s) || (%s)" % (left, right)
        return left

    def p_and(self):
        left = self.p_not()
        while self.peek() and self.peek().kind == "AND":
            self.take()
            right = self.p_not()
            if self.nullable:
                left = ("(%s) && (%s)" % (left[0], right[0]),
                        "(%s) || (%s)" % (left[1], right[1]))
            else:
                left = "(%s) && (%s)" % (left, right)
        return left

    def p_not(self):
        if self.peek() and self.peek().kind == "NOT":
            self.take()
            inner = self.p_not()
            if self.nullable:
                return inner[1], inner[0]
            return "!(%s)" % inner
        return self.p_cmp()

    def p_cmp(self):
        """One comparison or parenthesized boolean: a C string, or its
        (T, F) pair when there are nullable columns."""
        outer, self._touched = self._touched, []
        try:
            try:
                res = self._p_cmp_inner()
            except _Folded as f:
                res = f.expr
            if self.nullable and not isinstance(res, tuple):
                res = self._leaf3(res, self._touched)
            return res
        finally:
            self._touched = outer

    def _p_is_null(self):
        """After an arithmetic operand: 'IS [NOT] NULL' over the nullable
        columns it references. Without any, every value is non-null and
        the test folds to a constant."""
        self.take("IS")
        neg = False
        if self.peek() and self.peek().kind == "NOT":
            self.take()
            neg = True
        self.take("NULL")
        v = self._valid_expr(self._touched)
        if not v:
            res = ("(0)", "(1)")
        else:
            res = ("!(%s)" % v, "(%s)" % v)
        if neg:
            res = (res[1], res[0])
        return res if self.nullable else res[0]

    def _p_cmp_inner(self):
        t = self.peek()
        if t and t.kind == "op" and t.val == "(":
            # lookahead: parenthesized boolean vs arithmetic group
            save = self.i
            try:
                self.take()
                inner = self.p_or()
                close = self.take("op")
                if close.val != ")":
                    raise ValueError("expected )")
                nxt = self.peek()
                if nxt is None or nxt.kind in ("AND", "OR") or \
                        (nxt.kind == "op" and nxt.val == ")"):
                    if self.nullable:
                        return "(%s)" % inner[0], "(%s)" % inner[1]
                    return "(%s)" % inner
                raise ValueError("arith reparse")
            except ValueError:
                self.i = save
                self._touched = []
        left, lt = self.p_arith()
        t = self.peek()
        if t and t.kind == "IS":
            return self._p_is_null()
        if t and (t.kind == "IN" or
                  (t.kind == "NOT" and self.i + 1 < len(self.toks)
                   and self.toks[self.i + 1].kind == "IN")):
            neg = t.kind == "NOT"
            self.take()
            if neg:
                self.take("IN")
            els = self._p_in_list(allow_str=False)
            # an element no value of `left` can equal (an integer outside
            # int64 against an integer operand) folds to (0) and is dropped
            terms = [self._cmp(left, lt, "==", _lit_text(e), "lit")
                     for e in els]
            body = " || ".join("(%s)" % c for c in terms if c != "(0)") \
                or "(0)"
            return ("!(%s)" if neg else "(%s)") % body
        if t and t.kind == "BETWEEN":
            self.take()
            n_left = len(self._touched)
            lo, lot = self.p_arith()
            n_lo = len(self._touched)
            self.take("AND")
            hi, hit = self.p_arith()
            ge = self._cmp(left, lt, ">=", lo, lot)
            le = self._cmp(left, lt, "<=", hi, hit)
            if len(self._touched) > n_left:
                # a nullable bound: BETWEEN is the Kleene AND of its two
                # comparisons, each unknown only through its own operands
                # (lo NULL and left > hi is FALSE, not unknown)
                tl, fl = self._leaf3(ge, self._touched[:n_lo])
                th, fh = self._leaf3(le, self._touched[:n_left]
                                     + self._touched[n_lo:])
                return ("((%s) && (%s))" % (tl, th),
                        "((%s) || (%s))" % (fl, fh))
            return "((%s) && (%s))" % (ge, le)
        op = self.take("op").val
        if op not in ("<", "<=", ">", ">=", "=", "==", "<>", "!="):
            raise ValueError("expected comparison operator, got %r" % op)
        cop = {"=": "==", "<>": "!="}.get(op, op)
        right, rt = self.p_arith()
        return self._cmp(left, lt, cop, right, rt)

    def _p_in_list(self, allow_str):
        """Parse IN's '(v1, v2, ...)' — literal numbers (and strings when
        allow_str) only."""
        p = self.take("op")   # caller already consumed IN (and NOT)
        if p.val != "(":
            raise ValueError("expected ( after IN")
        out = []
        while True:
            t = self.take()
            neg = False
            if t.kind == "op" and t.val in ("-", "+"):
                neg = t.val == "-"
                t = self.take()
            if t.kind == "num":
                out.append(-t.val if neg else t.val)
            elif t.kind == "date" and not neg:
                out.append(t.val)
            elif t.kind == "str" and allow_str and not neg:
                out.append(t.val)
            else:
                raise ValueError("bad IN list element %r" % (t,))
            t = self.take("op")
            if t.val == ")":
                break
            if t.val != ",":
                raise ValueError("expected , or ) in IN list")
        if not out:
            raise ValueError("empty IN list")
        return out

    def p_arith(self):
        left, lt = self.p_term()
        while self.peek() and self.peek().kind == "op" and \
                self.peek().val in "+-":
            op = self.take().val
            right, rt = self.p_term()
            left, lt = self._fold(left, lt, op, right, rt)
        return left, lt

    def p_term(self):
        left, lt = self.p_atom()
        while self.peek() and self.peek().kind == "op" and \
                self.peek().val in "*/":
            op = self.take().val
            right, rt = self.p_atom()
            left, lt = self._fold(left, lt, op, right, rt)
        return left, lt

    # Arithmetic operands carry a type tag: "lit" (a folded literal, its
    # text the Python repr), "n" (an i32/u8 column), "l" (long long) or
    # "d" (double). Integer arithmetic is carried in long long, so it is
    # exact whenever the true result fits in int64; `/` is always f64
    # division, as the reference's SQL engines divide.
    @staticmethod
    def _fold(l, lt, op, r, rt):
        # host-fold literal arithmetic in f64, exactly as the reference
        # SQL engine evaluates constant expressions (bit-identical bounds)
        if lt == "lit" and rt == "lit":
            try:
                v = eval("(%s) %s (%s)" % (l, op, r))
            except (ZeroDivisionError, OverflowError) as e:
                raise ValueError("cannot fold (%s) %s (%s): %s"
                                 % (l, op, r, e))
            return _lit_text(v), "lit"
        lf = lt == "d" or (lt == "lit" and isinstance(_lit_val(l), float))
        rf = rt == "d" or (rt == "lit" and isinstance(_lit_val(r), float))
        if lt == "lit":
            l = _c_lit(l, as_double=rf)
        if rt == "lit":
            r = _c_lit(r, as_double=lf)
        if lf or rf:
            return "(%s) %s (%s)" % (l, op, r), "d"
        if op == "/":
            return "(double)(%s) / (double)(%s)" % (l, r), "d"
        if lt == "n" or rt == "n":
            if lt == "n":
                l = "(long long)(%s)" % l
            if rt == "n":
                r = "(long long)(%s)" % r
        return "(%s) %s (%s)" % (l, op, r), "l"

    @staticmethod
    def _cmp(l, lt, cop, r, rt):
        """Two-valued C text of `l cop r`. An integer literal outside
        int64 never reaches the C text: against an integer operand the
        comparison is decided here, as the mathematical integers decide
        it; against a double it becomes the double it converts to."""
        lv = _lit_val(l) if lt == "lit" else None
        rv = _lit_val(r) if rt == "lit" else None
        if lt == "lit" and rt == "lit":
            if _fits_i64(lv) and _fits_i64(rv):
                return "(%s) %s (%s)" % (_c_lit(l), cop, _c_lit(r))
            return "(1)" if _PY_CMP[cop](lv, rv) else "(0)"
        if lt == "lit" and not _fits_i64(lv):
            if rt == "d":
                return "(%s) %s (%s)" % (_c_lit(l, True), cop, r)
            return "(1)" if _PY_CMP[cop](lv, 0) else "(0)"
        if rt == "lit" and not _fits_i64(rv):
            if lt == "d":
                return "(%s) %s (%s)" % (l, cop, _c_lit(r, True))
            # every int64 lies on the same side of rv as 0 does
            return "(1)" if _PY_CMP[cop](0, rv) else "(0)"
        if lt == "lit":
            l = _c_lit(l)
        if rt == "lit":
            r = _c_lit(r)
        return "(%s) %s (%s)" % (l, cop, r)

    def p_atom(self):
        t = self.take()
        if t.kind == "op" and t.val in ("-", "+"):
            e, et = self.p_atom()
            if t.val == "-":
                if et == "lit":
                    return _lit_text(-_lit_val(e)), "lit"
                if et == "n":
                    return "(-(long long)(%s))" % e, "l"
                return "(-(%s))" % e, et
            return e, et
        if t.kind == "op" and t.val == "(":
            e, et = self.p_arith()
            c = self.take("op")
            if c.val != ")":
                raise ValueError("expected )")
            return "(%s)" % e, et
        if t.kind == "num":
            return _lit_text(t.val), "lit"
        if t.kind == "date":
            days = t.val
            # date +/- interval chains, folded host-side
            while self.peek() and self.peek().kind == "op" and \
                    self.peek().val in "+-" and self.i + 1 < len(self.toks) \
                    and self.toks[self.i + 1].kind == "interval":
                op = self.take().val
                n, unit = self.take("interval").val
                days = _date_add(days, n if op == "+" else -n, unit)
            return repr(days), "lit"
        if t.kind == "str":
            # a string literal is consumed by its dict-coded or raw string
            # column partner; anywhere else it has no C form
            raise ValueError("string literal %r needs a string column "
                             "partner" % t.val)
        if t.kind == "ident":
            if t.val in self.schema and self.schema[t.val] == RAW_STRING:
                if t.val in self.nullable:
                    raise ValueError("raw string column %r is nullable: "
                                     "null strings are not supported"
                                     % t.val)
                self._p_raw_string(t.val)      # raises _Folded
            ref, dtype = self.col_ref(t.val)
            # string equality: partner literal becomes the dict code
            nxt = self.peek()
            if dtype == np.dtype(np.uint8) and nxt and (
                    nxt.kind == "LIKE" or
                    (nxt.kind == "NOT" and self.i + 1 < len(self.toks)
                     and self.toks[self.i + 1].kind == "LIKE")):
                neg = nxt.kind == "NOT"
                self.take()
                if neg:
                    self.take("LIKE")
                p = self.take("str")
                sd = self.string_dicts.get(t.val)
                if sd is None:
                    raise ValueError("LIKE on %r needs its StringDict"
                                     % t.val)
                import re as _re
                rx = _re.compile(
                    "^" + "".join(
                        ".*" if ch == "%" else "." if ch == "_"
                        else _re.escape(ch) for ch in p.val) + "$", _re.S)
                codes = [c for v, c in sd.codes.items() if rx.match(v)]
                if not codes:
                    raise _Folded("(0)" if not neg else "(1)")
                body = " || ".join("((%s) == (%d))" % (ref, c)
                                   for c in sorted(codes))
                raise _Folded(("!(%s)" if neg else "(%s)") % body)
            if dtype == np.dtype(np.uint8) and nxt and (
                    nxt.kind == "IN" or
                    (nxt.kind == "NOT" and self.i + 1 < len(self.toks)
                     and self.toks[self.i + 1].kind == "IN")):
                neg = nxt.kind == "NOT"
                self.take()
                if neg:
                    self.take("IN")
                codes = []
                for el in self._p_in_list(allow_str=True):
                    if isinstance(el, str):
                        sd = self.string_dicts.get(t.val)
                        if sd is None:
                            raise ValueError(
                                "string IN list on %r needs its "
                                "StringDict" % t.val)
                        # absent literal: no code can ever equal it — drop
                        # it (a sentinel code could collide with a later
                        # legitimate dictionary entry)
                        c = sd.codes.get(el)
                        if c is not None:
                            codes.append(c)
                    else:
                        codes.append(int(el))
                if not codes:
                    raise _Folded("(1)" if neg else "(0)")
                body = " || ".join("((%s) == (%d))" % (ref, c)
                                   for c in codes)
                raise _Folded(("!(%s)" if neg else "(%s)") % body)
            if dtype == np.dtype(np.uint8) and nxt and nxt.kind == "op" \
                    and nxt.val in ("=", "==", "!=", "<>"):
                save = self.i
                op = self.take().val
                p = self.peek()
                if p is not None and p.kind == "str":
                    self.take()
                    sd = self.string_dicts.get(t.val)
                    if sd is None:
                        raise ValueError(
                            "string literal compare on %r needs its "
                            "StringDict" % t.val)
                    code = sd.codes.get(p.val)
                    if code is None:
                        # absent value: constant false for =, true for != —
                        # never a sentinel code (it could collide with a
                        # later legitimate dictionary entry)
                        raise _Folded("(1)" if op in ("!=", "<>") else "(0)")
                    cop = {"=": "==", "<>": "!="}.get(op, op)
                    raise _Folded("(%s) %s (%d)" % (ref, cop, code))
                self.i = save
            if dtype not in _TYPE_CODE:
                raise ValueError("column %r of dtype %s has no arithmetic"
                                 % (t.val, dtype))
            return ref, {0: "n", 1: "d", 2: "n", 3: "l"}[_TYPE_CODE[dtype]]
        raise ValueError("unexpected token %r" % t)


class _Folded(Exception):
    """Early-return carrier for already-complete comparisons."""

    def __init__(self, expr):
        self.expr = expr


def translate(predicate, schema, string_dicts=None, nullable=()):
    """-> (c_expr, ordered column names). schema: name -> np dtype.
    nullable: names of columns that may hold NULL (SQL three-valued
    logic; each one referenced adds a `__valid_<name>` u8 input)."""
    tr = Translator(schema, string_dicts, nullable)
    return tr.translate(predicate), tr.cols


def translate_terms(predicate, schema, string_dicts=None):
    """translate() plus the raw-string terms: -> (c_expr, columns,
    str_terms). Each term is (flag_column, column, pattern, exact); its
    flag column is a synthetic u8 entry of `columns` that ops.like fills
    at run time."""
    tr = Translator(schema, string_dicts)
    return tr.translate(predicate), tr.cols, tr.str_terms


def _eval_str_terms(str_terms, cols, stream):
    """Run each string term's LIKE kernel -> {flag column: DevColumn u8}."""
    from . import ops
    flags = {}
    for name, col, pattern, exact in str_terms:
        sc = cols[col]
        if not isinstance(sc, ops.StringColumn):
            raise TypeError("column %r is a raw string in the schema: "
                            "cols[%r] must be an ops.StringColumn"
                            % (col, col))
        flags[name] = ops.like(sc, pattern, exact=exact, stream=stream)
    return flags


def _eval_valid_terms(valid_terms, cols, stream):
    """Expand each nullable input's bitmap (qk_valid_to_u8) ->
    {validity flag column: DevColumn u8}."""
    from . import ops
    flags = {}
    for name, col in valid_terms:
        nc = cols[col]
        if not isinstance(nc, ops.NullableColumn):
            raise TypeError("column %r is declared nullable: cols[%r] "
                            "must be an ops.NullableColumn" % (col, col))
        flags[name] = nc.valid_flags(stream)
    return flags


def translate_arith(expr, schema, translator=None):
    """Arithmetic expression (no comparisons) -> (c_expr, columns)."""
    tr = translator or Translator(schema)
    tr.toks = _tokenize(expr)
    tr.i = 0
    e, _ = tr.p_arith()
    if tr.i != len(tr.toks):
        raise ValueError("trailing tokens in %r" % expr)
    return e, tr.cols


_AGG_SQL = re.compile(r"^\s*(sum|count|min|max)\s*\(\s*(.*?)\s*\)\s*"
                      r"(?:as\s+([A-Za-z_][A-Za-z0-9_]*))?\s*$",
                      re.I | re.S)


class JitAggregate:
    """JIT-fused scan + small-cardinality group-by partial aggregate:
    the generalization of the hand-written Q1 kernel (csrc qk_jit_agg_*).

    group_keys: list of (column_name, cardinality) over u8 code columns;
    aggs: list of 'SUM(expr)' / 'COUNT(*)' strings (the map-side partial
    forms the two-phase rewrite emits, sql_utils.py:299-413);
    predicate: optional filter_sql string fused into the same pass.
    run() ACCUMULATES into a DevBuffer of ngroups*naggs f64 (executor
    state semantics, like qk_q1_agg). A row whose key is outside
    [0, cardinality) contributes to no group.

    nullable: names of columns that may hold NULL (run() takes an
    ops.NullableColumn for each). The predicate follows SQL three-valued
    logic, SUM/MIN/MAX skip rows whose expression is NULL and COUNT(expr)
    counts the rows where it is not; COUNT(*) counts rows. A group whose
    inputs were ALL null reads back as the aggregate's identity (0 /
    +inf / -inf), not as NULL: put COUNT(col) beside it to tell the two
    apart. Group keys must be non-null; a nullable one raises TypeError.

    NaN inputs (DESIGN.md §3a''''''): SUM with a NaN is NaN; MIN/MAX skip
    NaN beside other values, and a group whose MIN/MAX inputs were all NaN
    reads back as NaN, not as the identity."""

    def __init__(self, schema, group_keys, aggs, predicate=None,
                 string_dicts=None, nullable=()):
        tr = Translator(schema, string_dicts, nullable)
        pred_expr = ""
        if predicate:
            pred_expr = tr.translate(predicate)
        self.group_keys = list(group_keys or [])
        self.ngroups = 1
        gparts = []
        for name, card in self.group_keys:
            if name in tr.nullable:
                raise TypeError("group key %r is nullable: null group keys "
                                "are not supported" % name)
            ref, dt = tr.col_ref(name)
            if dt not in (np.dtype(np.uint8), np.dtype(np.int32)):
                raise TypeError("group keys must be u8 code or small-"
                                "cardinality i32 columns (values in "
                                "[0, cardinality), e.g. nation keys)")
            gparts.append((ref, card))
            self.ngroups *= int(card)
        gexpr = "0"   # [] group keys -> one grand-aggregate group
        for ref, card in gparts:
            gexpr = "(%s) * %d + (int)%s" % (gexpr, card, ref)
        if len(gparts) > 1:
            # a key outside [0, cardinality) would alias into another
            # group's id: such a row gets id -1 and reaches no group, as
            # with one key (where the id is the key itself)
            gexpr = "(%s) ? (%s) : -1" % (
                " && ".join("(unsigned)(%s) < %du" % (ref, card)
                            for ref, card in gparts), gexpr)
        self.group_expr = gexpr
        self.agg_names = []
        self.agg_ops = []            # 0=SUM, 1=MIN, 2=MAX (COUNT -> SUM 1)
        agg_exprs = []
        for a in aggs:
            m = _AGG_SQL.match(a)
            if not m:
                raise ValueError("unsupported aggregate %r (SUM/MIN/MAX"
                                 "(expr) / COUNT(*))" % a)
            fn, inner, alias = m.group(1).lower(), m.group(2), m.group(3)
            tr._touched = []
            if fn == "count":
                e = "1.0"
                if tr.nullable and inner != "*":
                    translate_arith(inner, schema, tr)
                self.agg_ops.append(0)
            else:
                e, _ = translate_arith(inner, schema, tr)
                self.agg_ops.append({"sum": 0, "min": 1, "max": 2}[fn])
            v = tr._valid_expr(tr._touched)
            if v and self.agg_ops[-1]:
                # a NULL input leaves a MIN/MAX accumulator alone: it is
                # spelt as the no-input pattern, which no value can be
                # taken for once qk_num has made every NaN the canonical
                # one (csrc gen_agg_source does that for expressions that
                # do not name QK_MM_SKIP)
                e = "((%s) ? qk_num((double)(%s)) : QK_MM_SKIP)" % (v, e)
            elif v:
                # a NULL input leaves the accumulator alone
                e = "((%s) ? (double)(%s) : 0.0)" % (v, e)
            agg_exprs.append(e)
            self.agg_names.append(alias or a.strip())
        self.naggs = len(agg_exprs)
        self.cols = tr.cols
        self.str_terms = tr.str_terms
        self.valid_terms = tr.valid_terms
        self.dtypes = [tr.dtype_of(c) for c in self.cols]

        lib = shim._lib
        lib.qk_jit_agg_build.argtypes = [
            ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int),
            ctypes.c_int, ctypes.POINTER(ctypes.c_int), c_vp]
        lib.qk_jit_last_error.restype = ctypes.c_char_p
        exprs_c = (ctypes.c_char_p * self.naggs)(
            *[e.encode() for e in agg_exprs])
        types_c = (ctypes.c_int * len(self.cols))(
            *[_TYPE_CODE[d] for d in self.dtypes])
        ops_c = (ctypes.c_int * self.naggs)(*self.agg_ops)
        prog = c_vp(0)
        rc = lib.qk_jit_agg_build(pred_expr.encode(), gexpr.encode(),
                                  self.ngroups, self.naggs, exprs_c,
                                  ops_c, len(self.cols), types_c,
                                  ctypes.byref(prog))
        if rc != 0:
            raise shim.QkError("jit agg build failed: %s"
                               % lib.qk_jit_last_error().decode())
        self.prog = prog

    def make_acc(self):
        """Accumulator initialized to 0 for SUM/COUNT and to the no-input
        pattern of MIN/MAX slots (ops.MM_NONE_BITS), which read() gives
        back as the identity +inf / -inf."""
        from .shim import DevBuffer, c_vp as _vp
        from .ops import MM_NONE_BITS
        b = DevBuffer(self.ngroups * self.naggs * 8)
        init = np.zeros((self.ngroups, self.naggs), dtype=np.uint64)
        for a, o in enumerate(self.agg_ops):
            if o:
                init[:, a] = MM_NONE_BITS
        flat = np.ascontiguousarray(init.reshape(-1))
        shim.call("qk_h2d", b.ptr, flat.ctypes.data_as(_vp),
                  c_u64(flat.nbytes))
        return b

    def run(self, cols, acc, stream=None):
        lib = shim._lib
        lib.qk_jit_agg_run.argtypes = [c_vp, c_vp, c_u64,
                                       ctypes.POINTER(c_vp), c_vp]
        flags = _eval_str_terms(self.str_terms, cols, stream)
        flags.update(_eval_valid_terms(self.valid_terms, cols, stream))
        if flags:
            cols = dict(cols, **flags)
        n = cols[self.cols[0]].n
        ptrs = (c_vp * len(self.cols))(*[cols[c].ptr for c in self.cols])
        sh = stream.handle if stream else None
        rc = lib.qk_jit_agg_run(self.prog, sh, c_u64(n), ptrs, acc.ptr)
        if flags:
            # the flag columns go back to the pool: the kernel reading
            # them must have finished first
            shim.call("qk_stream_sync", sh)
            for f in flags.values():
                f.free()
        if rc != 0:
            raise shim.QkError("jit agg run failed: %s"
                               % lib.qk_jit_last_error().decode())

    def read(self, acc):
        """d2h -> (ngroups, naggs) f64. A MIN/MAX that met no value reads
        as +inf / -inf; one that met only NaN reads as NaN."""
        from .ops import MM_NONE_BITS
        host = np.zeros(self.ngroups * self.naggs, dtype=np.float64)
        shim.call("qk_d2h", host.ctypes.data_as(c_vp), acc.ptr,
                  c_u64(host.nbytes))
        out = host.reshape(self.ngroups, self.naggs)
        for a, o in enumerate(self.agg_ops):
            if o:
                none = out[:, a].view(np.uint64) == MM_NONE_BITS
                out[none, a] = np.inf if o == 1 else -np.inf
        return out

    def free(self):
        if self.prog:
            shim._lib.qk_jit_filter_free(self.prog)
            self.prog = None


class JitMap:
    """JIT elementwise transform: out f64 column = expr(columns) per row
    (the reference's transform_sql / with_columns_sql batch expressions,
    datastream.py:652-815; generalizes the static qk_mul_1md)."""

    def __init__(self, expr, schema):
        self.expr, self.cols = translate_arith(expr, schema)
        self.dtypes = [np.dtype(schema[c]) for c in self.cols]
        lib = shim._lib
        lib.qk_jit_map_build.argtypes = [ctypes.c_char_p, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int), c_vp]
        lib.qk_jit_last_error.restype = ctypes.c_char_p
        types_c = (ctypes.c_int * len(self.cols))(
            *[_TYPE_CODE[d] for d in self.dtypes])
        prog = c_vp(0)
        rc = lib.qk_jit_map_build(self.expr.encode(), len(self.cols),
                                  types_c, ctypes.byref(prog))
        if rc != 0:
            raise shim.QkError("jit map build failed: %s"
                               % lib.qk_jit_last_error().decode())
        self.prog = prog

    def run(self, cols, stream=None, out=None):
        lib = shim._lib
        lib.qk_jit_map_run.argtypes = [c_vp, c_vp, c_u64,
                                       ctypes.POINTER(c_vp), c_vp]
        n = cols[self.cols[0]].n
        if out is None:
            out = DevColumn(np.float64, max(1, n))
            out.n = n
        ptrs = (c_vp * len(self.cols))(*[cols[c].ptr for c in self.cols])
        sh = stream.handle if stream else None
        rc = lib.qk_jit_map_run(self.prog, sh, c_u64(n), ptrs, out.ptr)
        if rc != 0:
            raise shim.QkError("jit map run failed: %s"
                               % lib.qk_jit_last_error().decode())
        return out

    def free(self):
        if self.prog:
            shim._lib.qk_jit_filter_free(self.prog)
            self.prog = None


class JitFilter:
    """Compiled fused filter for one predicate over a fixed schema."""

    def __init__(self, predicate, schema, string_dicts=None, nullable=()):
        """nullable: names of columns that may hold NULL; run() then takes
        an ops.NullableColumn for each and keeps the rows for which the
        predicate is TRUE under SQL three-valued logic."""
        tr = Translator(schema, string_dicts, nullable)
        self.expr = tr.translate(predicate)
        self.cols, self.str_terms = tr.cols, tr.str_terms
        self.valid_terms = tr.valid_terms
        self.dtypes = [tr.dtype_of(c) for c in self.cols]
        types = (ctypes.c_int * len(self.cols))(
            *[_TYPE_CODE[d] for d in self.dtypes])
        prog = c_vp(0)
        lib = shim._lib
        lib.qk_jit_filter_build.argtypes = [ctypes.c_char_p, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_int),
                                            c_vp]
        lib.qk_jit_last_error.restype = ctypes.c_char_p
        rc = lib.qk_jit_filter_build(self.expr.encode(), len(self.cols),
                                     types, ctypes.byref(prog))
        if rc != 0:
            raise shim.QkError("jit build failed: %s"
                               % lib.qk_jit_last_error().decode())
        self.prog = prog

    def run(self, cols, stream=None):
        """cols: dict name -> DevColumn (must include every referenced
        column, all same length; an ops.StringColumn for each raw string
        column). Returns (idx DevColumn u32, count)."""
        from . import ops
        flags = _eval_str_terms(self.str_terms, cols, stream)
        flags.update(_eval_valid_terms(self.valid_terms, cols, stream))
        if flags:
            cols = dict(cols, **flags)
        n = cols[self.cols[0]].n
        ptrs = (c_vp * len(self.cols))(
            *[cols[c].ptr for c in self.cols])
        idx = DevColumn(np.uint32, max(1, n))
        cnt = ops._count_buf()
        lib = shim._lib
        lib.qk_jit_filter_run.argtypes = [c_vp, c_vp, c_u64,
                                          ctypes.POINTER(c_vp), c_vp, c_vp]
        sh = stream.handle if stream else None
        rc = lib.qk_jit_filter_run(self.prog, sh, c_u64(n), ptrs, idx.ptr,
                                   cnt.ptr)
        if rc != 0:
            for f in flags.values():
                f.free()
            raise shim.QkError("jit run failed: %s"
                               % lib.qk_jit_last_error().decode())
        if stream:
            stream.sync()
        k = ops._read_u64(cnt)
        cnt.free()
        for f in flags.values():
            f.free()
        idx.n = k
        return idx, k

    def free(self):
        if self.prog:
            shim._lib.qk_jit_filter_free(self.prog)
            self.prog = None
