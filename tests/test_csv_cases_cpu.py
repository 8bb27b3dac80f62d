"""The CSV case tables (tests/_csv_cases.py) are right, proven without a
GPU: every accept value comes from an independent parser, every reject
text is refused by one or is tagged "stricter by contract" for a reason
this file re-derives from the text."""
import calendar
import csv
import datetime
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _csv_cases as C  # noqa: E402


def strict_float(field):
    """The independent f64 parser: float() is strtod on the text. What it
    reads beyond plain decimals (exponents, inf, blanks) is tagged."""
    return float(field.decode())


def test_f64_accept_values_and_ranges():
    fields = C.F64_ACCEPT_FIXED + C.f64_random_fields()
    assert len(fields) == len(C.F64_ACCEPT_FIXED) + C.N_RANDOM
    seen_k, seen_nd = set(), set()
    for f in fields:
        v = strict_float(f)                     # parses at all
        assert np.isfinite(v)
        sig, dec = C.f64_digit_counts(f)
        assert sig <= C.F64_MAX_SIG and dec <= C.F64_MAX_DEC, f
        assert set(f) <= set(b"+-.0123456789"), f
        assert any(48 <= ch <= 57 for ch in f), f
        seen_k.add(dec)
        seen_nd.add(sig)
    # the generator reaches every digit count and every scale
    assert seen_nd >= set(range(1, 16)) and seen_k == set(range(19))
    # -0 keeps its sign in the expectation: bit patterns, not ==
    bits = C.f64_bits([strict_float(f) for f in (b"0", b"-0", b"-0.0")])
    assert bits[0] == 0 and bits[1] == bits[2] == 1 << 63
    signs = {f[:1] for f in fields}
    assert b"+" in signs and b"-" in signs
    assert any(f.lstrip(b"+-").startswith(b"00") for f in fields)


def test_f64_reject_cases():
    for f, tag in C.F64_REJECT:
        if tag is None:
            with pytest.raises(ValueError):
                strict_float(f)
            continue
        v = strict_float(f)          # the tag is needed: float() reads it
        if tag == C.STRICTER_DIGITS:
            sig, dec = C.f64_digit_counts(f)
            assert sig > 15 or dec > 18, f
            # one digit fewer would be inside the range
            assert sig <= 16 and dec <= 19, f
        else:
            assert tag == C.STRICTER_SYNTAX
            plain = set(f) <= set(b"+-.0123456789")
            assert not plain or not np.isfinite(v), f


def test_i64_cases():
    for f in C.I64_ACCEPT:
        v = int(f.decode())
        assert -(1 << 63) <= v < (1 << 63)
        assert len(f.lstrip(b"+-")) <= C.I64_MAX_DIGITS
    assert max(len(f.lstrip(b"+-")) for f in C.I64_ACCEPT) == 18
    for f, tag in C.I64_REJECT:
        if tag is None:
            with pytest.raises(ValueError):
                int(f.decode())
            continue
        int(f.decode())              # the tag is needed: int() reads it
        if tag == C.STRICTER_DIGITS:
            assert len(f.lstrip(b"+-")) == 19 and f.lstrip(b"+-").isdigit()
        elif tag == C.STRICTER_ASCII:
            assert not f.isascii()
        else:
            assert tag == C.STRICTER_SYNTAX and f != f.strip()


def test_date_accept_values_and_coverage():
    days = C.date_accept_days()
    texts = C.date_texts(days)
    assert len(days) == len(texts) >= C.N_RANDOM + 14 * 365
    # expectation as the issue defines it, and a second calendar agrees
    want = (texts.astype("datetime64[D]") - C.EPOCH).astype(np.int64)
    assert np.array_equal(want, days)
    for t, d in list(zip(texts, days))[::37]:
        assert C.ref_date(t.encode()) == d, t
    have = set(texts.tolist())
    for y in C.DATE_YEARS:
        for m in range(1, 13):               # every month end
            last = calendar.monthrange(y, m)[1]
            assert "%04d-%02d-%02d" % (y, m, last) in have
            assert "%04d-%02d-01" % (y, m) in have
    # both sides of every leap rule: /4, /100, /400
    assert "2024-02-29" in have and "1972-02-29" in have
    assert "2023-02-28" in have and "2023-02-29" not in have
    assert "1900-02-28" in have and "1900-02-29" not in have
    assert "2100-02-28" in have and "2100-02-29" not in have
    assert "2000-02-29" in have and "1600-02-29" in have
    assert "2400-02-29" in have
    assert min(have) == "0001-01-01" and max(have) == "9999-12-31"
    assert days.min() == C.DAY_LO and days.max() == C.DAY_HI


def test_date_reject_cases():
    for f in C.DATE_REJECT:
        with pytest.raises(ValueError):
            C.ref_date(f)
    rej = set(C.DATE_REJECT)
    for must in (b"2023-02-29", b"1900-02-29", b"2100-02-29", b"2023-02-30",
                 b"2023-04-31", b"2023-06-31", b"2023-09-31", b"2023-11-31"):
        assert must in rej
        # shape is fine: only the calendar refuses them
        y, m, d = (int(x) for x in must.decode().split("-"))
        assert 1 <= m <= 12 and 1 <= d <= 31
        with pytest.raises(ValueError):
            datetime.date(y, m, d)


def test_dict_cases():
    cands = [c.encode() for c in C.DICT_CANDS]
    assert len(set(cands)) == len(cands)
    for f in C.DICT_REJECT:
        assert f not in cands
    # the rejects that the (first 8 bytes, length) key cannot see
    key = lambda b: (b[:8], min(len(b), 255))
    assert key(b"AUTOMOBILX") == key(b"AUTOMOBILE")
    assert key(b"MACHINERZ") == key(b"MACHINERY")
    long_ = C.DICT_LONG.encode()
    for f in C.DICT_LONG_REJECT:
        assert f != long_ and key(f) == key(long_)
    assert C.DICT_LONG_REJECT[1][200] != long_[200]
    assert C.DICT_LONG_REJECT[1][:200] == long_[:200]
    assert key(b"CUSTOMER#1") == key(b"CUSTOMER#2")
    for f in C.DICT_TWINS_REJECT:
        assert f.decode() not in C.DICT_TWINS


def test_all_cases_shape():
    n = {"f64": 0, "i64": 0, "date": 0, "dict": 0}
    rejects = 0
    for field, typ, want in C.all_cases():
        assert isinstance(field, bytes)
        n[typ] += 1
        rejects += want == C.REJECT
    assert n["f64"] > C.N_RANDOM and n["date"] > C.N_RANDOM
    assert rejects == (len(C.F64_REJECT) + len(C.I64_REJECT) +
                       len(C.DATE_REJECT) + len(C.DICT_REJECT))


@pytest.mark.parametrize("total", [(1 << 20) + 4097, (3 << 20) + 131])
def test_quoted_buffer_builder(total):
    """The quoted-index buffer holds what the GPU test says it holds, and
    the toggle state machine agrees with the standard csv module."""
    raw, ds, values, marks = C.build_quoted_buffer(total)
    assert len(raw) == total and ds % 64 != 0
    unit = C.quoted_unit(total - ds)
    assert unit > C.STEP and unit % C.STEP == 0
    pos, inq = C.ref_newlines(raw, ds)
    assert inq == 0
    rows = list(csv.reader(io.StringIO(raw[ds:].decode(), newline="")))
    assert len(rows) == len(pos) == len(values)
    assert [int(r[0]) for r in rows] == values.tolist()
    rel = lambda name: np.array(marks[name]) % unit
    got = set(pos.tolist())
    q = ord('"')
    for name in ("open63_close0", "open63_nl0", "escape_step"):
        assert set(rel(name).tolist()) == set(range(63, unit - 1, 64))
        for p in marks[name]:
            assert raw[ds + p] == q
    for p in marks["open63_close0"] + marks["escape_step"]:
        assert raw[ds + p + 1] == q
    for p in marks["open63_nl0"]:
        assert raw[ds + p + 1] == 10 and ds + p + 1 not in got
    for p in marks["escape_unit"]:
        assert p % unit == unit - 1 and raw[ds + p] == raw[ds + p + 1] == q
    for name, at, counted in (("quoted_nl_first", 0, False),
                              ("quoted_nl_last", unit - 1, False),
                              ("plain_nl_first", 0, True),
                              ("plain_nl_last", unit - 1, True)):
        assert marks[name]
        for p in marks[name]:
            assert p % unit == at and raw[ds + p] == 10
            assert (ds + p in got) == counted
    # a long run with no quote at all
    qpos = np.flatnonzero(np.frombuffer(raw, dtype=np.uint8) == q)
    assert np.diff(qpos).max() > 8 * 1024
