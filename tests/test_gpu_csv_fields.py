"""csv_gpu.read_csv held to its contract, "anything unparseable raises
QkCsvError with the failing row, never a silently different value", on
every accept / reject edge of tests/_csv_cases.py (whose expectations
come from float(), int(), datetime.date and np.datetime64, proven in
tests/test_csv_cases_cpu.py), plus the two loops small inputs never
reach: the grid-stride loop of the row parser and the per-step quote
parity carry of the quoted newline index."""
import csv
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _csv_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def one_column(fields):
    """all fields as one column plus a trailing separator"""
    return b"".join(f + b"|\n" for f in fields)


def read_one(raw, spec, n, **kw):
    from quokka_amd import csv_gpu
    cols = csv_gpu.read_csv(raw, [spec], **kw)
    try:
        (col,) = cols.values()
        assert col.n == n
        return col.to_numpy(n)
    finally:
        for c in cols.values():
            c.free()


def failing_row(raw, schema, **kw):
    """read_csv must raise QkCsvError; -> the row its message names"""
    from quokka_amd import csv_gpu
    with pytest.raises(csv_gpu.QkCsvError) as ei:
        cols = csv_gpu.read_csv(raw, schema, **kw)
        got = {k: c.to_numpy(c.n).tolist() for k, c in cols.items()}
        pytest.fail("accepted as %r" % (got,))
    m = re.search(r"row (\d+)", str(ei.value))
    assert m, str(ei.value)
    return int(m.group(1))


# ---- accept tables -----------------------------------------------------

def test_f64_accept_bit_exact(gpu):
    fields = C.F64_ACCEPT_FIXED + C.f64_random_fields()
    want = C.f64_bits([float(f.decode()) for f in fields])
    got = read_one(one_column(fields), ("v", "f64"), len(fields))
    bad = np.flatnonzero(got.view(np.uint64) != want)
    assert bad.size == 0, [(fields[i], got[i]) for i in bad[:5]]


def test_i64_accept(gpu):
    want = np.array([int(f.decode()) for f in C.I64_ACCEPT], dtype=np.int64)
    got = read_one(one_column(C.I64_ACCEPT), ("v", "i64"), len(want))
    assert got.tolist() == want.tolist()


def test_date_accept(gpu):
    days = C.date_accept_days()
    texts = C.date_texts(days)
    raw = "".join(np.char.add(texts, "|\n").tolist()).encode()
    got = read_one(raw, ("d", "date"), len(days))
    bad = np.flatnonzero(got != days)
    assert bad.size == 0, [(texts[i], int(got[i]), int(days[i]))
                           for i in bad[:5]]


def test_dict_accept(gpu):
    fields = [c.encode() for c in C.DICT_CANDS]
    got = read_one(one_column(fields), ("s", "dict", C.DICT_CANDS), 5)
    assert got.tolist() == [0, 1, 2, 3, 4]
    # an empty-string candidate is legal and the empty field maps to it
    got = read_one(b"A|\n|\nB|\n", ("s", "dict", ["A", "", "B"]), 3)
    assert got.tolist() == [0, 1, 2]
    # 255-byte candidate, next to one that shares its first 8 bytes
    cands = ["LONGNAME", C.DICT_LONG, "LONGNAMEab"]
    fields = [C.DICT_LONG.encode(), b"LONGNAME", b"LONGNAMEab"]
    got = read_one(one_column(fields), ("s", "dict", cands), 3)
    assert got.tolist() == [1, 0, 2]


def test_dict_candidates_sharing_the_key_are_told_apart(gpu):
    """CUSTOMER#1 / CUSTOMER#2 share (first 8 bytes, length): the full
    byte compare decides, in either candidate order."""
    from quokka_amd import csv_gpu
    fields = [b"CUSTOMER#2", b"CUSTOMER#10", b"CUSTOMER#1", b"CUSTOMER#2"]
    for cands in (C.DICT_TWINS, C.DICT_TWINS[::-1]):
        got = read_one(one_column(fields), ("s", "dict", cands), 4)
        assert [cands[i] for i in got] == [f.decode() for f in fields]
    # the same candidate twice has no one right code: refused up front
    with pytest.raises(csv_gpu.QkCsvError):
        csv_gpu.read_csv(b"A|\n", [("s", "dict", ["A", "B", "A"])])


# ---- reject tables: the bad field alone, as row 1 of 3 ------------------

GOOD = {"f64": b"1.5", "i64": b"7", "date": b"2001-02-03"}


def _id(f):
    return repr(f[:24] + (b"..." if len(f) > 24 else b""))[1:]


def check_rejected(field, spec, good):
    raw = good + b"|\n" + field + b"|\n" + good + b"|\n"
    assert failing_row(raw, [spec]) == 1


@pytest.mark.parametrize("field", [f for f, _ in C.F64_REJECT], ids=_id)
def test_f64_reject(gpu, field):
    check_rejected(field, ("v", "f64"), GOOD["f64"])


@pytest.mark.parametrize("field", [f for f, _ in C.I64_REJECT], ids=_id)
def test_i64_reject(gpu, field):
    check_rejected(field, ("v", "i64"), GOOD["i64"])


@pytest.mark.parametrize("field", C.DATE_REJECT, ids=_id)
def test_date_reject(gpu, field):
    check_rejected(field, ("v", "date"), GOOD["date"])


@pytest.mark.parametrize("field", C.DICT_REJECT, ids=_id)
def test_dict_reject(gpu, field):
    check_rejected(field, ("s", "dict", C.DICT_CANDS), b"BUILDING")


@pytest.mark.parametrize("field", C.DICT_LONG_REJECT, ids=_id)
def test_dict_long_reject(gpu, field):
    check_rejected(field, ("s", "dict", ["SHORT", C.DICT_LONG]), b"SHORT")


@pytest.mark.parametrize("field", C.DICT_TWINS_REJECT, ids=_id)
def test_dict_twins_reject(gpu, field):
    check_rejected(field, ("s", "dict", C.DICT_TWINS), b"CUSTOMER#1")


# ---- more rows than one pass of the grid --------------------------------

def test_lowest_failing_row_across_grid_stride_iterations(gpu):
    n = 600000
    assert gpu.MAX_BLOCKS * gpu.BLOCK_THREADS < 555555   # second iteration
    assert 300000 < gpu.MAX_BLOCKS * gpu.BLOCK_THREADS   # first iteration
    rows = np.arange(n).astype(str)
    rows[300000] = "3x"
    rows[555555] = "5x"
    raw = "".join(np.char.add(rows, "\n").tolist()).encode()
    assert failing_row(raw, [("v", "i64")]) == 300000
    rows[300000] = "300000"
    raw = "".join(np.char.add(rows, "\n").tolist()).encode()
    assert failing_row(raw, [("v", "i64")]) == 555555


def test_grid_stride_rows_equal_their_source(gpu):
    from quokka_amd import csv_gpu
    n = gpu.MAX_BLOCKS * gpu.BLOCK_THREADS + 257
    assert n == 524288 + 257
    rng = np.random.default_rng(C.SEED + 2)
    ints = rng.integers(-10**18 + 1, 10**18, n)
    cents = rng.integers(0, 10**13, n)
    neg = rng.integers(0, 2, n).astype(bool)
    days = rng.integers(C.DAY_LO, C.DAY_HI + 1, n)
    ftext = np.char.add(np.char.add(np.where(neg, "-", ""),
                                    (cents // 100).astype(str)),
                        np.char.add(".", np.char.zfill(
                            (cents % 100).astype(str), 2)))
    line = np.char.add(np.char.add(ints.astype(str), "|"),
                       np.char.add(ftext, "|"))
    line = np.char.add(line, np.char.add(C.date_texts(days), "|\n"))
    raw = "".join(line.tolist()).encode()
    want_f = np.array([float(t) for t in ftext.tolist()])
    cols = csv_gpu.read_csv(raw, [("i", "i64"), ("f", "f64"),
                                  ("d", "date")])
    try:
        assert cols["i"].n == n
        assert np.array_equal(cols["i"].to_numpy(n), ints)
        assert np.array_equal(cols["f"].to_numpy(n).view(np.uint64),
                              want_f.view(np.uint64))
        assert np.array_equal(cols["d"].to_numpy(n), days)
    finally:
        for c in cols.values():
            c.free()


# ---- row structure -----------------------------------------------------

def test_row_with_fewer_fields_than_the_schema(gpu):
    two = [("a", "i64"), ("b", "i64")]
    assert failing_row(b"1|2|\n3|\n5|6|\n", two) == 1
    assert failing_row(b"1|2|\n3\n5|6|\n", two) == 1
    # also when the missing column would take any bytes
    assert failing_row(b"1|x\n3\n5|y\n", [("a", "i64"), ("b", "skip")]) == 1
    assert failing_row(b"1|2\n\n5|6\n", two) == 1


def test_crlf_row_then_lf_row(gpu):
    from quokka_amd import csv_gpu
    cols = csv_gpu.read_csv(b"1|2.5\r\n3|4.5\n5|6.5|\r\n",
                            [("a", "i64"), ("b", "f64")])
    try:
        assert cols["a"].to_numpy(3).tolist() == [1, 3, 5]
        assert cols["b"].to_numpy(3).tolist() == [2.5, 4.5, 6.5]
    finally:
        for c in cols.values():
            c.free()


def test_lone_cr_inside_a_numeric_field(gpu):
    assert failing_row(b"1|\n2\r3|\n4|\n", [("a", "i64")]) == 1
    assert failing_row(b"1.5|\n2\r.5|\n4|\n", [("a", "f64")]) == 1
    assert failing_row(b"1|\n\r2|\n4|\n", [("a", "i64")]) == 1


def test_final_row_without_newline_is_parsed(gpu):
    assert read_one(b"1\n2\n3", ("a", "i64"), 3).tolist() == [1, 2, 3]
    assert read_one(b"1|\n2|\n3|", ("a", "i64"), 3).tolist() == [1, 2, 3]
    assert failing_row(b"1\n2\n3x", [("a", "i64")]) == 2


def test_exactly_one_trailing_separator(gpu):
    one = [("a", "i64")]
    assert read_one(b"1\n2|\n3\n", ("a", "i64"), 3).tolist() == [1, 2, 3]
    assert failing_row(b"1|\n2||\n3|\n", one) == 1
    assert failing_row(b"1|\n2|||\n3|\n", one) == 1
    # quoted last field
    assert read_one(b'"1",\n"2"\n', ("a", "i64"), 2,
                    sep=",").tolist() == [1, 2]
    assert failing_row(b'"1",\n"2",,\n', one, sep=",") == 1


def test_surplus_fields_are_an_error(gpu):
    """No in-tree caller passes a prefix schema, so a field beyond the
    schema is a mismatch to report, not bytes to drop."""
    one = [("a", "i64")]
    assert failing_row(b"1|\n2|9\n3|\n", one) == 1
    assert failing_row(b"1|\n2|9|\n3|\n", one) == 1
    assert failing_row(b"1|x|\n2|y|z\n", [("a", "i64"), ("b", "skip")]) == 1
    # named, they are fine
    from quokka_amd import csv_gpu
    cols = csv_gpu.read_csv(b"1|x|z\n2|y|\n",
                            [("a", "i64"), ("b", "skip"), ("c", "skip")])
    try:
        assert cols["a"].to_numpy(2).tolist() == [1, 2]
    finally:
        for c in cols.values():
            c.free()


# ---- quoting -----------------------------------------------------------

def test_bytes_after_a_closing_quote(gpu):
    two = [("a", "i64"), ("b", "i64")]
    assert failing_row(b'1,2\n"12"9,5\n3,4\n', two, sep=",") == 1
    assert failing_row(b'1,2\n"12" ,5\n3,4\n', two, sep=",") == 1
    assert failing_row(b'1,2\n3,"4"x\n5,6\n', two, sep=",") == 1
    # a quoted field that is still open at the end of its row (the quote
    # inside x"y keeps the buffer's quote count even)
    assert failing_row(b'1,2\nx"y,"3\n5,6\n',
                       [("a", "skip"), ("b", "i64")], sep=",") == 1


@pytest.mark.parametrize("raw", [
    b'1,2\n"3,4\n5,6\n7,8\n',             # never closed: would eat 3 rows
    b'1,2\n3,4\n5,"6\n',                  # in the last row
    b'1,"2"\n3,"4""\n5,"6"\n',            # "" leaves the field open
], ids=["early", "last_row", "escape_left_open"])
def test_odd_quote_count_raises(gpu, raw):
    from quokka_amd import csv_gpu
    assert raw.count(b'"') % 2 == 1
    with pytest.raises(csv_gpu.QkCsvError):
        cols = csv_gpu.read_csv(raw, [("a", "i64"), ("b", "skip")], sep=",")
        pytest.fail("returned %d rows" % cols["a"].n)


@pytest.mark.parametrize("total,unit_want", [((1 << 20) + 4097, 128),
                                             ((3 << 20) + 131, 256)])
def test_quoted_newline_index_at_scale(gpu, total, unit_want):
    """Units of more than one 64-byte step: the quote parity has to carry
    from step to step inside a wave's unit, with quotes in lane 63 / lane
    0, "" pairs across step and unit boundaries, and newlines - quoted
    and not - on the first and last byte of a unit."""
    from quokka_amd import csv_gpu
    from quokka_amd.shim import DevBuffer, DevColumn, c_u64, c_vp
    raw, ds, values, marks = C.build_quoted_buffer(total)
    n = len(raw)
    assert n == total and ds % 64 != 0
    # the header's formula, re-derived: a unit must span several steps
    span = n - ds
    unit = -(-span // 16384)
    unit = -(-unit // 64) * 64
    assert unit == unit_want == C.quoted_unit(span) and unit // 64 > 1
    q = ord('"')
    for name in ("open63_close0", "open63_nl0", "escape_step"):
        rel = {p % unit for p in marks[name]}
        assert rel == set(range(63, unit - 1, 64)), name
        assert all(raw[ds + p] == q for p in marks[name])
    assert all(raw[ds + p + 1] == q
               for p in marks["open63_close0"] + marks["escape_step"])
    assert all(p % unit == unit - 1 and raw[ds + p] == raw[ds + p + 1] == q
               for p in marks["escape_unit"])
    for name, at in (("quoted_nl_first", 0), ("quoted_nl_last", unit - 1),
                     ("plain_nl_first", 0), ("plain_nl_last", unit - 1)):
        assert marks[name] and all(
            p % unit == at and raw[ds + p] == 10 for p in marks[name]), name

    want, inq = C.ref_newlines(raw, ds)
    assert inq == 0
    nrows = len(list(csv.reader(io.StringIO(raw[ds:].decode(), newline=""))))
    assert nrows == len(want) == len(values)
    wantset = set(want.tolist())
    assert all(ds + p not in wantset for p in
               marks["quoted_nl_first"] + marks["quoted_nl_last"])
    assert all(ds + p in wantset for p in
               marks["plain_nl_first"] + marks["plain_nl_last"])

    arr = np.frombuffer(raw, dtype=np.uint8)
    dev = DevBuffer(n + 8)
    pos = DevColumn(np.uint64, span)
    cnt = DevBuffer(8)
    try:
        gpu._bounce.h2d(dev.ptr, arr)
        gpu.call("qk_dmemset", cnt.ptr, 0, c_u64(8))
        gpu.call("qk_dmemset", pos.ptr, 0xFF, c_u64(8 * span))
        gpu.call("qk_csv_newlines_quoted", None, c_u64(ds), c_u64(n),
                 dev.ptr, ctypes.c_uint8(q), pos.ptr, cnt.ptr)
        host_cnt = np.zeros(1, dtype=np.uint64)
        gpu.call("qk_d2h", host_cnt.ctypes.data_as(c_vp), cnt.ptr, c_u64(8))
        assert int(host_cnt[0]) == len(want)
        got = pos.to_numpy(len(want) + 1)
        assert np.array_equal(got[:-1], want)
        assert got[-1] == np.iinfo(np.uint64).max   # nothing past the count
    finally:
        for b in (dev, pos, cnt):
            b.free()

    cols = csv_gpu.read_csv(raw, [("v", "i64"), ("junk", "skip")], sep=",",
                            header=True)
    try:
        assert cols["v"].n == len(values)
        assert np.array_equal(cols["v"].to_numpy(len(values)), values)
    finally:
        for c in cols.values():
            c.free()
