"""Shared CSV field-parser test material: accept / reject tables per
column type, seeded generators and the quoted-newline buffer builder.
Host-only and deterministic, imports nothing from quokka_amd;
tests/test_csv_cases_cpu.py proves the tables against independent
parsers (float(), int(), datetime.date, np.datetime64) and
tests/test_gpu_csv_fields.py holds csv_gpu.read_csv to them.

A case is (field bytes, column type, expected): expected is the value an
independent parser gives, or REJECT. Reject cases carry a tag: None when
the independent parser refuses the text too, otherwise one of the
STRICTER_* reasons — text strtod / Python would read but the contract
next to the qk_csv_parse prototype (include/quokka_amd.h) refuses."""
import datetime

import numpy as np

REJECT = "REJECT"
SEED = 20240917
N_RANDOM = 20000

# header sentence: "f64 text with >15 significant digits or >18 decimals
# and i64 text with >18 digits are errors although strtod / strtoll can
# read them (the parse would no longer be exact)"
STRICTER_DIGITS = "stricter than strtod by contract: digit count"
# header sentence: "no exponent, inf, nan, hex or surrounding blanks"
STRICTER_SYNTAX = "stricter than strtod by contract: plain decimal only"
# Python's int() reads any Unicode decimal digit; the kernel reads ASCII
STRICTER_ASCII = "stricter than int() by contract: ASCII digits only"

F64_MAX_SIG = 15          # significant digits: first non-zero digit to end
F64_MAX_DEC = 18          # digits after the point
I64_MAX_DIGITS = 18


# ---- f64 ---------------------------------------------------------------
F64_ACCEPT_FIXED = [
    b"0", b"-0", b"+0", b"-0.0", b"5.", b".5", b"-.5", b"1.",
    b"999999999999999", b"0.999999999999999", b"999999999999.999",
    b"0.000000000000000001",            # k = 18
    b"0.000123456789012345",            # 15 significant digits, k = 18
    b"0000000000000000000000.5",        # leading zeros are not significant
    b"123456789.123456",
]

F64_REJECT = [
    (b"", None), (b"+", None), (b"-", None), (b".", None), (b"+.", None),
    (b"-.", None),
    (b"1e5", STRICTER_SYNTAX), (b"1E5", STRICTER_SYNTAX),
    (b"inf", STRICTER_SYNTAX), (b"nan", STRICTER_SYNTAX), (b"0x10", None),
    (b" 1", STRICTER_SYNTAX), (b"1 ", STRICTER_SYNTAX),
    (b"1..2", None), (b"1.2.3", None), (b"--1", None), (b"1-", None),
    (b"1,5", None),
    (b"1234567890123456", STRICTER_DIGITS),          # 16 significant
    (b"0.0000000000000000001", STRICTER_DIGITS),     # 19 decimals
]


def f64_random_fields(n=N_RANDOM, seed=SEED):
    """n decimal texts with 1-15 significant digits, 0 <= k <= 18
    decimals, random or no sign, random leading zeros; every one is
    inside the bit-exact range, so none may be rejected."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nd = int(rng.integers(1, F64_MAX_SIG + 1))
        k = int(rng.integers(0, F64_MAX_DEC + 1))
        digs = str(int(rng.integers(1, 10))) + "".join(
            str(int(d)) for d in rng.integers(0, 10, nd - 1))
        if k <= nd:
            whole, frac = digs[:nd - k], digs[nd - k:]
        else:
            whole, frac = "", "0" * (k - nd) + digs
        whole = "0" * int(rng.integers(0, 6)) + whole
        if frac:
            text = whole + "." + frac
        else:
            text = whole + ("." if rng.integers(0, 4) == 0 else "")
        text = ("", "+", "-")[int(rng.integers(0, 3))] + text
        out.append(text.encode())
    return out


def f64_digit_counts(field):
    """(significant digits, decimals) of a plain decimal text, counted
    from the text alone: significant = first non-zero digit to the last
    digit, point removed."""
    t = field.decode().lstrip("+-")
    whole, _, frac = t.partition(".")
    return len((whole + frac).lstrip("0")), len(frac)


def f64_bits(values):
    return np.array(values, dtype=np.float64).view(np.uint64)


# ---- i64 ---------------------------------------------------------------
I64_ACCEPT = [
    b"0", b"-0", b"+0", b"999999999999999999", b"-999999999999999999",
    b"+999999999999999999", b"000000000000000007",
]

I64_REJECT = [
    (b"", None), (b"-", None), (b"+", None), (b"1.0", None),
    (b"1 ", STRICTER_SYNTAX), (b"12a", None),
    (b"1000000000000000000", STRICTER_DIGITS),       # 19 digits
    (b"-9223372036854775808", STRICTER_DIGITS),
    ("\u0661\u0662\u0663".encode(), STRICTER_ASCII),  # Arabic-Indic 123
]


# ---- date --------------------------------------------------------------
DATE_YEARS = (1, 1600, 1899, 1900, 1901, 1969, 1970, 1972, 2000, 2023,
              2024, 2100, 2400, 9999)
EPOCH = np.datetime64("1970-01-01")
DAY_LO = int((np.datetime64("0001-01-01") - EPOCH).astype(np.int64))
DAY_HI = int((np.datetime64("9999-12-31") - EPOCH).astype(np.int64))


def date_accept_days(n=N_RANDOM, seed=SEED):
    """-> int64 days since 1970-01-01: every day of DATE_YEARS, then n
    seeded random days of [0001-01-01, 9999-12-31]."""
    parts = []
    for y in DATE_YEARS:
        lo = np.datetime64("%04d-01-01" % y)
        hi = np.datetime64("%04d-12-31" % y)
        parts.append(np.arange((lo - EPOCH).astype(np.int64),
                               (hi - EPOCH).astype(np.int64) + 1))
    rng = np.random.default_rng(seed + 1)
    parts.append(rng.integers(DAY_LO, DAY_HI + 1, n))
    return np.concatenate(parts).astype(np.int64)


def date_texts(days):
    """days since epoch -> array of 'YYYY-MM-DD' str (numpy's printer)."""
    return np.asarray(days).astype("datetime64[D]").astype(str)


DATE_REJECT = [
    b"2023-00-10", b"2023-13-10", b"2023-05-00", b"2023-05-32",
    b"2023-02-29", b"1900-02-29", b"2100-02-29", b"2023-02-30",
    b"2023-04-31", b"2023-06-31", b"2023-09-31", b"2023-11-31",
    b"2023-1-01", b"2023/01/01", b"20230101", b"2023-01-01 ",
    b"2023-01-0a", b"",
]


def ref_date(field):
    """Independent strict parse: the fixed 'YYYY-MM-DD' shape by hand, the
    calendar by datetime.date. -> days since epoch, or ValueError."""
    t = field.decode()
    if (len(t) != 10 or t[4] != "-" or t[7] != "-" or
            not (t[:4] + t[5:7] + t[8:]).isascii() or
            not (t[:4] + t[5:7] + t[8:]).isdigit()):
        raise ValueError(t)
    d = datetime.date(int(t[:4]), int(t[5:7]), int(t[8:]))
    return d.toordinal() - datetime.date(1970, 1, 1).toordinal()


# ---- dict --------------------------------------------------------------
DICT_CANDS = ["BUILDING", "AUTOMOBILE", "MACHINERY", "HOUSEHOLD",
              "FURNITURE"]
DICT_REJECT = [
    b"AUTOMOBILX", b"MACHINERZ",        # tail differs after byte 8
    b"AUTOMOBIL",                       # prefix of a candidate
    b"AUTOMOBILES",                     # candidate plus one byte
    b"building",                        # lower case
    b"",
]
# one 255-byte candidate: a field matching its first 8 bytes but longer
# (all lengths > 255 clamp to 255), or equal in length and differing at
# byte 200, is not that candidate
DICT_LONG = "LONGNAME" + "".join(chr(97 + i % 26) for i in range(247))
DICT_LONG_REJECT = [
    (DICT_LONG + "q" * 45).encode(),
    (DICT_LONG[:200] + "#" + DICT_LONG[201:]).encode(),
]
assert len(DICT_LONG) == 255 and len(DICT_LONG_REJECT[0]) == 300
assert len(DICT_LONG_REJECT[1]) == 255
# candidates that share (first 8 bytes, length): told apart by the tail
DICT_TWINS = ["CUSTOMER#1", "CUSTOMER#2", "CUSTOMER#10"]
DICT_TWINS_REJECT = [b"CUSTOMER#3", b"CUSTOMER#", b"CUSTOMER#11"]


def all_cases():
    """Every table as (field bytes, column type, expected or REJECT);
    dict cases use DICT_CANDS."""
    for f in F64_ACCEPT_FIXED + f64_random_fields():
        yield f, "f64", float(f.decode())
    for f, _ in F64_REJECT:
        yield f, "f64", REJECT
    for f in I64_ACCEPT:
        yield f, "i64", int(f.decode())
    for f, _ in I64_REJECT:
        yield f, "i64", REJECT
    days = date_accept_days()
    for t, d in zip(date_texts(days), days):
        yield t.encode(), "date", int(d)
    for f in DATE_REJECT:
        yield f, "date", REJECT
    for i, c in enumerate(DICT_CANDS):
        yield c.encode(), "dict", i
    for f in DICT_REJECT:
        yield f, "dict", REJECT


# ---- quoted newline index ----------------------------------------------
MAX_UNITS = 16384        # qk_csv_newlines_quoted: waves per launch
STEP = 64                # bytes one wave reads per step


def quoted_unit(span):
    """The header's formula: bytes per wave, rounded up to whole steps."""
    unit = -(-span // MAX_UNITS)
    return max(STEP, -(-unit // STEP) * STEP)


def ref_newlines(raw, data_start, quote=34):
    """Toggle on quote, record a newline when the state is even. Walks
    only the quote and newline bytes. -> (positions, final state)."""
    a = np.frombuffer(raw, dtype=np.uint8)
    ev = np.flatnonzero((a == quote) | (a == 10))
    ev = ev[ev >= data_start]
    inq, pos = 0, []
    for p in ev.tolist():
        if raw[p] == quote:
            inq ^= 1
        elif not inq:
            pos.append(p)
    return np.array(pos, dtype=np.uint64), inq


def build_quoted_buffer(total_len, header=b"col\n", seed=SEED):
    """-> (raw, data_start, values, marks). raw is exactly total_len
    bytes: the header, then rows '<int>,<junk>\\n' whose junk field is
    plain text or a quoted field. The quoted rows are laid out so that
    chosen bytes land on chosen offsets (relative to data_start) modulo
    the unit; marks[name] lists those offsets, for the test to check
    against the unit it re-derives. Between the constructs run ~12 KB of
    quote-free rows."""
    data_start = len(header)
    span = total_len - data_start
    unit = quoted_unit(span)
    rng = np.random.default_rng(seed)
    buf = bytearray()
    values = []
    marks = {}

    def row(junk):
        v = int(rng.integers(-10**9, 10**9))
        values.append(v)
        return b"%d," % v + junk + b"\n"

    def pad_to(target):
        """plain rows until len(buf) == target exactly"""
        assert target - len(buf) >= 32
        while target - len(buf) > 200:
            buf.extend(row(b"x" * int(rng.integers(20, 80))))
        gap = target - len(buf)
        v = int(rng.integers(0, 1000))
        values.append(v)
        head = b"%d," % v
        buf.extend(head + b"y" * (gap - len(head) - 1) + b"\n")
        assert len(buf) == target

    def place(name, junk, key, mod, newline_key=False):
        """emit a row so that junk[key] (or the row's own newline) sits at
        an offset == mod (modulo unit)"""
        v = int(rng.integers(0, 10**6))
        head = b"%d," % v
        k = len(head) + (len(junk) if newline_key else key)
        start = len(buf) + 64
        start += (mod - (start + k)) % unit
        pad_to(start)
        values.append(v)
        buf.extend(head + junk + b"\n")
        marks.setdefault(name, []).append(start + k)

    bounds = list(range(STEP, unit, STEP))    # step boundaries in a unit
    while len(buf) + 16 * 1024 + 8 * unit * (len(bounds) + 6) < span:
        for b0 in bounds:
            # opening quote in lane 63, closing quote in lane 0
            place("open63_close0", b'""', 0, b0 - 1)
            # ... and with a quoted newline right behind the opener
            place("open63_nl0", b'"\nz"', 0, b0 - 1)
            # "" escape across a step boundary, quoted newline after it
            place("escape_step", b'"ab""c\nd"', 3, b0 - 1)
        place("escape_unit", b'"ab""c\nd"', 3, unit - 1)
        place("quoted_nl_first", b'"p\nq"', 2, 0)
        place("quoted_nl_last", b'"p\nq"', 2, unit - 1)
        place("plain_nl_first", b"pq", 0, 0, newline_key=True)
        place("plain_nl_last", b"pq", 0, unit - 1, newline_key=True)
        pad_to(len(buf) + 12 * 1024)          # long run with no quote
    pad_to(span)
    raw = header + bytes(buf)
    assert len(raw) == total_len
    return raw, data_start, np.array(values, dtype=np.int64), marks
