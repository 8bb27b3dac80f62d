"""CPU tests of the LIKE matcher: qk_like_compile + qk_str_like_host_i64
(the __host__ __device__ matcher the kernel shares) against Python `re`
on the decoded strings, bit for bit; plus jit.translate on raw-string
(object dtype) schemas. No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _like_cases as L  # noqa: E402

from quokka_amd import shim  # noqa: E402

c_vp = ctypes.c_void_p


def host_like(pattern, strings, negate=False, exact=False):
    pat = shim.like_compile(pattern, exact)
    off, data = L.arrow_layout(strings, np.int64)
    data = np.ascontiguousarray(np.append(data, np.uint8(0)))  # never NULL
    out = np.full(len(strings), 7, dtype=np.uint8)
    shim.call("qk_str_like_host_i64", ctypes.c_uint64(len(strings)),
              off.ctypes.data_as(c_vp), data.ctypes.data_as(c_vp),
              ctypes.byref(pat), int(negate), out.ctypes.data_as(c_vp))
    return out


def arrow_like(pattern, strings):
    import pyarrow as pa
    import pyarrow.compute as pc
    return np.asarray(pc.match_like(pa.array(strings, pa.string()),
                                    pattern)).astype(np.uint8)


HAND = [
    ("", ["", "a"]),
    ("%", [""]),
    ("_%", ["", "a"]),
    ("a%a", ["a", "aa", "aba"]),
    ("%ab", ["abab", "aba"]),
    ("%aab%", ["aaab"]),
    ("%ab%ab%", ["abab", "aba"]),
    ("ab%", ["a"]),
    ("%%a%%", ["", "a", "ba", "bab", "bb"]),
    ("__", ["é", "éa"]),
    ("%_", ["é"]),
    ("a\\b", ["a\\b", "ab", "a\\\\b"]),
]


@pytest.mark.parametrize("pattern,strings", HAND,
                         ids=[repr(p) for p, _ in HAND])
def test_hand_cases(pattern, strings):
    for negate in (False, True):
        want = L.oracle(pattern, strings, negate)
        np.testing.assert_array_equal(
            host_like(pattern, strings, negate), want)
    if "\\" not in pattern:
        np.testing.assert_array_equal(arrow_like(pattern, strings),
                                      L.oracle(pattern, strings))


def test_hand_cases_expected_values():
    """The cases the oracle must get right for the above to mean anything."""
    assert list(host_like("a%a", ["a", "aa", "aba"])) == [0, 1, 1]
    assert list(host_like("__", ["é", "éa"])) == [0, 1]
    assert list(host_like("%_", ["é"])) == [1]
    assert list(host_like("%aab%", ["aaab"])) == [1]
    assert list(host_like("a\\b", ["a\\b"])) == [1]


def test_exact_is_all_literal():
    strings = ["50%_off", "50xyoff", "50%_of", "50%_offf", ""]
    got = host_like("50%_off", strings, exact=True)
    np.testing.assert_array_equal(got, L.oracle("50%_off", strings,
                                                exact=True))
    assert list(got) == [1, 0, 0, 0, 0]
    assert list(host_like("50%_off", strings[:2])) == [1, 1]
    assert list(host_like("", ["", "a"], exact=True)) == [1, 0]
    assert list(host_like("50%_off", strings[:2], negate=True,
                          exact=True)) == [0, 1]


def test_seeded_fuzz():
    pats, strs = L.fuzz_cases(300, 1500)
    assert len(pats) == 300 and len(strs) == 1500
    matched = 0
    for p in pats:
        want = L.oracle(p, strs)
        got = host_like(p, strs)
        assert np.array_equal(got, want), (
            p, [strs[i] for i in np.nonzero(got != want)[0][:5]])
        matched += int(want.sum())
    frac = matched / (len(pats) * len(strs))
    assert 0.05 < frac < 0.95, frac


def test_fuzz_agrees_with_arrow():
    pats, strs = L.fuzz_cases(40, 300, seed=L.FUZZ_SEED + 1)
    for p in pats:
        np.testing.assert_array_equal(arrow_like(p, strs),
                                      L.oracle(p, strs), err_msg=p)


def test_compile_bounds():
    with pytest.raises(ValueError, match="256"):
        shim.like_compile("a" * 257)
    with pytest.raises(ValueError, match="256"):
        shim.like_compile("a" * 257, exact=True)
    seg17 = "%".join(["a"] * 17)
    with pytest.raises(ValueError, match="segments"):
        shim.like_compile(seg17)
    # 16 segments, 256 bytes: 15 x 'aaaaaaaaaaaaaaa%' + a 16-byte segment
    big = ("a" * 15 + "%") * 15 + "b" * 16
    assert len(big) == 256
    pat = shim.like_compile(big)
    assert pat.nseg == 16 and pat.anchor_start == 1 and pat.anchor_end == 1
    s = "a" * 15 * 15 + "b" * 16
    # expected values by hand (a backtracking regex engine needs
    # exponential time to reject with 15 `.*` groups): the extra b is
    # absorbed by the last %, the x breaks the start anchor, 15 b's are one
    # short of the end segment
    strings = [s, s + "b", "x" + s, s[:-1]]
    assert list(host_like(big, strings)) == [1, 1, 0, 0]
    # the 17-segment pattern is legal as an exact literal (one segment)
    assert shim.like_compile(seg17, exact=True).nseg == 1
    # % runs collapse: they add no segments
    assert shim.like_compile("%%a%%").nseg == 1


def test_translate_raw_string_terms():
    from quokka_amd import jit
    schema = {"c": np.dtype(object), "q": np.dtype(np.float64)}
    expr, cols, terms = jit.translate_terms("c LIKE '%x%' and q < 5", schema)
    assert len(terms) == 1
    flag, col, pattern, exact = terms[0]
    assert (col, pattern, exact) == ("c", "%x%", False)
    assert cols == [flag, "q"] and "c" not in cols
    assert expr == "((v0) != 0) && ((v1) < (5))"
    # translate() keeps its two-value shape
    assert jit.translate("c LIKE '%x%' and q < 5", schema) == (expr, cols)

    expr2, cols2, terms2 = jit.translate_terms(
        "c like '%x%' or (q > 1 and c like '%x%')", schema)
    assert len(terms2) == 1 and cols2 == [terms2[0][0], "q"]
    assert expr2.count("(v0) != 0") == 2

    expr3, cols3, terms3 = jit.translate_terms(
        "c <> 'ab' and c not like '%b' and c = 'ab'", schema)
    assert [t[1:] for t in terms3] == [("c", "ab", True), ("c", "%b", False)]
    assert expr3 == "(((v0) == 0) && ((v1) == 0)) && ((v0) != 0)"

    with pytest.raises(ValueError, match="IN"):
        jit.translate("c IN ('a','b')", schema)
    with pytest.raises(ValueError):
        jit.translate("c NOT IN ('a','b')", schema)
    with pytest.raises(ValueError):
        jit.translate("c < 'a'", schema)


def test_translate_dict_coded_column_unchanged():
    from quokka_amd import jit

    class SD:
        codes = {"BUILDING": 1, "MACHINERY": 2, "AUTOMOBILE": 3}

    schema = {"seg": np.dtype(np.uint8), "c": np.dtype(object)}
    dicts = {"seg": SD()}
    e, cols, terms = jit.translate_terms("seg like '%I%'", schema, dicts)
    assert e == "(((v0) == (1)) || ((v0) == (2)) || ((v0) == (3)))"
    assert cols == ["seg"] and terms == []
    e2, cols2, terms2 = jit.translate_terms(
        "seg = 'BUILDING' and seg not like 'M%'", schema, dicts)
    assert e2 == "((v0) == (1)) && (!(((v0) == (2))))"
    assert cols2 == ["seg"] and terms2 == []


def test_jit_filter_with_string_term_compiles_cpu():
    """The flag column is a u8 kernel input: hiprtc compiles the fused
    filter without a GPU, and flag columns count against the column cap."""
    from quokka_amd import jit
    schema = {"c": np.dtype(object), "q": np.dtype(np.float64)}
    f = jit.JitFilter("c like '%ab%' and q < 0.5", schema)
    assert f.prog and [np.dtype(d) for d in f.dtypes] == [
        np.dtype(np.uint8), np.dtype(np.float64)]
    f.free()
    wide = {("c%d" % i): np.dtype(object) for i in range(9)}
    pred = " and ".join("c%d like 'a%%'" % i for i in range(9))
    with pytest.raises(shim.QkError, match="ncols"):
        jit.JitFilter(pred, wide)
