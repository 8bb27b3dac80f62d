"""CPU tests of the C-ABI library: it must build, load on a GPU-less host,
and export every symbol include/quokka_amd.h declares. No compute calls."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "quokka_amd", "libquokka_amd.so")
HDR = os.path.join(ROOT, "include", "quokka_amd.h")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(SO):
        subprocess.run(["make", "-C",
                        os.path.join(ROOT, "quokka_amd", "csrc")], check=True)
    assert os.path.exists(SO)


def header_symbols():
    syms = []
    with open(HDR) as f:
        for m in re.finditer(r"^\s*(?:int|const char \*)\s*(qk_\w+)\s*\(",
                             open(HDR).read(), re.M):
            syms.append(m.group(1))
    return syms


def test_header_declares_expected_surface():
    syms = header_symbols()
    assert len(syms) >= 30
    for must in ("qk_q1_agg", "qk_q6_agg", "qk_join_build", "qk_join_probe",
                 "qk_groupby_i64_sum", "qk_partition_hist", "qk_filter_i32",
                 "qk_gen_lineitem", "qk_block_threads", "qk_max_blocks",
                 "qk_str_dict_encode", "qk_str_dict_rehash",
                 "qk_str_hash_i64"):
        assert must in syms


def test_so_loads_and_exports_all_header_symbols():
    lib = ctypes.CDLL(SO)
    for sym in header_symbols():
        assert hasattr(lib, sym), "missing export: %s" % sym
    lib.qk_build_arch.restype = ctypes.c_char_p
    assert lib.qk_build_arch() == b"gfx950"


def header_prototypes():
    """name -> list of parameter texts, comments stripped"""
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"^\s*(?:int|const char \*)\s*(qk_\w+)\s*"
                         r"\(([^;]*)\)\s*;", text, re.M):
        params = [p.strip() for p in m.group(2).split(",")]
        protos[m.group(1)] = [] if params in ([""], ["void"]) else params
    return protos


def test_shim_signatures_match_header_prototypes():
    """ctypes checks nothing: an argument missing from a shim signature
    shifts every later one silently. Every signature the shim declares
    must have the header's parameter count, and the CSV and Parquet page
    entry points the header's exact parameter kinds."""
    import ctypes as ct
    from quokka_amd import shim
    protos = header_prototypes()
    both = set(shim._SIGS) & set(protos)    # int / const char * returns
    assert len(both) >= 90, len(both)
    for name in sorted(both):
        assert len(shim._SIGS[name]) == len(protos[name]), name

    def kind(param):
        if "*" in param:
            return ct.c_void_p
        return {"uint64_t": ct.c_uint64, "uint8_t": ct.c_uint8,
                "int": ct.c_int}[param.split()[0]]
    for name in ("qk_csv_newlines", "qk_csv_newlines_quoted",
                 "qk_csv_parse", "qk_pq_rle_pages", "qk_pq_def_pages",
                 "qk_str_hash_i64"):
        assert [kind(p) for p in protos[name]] == shim._SIGS[name], name
    # qk_pq_rle_pages ends with the per-page error table
    assert [p.split()[-1].lstrip("*") for p in protos["qk_pq_rle_pages"]] \
        == ["stream", "npages", "ents", "src_bytes", "out", "err_dev"]
    # qk_csv_parse: (first 8 bytes, length) prefilter arrays, then the
    # candidates' full bytes and offsets for the exact compare
    names = [p.split()[-1].lstrip("*") for p in protos["qk_csv_parse"]]
    assert names[-7:] == ["out_ptrs", "dict_cands", "dict_lens", "ncands",
                          "dict_bytes", "dict_offs", "err_row"]
    assert len(names) == 16


def test_shim_imports_and_fails_loudly_without_gpu():
    from quokka_amd import shim
    assert shim.build_arch() == "gfx950"
    if shim.device_count() == 0:
        with pytest.raises(shim.QkError):
            shim.init(0)


def test_date_constants_match_generator():
    """The kernel's hardcoded date constants (csrc) must equal the
    oracle generator's."""
    from oracle import tpch_gen as G
    src = open(os.path.join(ROOT, "quokka_amd", "csrc",
                            "quokka_amd.hip")).read()
    assert "#define QK_ORDERDATE_LO %d" % G.ORDERDATE_LO in src
    assert "#define QK_ORDERDATE_HI %d" % G.ORDERDATE_HI in src
    assert "#define QK_RECEIPT_CUTOFF %d" % G.RECEIPT_CUTOFF in src
    from quokka_amd import queries as DQ
    assert DQ.Q1_CUTOFF == G.Q1_CUTOFF
    assert DQ.Q3_DATE == G.Q3_DATE
    assert DQ.Q6_LO == G.Q5_LO and DQ.Q6_HI == G.Q5_HI


def test_splitmix64_twin():
    """oracle splitmix64 (kernel-parity reference) matches a known vector of
    the canonical splitmix64."""
    import numpy as np
    from oracle.executors import splitmix64
    # canonical splitmix64(seed=0) first output
    assert int(splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF


def test_executors_importable_and_picklable_without_so_state():
    import pickle
    from quokka_amd import GPUBuildProbeJoinExecutor, GPUAggExecutor
    j = GPUBuildProbeJoinExecutor(on="k", how="inner")
    a = GPUAggExecutor(["g"], [("g", "asc")], "sum(x) as sx")
    pickle.loads(pickle.dumps(j))
    pickle.loads(pickle.dumps(a))


def test_aggexec_sql_parsing():
    from quokka_amd import GPUAggExecutor
    a = GPUAggExecutor([], None,
                       "sum(e0_agg_0) as sq, sum(e3_agg_0) / sum(e3_agg_1) as avg_x")
    assert a.sum_cols == ["e0_agg_0", "e3_agg_0", "e3_agg_1"]
    assert a.exprs[0][0] == "sq"
    assert a.exprs[1][0] == "avg_x"
    import numpy as np
    s = {"e0_agg_0": np.array([2.0]), "e3_agg_0": np.array([10.0]),
         "e3_agg_1": np.array([4.0])}
    assert eval(a.exprs[1][1], {"s": s})[0] == 2.5


def test_topk_executor_cpu():
    """GPUTopKExecutor (ConcatThenSQLExecutor mirror) is pure host logic
    over tiny partials -> testable without a GPU."""
    import numpy as np
    import pyarrow as pa
    from quokka_amd import GPUTopKExecutor
    rng = np.random.default_rng(3)
    rev = rng.random(1000)
    date = rng.integers(0, 100, 1000)
    t = pa.table({"revenue": rev, "o_orderdate": date,
                  "k": np.arange(1000)})
    ex = GPUTopKExecutor(["revenue", "o_orderdate"], 10,
                         descending=[True, False])
    ex.execute([t.slice(0, 500)], 0, 0)
    ex.execute([t.slice(500)], 0, 0)
    out = ex.done(0)
    order = np.lexsort((date, -rev))[:10]
    assert out.column("k").to_pylist() == list(order)


def test_jit_translate_and_compile_cpu():
    """Predicate translation + hiprtc compilation work without a GPU
    (pure compiler); covers the reference's TPC-H filter_sql grammar."""
    import numpy as np
    from quokka_amd import jit

    schema = {"l_shipdate": np.dtype(np.int32),
              "l_discount": np.dtype(np.float64),
              "l_quantity": np.dtype(np.float64),
              "c_mktsegment": np.dtype(np.uint8)}

    e, cols = jit.translate(
        "l_shipdate >= date '1994-01-01' and l_shipdate < "
        "date '1994-01-01' + interval '1' year and l_discount between "
        "0.06 - 0.01 and 0.06 + 0.01 and l_quantity < 24", schema)
    assert cols == ["l_shipdate", "l_discount", "l_quantity"]
    assert "8766" in e and "9131" in e and "0.049999999999999996" in e

    e2, cols2 = jit.translate(
        "l_shipdate <= date '1998-12-01' - interval '90' day", schema)
    assert e2 == "(v0) <= (10471)" and cols2 == ["l_shipdate"]

    class SD:
        codes = {"BUILDING": 1}
    e3, cols3 = jit.translate("c_mktsegment = 'BUILDING'", schema,
                              {"c_mktsegment": SD()})
    assert e3 == "(v0) == (1)"

    e4, _ = jit.translate(
        "not (l_quantity < 5 or l_quantity > 45)", schema)
    assert e4.startswith("!(")

    f = jit.JitFilter("l_quantity < 24 and l_discount >= 0.05", schema)
    assert f.expr and f.prog
    import ctypes
    from quokka_amd import shim
    shim._lib.qk_jit_code_size.restype = ctypes.c_uint64
    assert shim._lib.qk_jit_code_size(f.prog) > 1000   # real code object
    f.free()

    import pytest as _pytest
    with _pytest.raises(ValueError):
        jit.translate("no_such_col < 5", schema)


def test_jit_aggregate_compiles_cpu():
    import numpy as np
    from quokka_amd import jit
    schema = {"d": np.dtype(np.int32), "x": np.dtype(np.float64),
              "g": np.dtype(np.uint8)}
    agg = jit.JitAggregate(schema, [("g", 4)],
                           ["sum(x) as sx", "count(*) as n"],
                           predicate="d < 100")
    assert agg.ngroups == 4 and agg.naggs == 2
    agg.free()
    import pytest as _p
    with _p.raises(Exception):
        jit.JitAggregate(schema, [("g", 200)], ["sum(x)"])  # >64 accums


def test_jit_filter_col_cap_clean_error():
    import numpy as np
    import pytest as _p
    from quokka_amd import jit, shim
    schema = {("c%d" % i): np.dtype(np.float64) for i in range(10)}
    pred = " and ".join("c%d > 0" % i for i in range(10))
    with _p.raises(shim.QkError, match="ncols"):
        jit.JitFilter(pred, schema)


def test_jit_translate_r02_tail_expressions():
    """The late-r02 query-tail expressions translate as written in
    queries.py (pure-Python translator, no GPU): the Q21 arithmetic
    MIN-select over mixed f64/i64 columns and the multi-bound f64
    qualification filter."""
    import numpy as np
    from quokka_amd import jit
    e, cols = jit.translate_arith(
        "f * sk + (1 - f) * 1000000000",
        {"f": np.dtype(np.float64), "sk": np.dtype(np.int64)})
    assert set(cols) == {"f", "sk"}
    # C expression references both columns and keeps the select shape
    assert "*" in e and "+" in e
    e2, cols2 = jit.translate(
        "ac > 1.5 and lc > 0.5 and lc < 1.5",
        {"ac": np.dtype(np.float64), "lc": np.dtype(np.float64)})
    assert set(cols2) == {"ac", "lc"}
    assert "&&" in e2
    # comparisons are rejected by the ARITH entry (JitMap contract)
    import pytest as _pytest
    with _pytest.raises(Exception):
        jit.translate_arith("a > 1", {"a": np.dtype(np.float64)})


def _topk_want(t, keys, desc, k):
    return t.sort_by([(c, "descending" if d else "ascending")
                      for c, d in zip(keys, desc)]).slice(0, k)


def test_topk_executor_descending_string_key_cpu():
    """A descending string sort key, alone and as the second of two keys
    (negating the key is a TypeError on strings): == sort_by + slice."""
    import numpy as np
    import pyarrow as pa
    from quokka_amd import GPUTopKExecutor
    rng = np.random.default_rng(5)
    pool = np.array(["", "a", "a\0", "ab", "abc", "b", "é",
                     "日本", "日本語", "z"], dtype=object)
    n = 400
    t = pa.table({"s": pa.array(rng.choice(pool, n)),
                  "g": rng.integers(0, 5, n),
                  "id": np.arange(n)})
    for keys, desc in ((["s", "id"], [True, False]),
                       (["g", "s", "id"], [False, True, False]),
                       (["g", "s", "id"], [True, True, True]),
                       (["s", "id"], [False, True])):
        ex = GPUTopKExecutor(keys, 37, descending=desc)
        ex.execute([t.slice(0, 150)], 0, 0)
        ex.execute([t.slice(150)], 0, 0)
        out = ex.done(0)
        assert out.column("id").to_pylist() == \
            _topk_want(t, keys, desc, 37).column("id").to_pylist(), (keys, desc)
    ex = GPUTopKExecutor(["s"], 5, descending=[True])
    ex.execute([t], 0, 0)
    assert ex.done(0).column("s").to_pylist() == \
        _topk_want(t, ["s"], [True], 5).column("s").to_pylist()


def test_topk_executor_descending_needs_no_arithmetic_cpu():
    """Descending keys whose negation wraps or is undefined: uint64 above
    2**63, INT64_MIN and bool order like any other; NaN stays last."""
    import numpy as np
    import pyarrow as pa
    from quokka_amd import GPUTopKExecutor
    u = np.array([2 ** 63 + 5, 1, 2 ** 64 - 1, 0, 7], dtype=np.uint64)
    i = np.array([-2 ** 63, 5, -1, 2 ** 63 - 1, 0], dtype=np.int64)
    b = np.array([True, False, True, False, False])
    f = np.array([1.5, np.nan, -2.0, 9.0, np.nan])
    t = pa.table({"u": u, "i": i, "b": b, "f": f, "id": np.arange(5)})
    for key, want in (("u", [2, 0, 4, 1, 3]), ("i", [3, 1, 4, 2, 0]),
                      ("b", [0, 2, 1, 3, 4]), ("f", [3, 0, 2, 1, 4])):
        ex = GPUTopKExecutor([key, "id"], 5, descending=[True, False])
        ex.execute([t], 0, 0)
        assert ex.done(0).column("id").to_pylist() == want, key
