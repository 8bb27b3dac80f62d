"""GPU tests of device LIKE over free-text string columns: the kernels
(both offset widths, both paths), ops.StringColumn / ops.like, the JIT
composition and gpu_partition_fn — all against Python `re` on the decoded
strings, flags equal bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _like_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = ["%special%requests%", "forest%", "%BRASS", "%", "", "_%_"]


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def host_like(shim, pattern, strings, negate=False, exact=False):
    pat = shim.like_compile(pattern, exact)
    off, data = L.arrow_layout(strings, np.int64)
    data = np.ascontiguousarray(np.append(data, np.uint8(0)))
    out = np.full(len(strings), 7, dtype=np.uint8)
    vp = ctypes.c_void_p
    shim.call("qk_str_like_host_i64", ctypes.c_uint64(len(strings)),
              off.ctypes.data_as(vp), data.ctypes.data_as(vp),
              ctypes.byref(pat), int(negate), out.ctypes.data_as(vp))
    return out


def dev_like(strings, pattern, negate=False, exact=False, large=False):
    from quokka_amd import ops
    arr = pa.array(strings, pa.large_string() if large else pa.string())
    sc = ops.StringColumn.from_arrow(arr)
    assert sc.offsets.dtype == (np.int64 if large else np.int32)
    flags = ops.like(sc, pattern, negate=negate, exact=exact)
    out = flags.to_numpy(len(strings))
    flags.free()
    sc.free()
    return out


@pytest.fixture(scope="module")
def mixed_rows():
    """1000 strings of 0-40 bytes with two whole waves of empty strings
    and every pattern's hit planted; prefixes of it are the row counts."""
    rng = np.random.default_rng(11)
    rows = L.comments(rng, 1000, 0, 40, plant=("special", "requests"),
                      frac=0.05)
    for i in range(64, 192):
        rows[i] = ""
    for i in (0, 5, 62, 200, 256, 999):
        rows[i] = "forest of " + rows[i][:20]
    for i in (3, 63, 64 + 130, 255, 257, 998):
        rows[i] = rows[i][:20] + " BRASS"
    want = {(p, neg): L.oracle(p, rows, neg)
            for p in PATTERNS for neg in (False, True)}
    return rows, want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_kernel_vs_host_vs_re(gpu, mixed_rows, n):
    rows, want = mixed_rows
    sub = rows[:n]
    for p in PATTERNS:
        for neg in (False, True):
            w = want[(p, neg)][:n]
            np.testing.assert_array_equal(host_like(gpu, p, sub, neg), w)
            for large in (False, True):
                got = dev_like(sub, p, negate=neg, large=large)
                np.testing.assert_array_equal(got, w, err_msg=repr(
                    (p, neg, large)))
    assert want[("%special%requests%", False)].sum() > 10
    assert want[("forest%", False)].sum() >= 6
    assert want[("%BRASS", False)].sum() >= 6
    np.testing.assert_array_equal(
        want[("%BRASS", False)],
        np.asarray(pc.match_like(pa.array(rows), "%BRASS")).astype(np.uint8))


def test_both_kernel_paths(gpu):
    """One string longer than the LDS tile in the middle of 300 rows sends
    its block down the direct-global path (the hit sits past the tile
    size); the same rows without it all run the LDS path."""
    tile = gpu.LIKE_TILE
    assert tile >= 4096
    rng = np.random.default_rng(12)
    rows = L.comments(rng, 300, 0, 40, plant=("special", "requests"),
                      frac=0.1)
    short = list(rows)
    rows[150] = "x" * (tile + 100) + "special y requests" + "z" * 50
    for p in ("%special%requests%", "%requests%", "x%z", "%BRASS"):
        for large in (False, True):
            np.testing.assert_array_equal(
                dev_like(rows, p, large=large), L.oracle(p, rows))
            np.testing.assert_array_equal(
                dev_like(short, p, large=large), L.oracle(p, short))
    assert L.oracle("%special%requests%", rows)[150] == 1


def test_forced_paths_equal_default(gpu, mixed_rows):
    """Either path forced for every pattern (qk_str_like picks one by the
    pattern's shape) gives the same flags, with a long string present."""
    from quokka_amd import ops
    from quokka_amd.shim import DevColumn, c_u64
    rows, _ = mixed_rows
    rows = list(rows)
    rows[500] = "y" * (gpu.LIKE_TILE + 7) + " special requests BRASS"
    for large in (False, True):
        sc = ops.StringColumn.from_arrow(
            pa.array(rows, pa.large_string() if large else pa.string()))
        fn = "qk_str_like_path_i64" if large else "qk_str_like_path_i32"
        for p in PATTERNS:
            pat = gpu.like_compile(p)
            want = L.oracle(p, rows)
            for stage in (0, 1):
                out = DevColumn(np.uint8, len(rows))
                gpu.call(fn, None, c_u64(len(rows)), sc.offsets.ptr,
                         sc.data.ptr, ctypes.byref(pat), 0, stage, out.ptr)
                np.testing.assert_array_equal(out.to_numpy(), want,
                                              err_msg=repr((p, stage)))
                out.free()
        sc.free()


def test_all_empty_column(gpu):
    rows = [""] * 200
    for large in (False, True):
        assert dev_like(rows, "%", large=large).tolist() == [1] * 200
        assert dev_like(rows, "_%", large=large).tolist() == [0] * 200
        assert dev_like(rows, "", exact=True, large=large).tolist() == \
            [1] * 200


def test_string_column_from_arrow(gpu):
    from quokka_amd import ops
    rng = np.random.default_rng(13)
    rows = L.comments(rng, 120, 0, 30)
    rows[40] = "héllo wörld"
    p = "%e%"

    def run(col, expect_rows):
        sc = ops.StringColumn.from_arrow(col)
        assert sc.n == len(expect_rows)
        f = ops.like(sc, p)
        got = f.to_numpy(sc.n)
        f.free()
        sc.free()
        np.testing.assert_array_equal(got, L.oracle(p, expect_rows))

    arr = pa.array(rows)
    run(arr.slice(7), rows[7:])
    run(arr.slice(7, 50), rows[7:57])
    run(pa.chunked_array([pa.array(rows[:45]), pa.array(rows[45:])]), rows)
    run(pa.array(rows, pa.large_string()).slice(7), rows[7:])
    run(arr.dictionary_encode(), rows)
    run(pa.chunked_array([], pa.string()), [])
    with pytest.raises(TypeError):
        ops.StringColumn.from_arrow(pa.array(["a", None, "b"]))
    with pytest.raises(TypeError):
        ops.StringColumn.from_arrow(pa.array([1, 2, 3]))


def test_gpu_seeded_fuzz(gpu):
    from quokka_amd import ops
    pats, strs = L.fuzz_cases(100, 1500)
    sc = ops.StringColumn.from_arrow(pa.array(strs))
    matched = 0
    for p in pats:
        want = L.oracle(p, strs)
        f = ops.like(sc, p)
        got = f.to_numpy(sc.n)
        f.free()
        assert np.array_equal(got, want), (
            p, [strs[i] for i in np.nonzero(got != want)[0][:5]])
        matched += int(want.sum())
    sc.free()
    assert 0.05 < matched / (100 * 1500) < 0.95


def test_jit_filter_composition(gpu):
    from quokka_amd import jit, ops
    from quokka_amd.shim import DevColumn
    n = 5000
    _, strs = L.fuzz_cases(0, n, seed=77)
    rng = np.random.default_rng(14)
    q = rng.random(n)
    d = rng.integers(0, 8, n).astype(np.int32)
    schema = {"c": np.dtype(object), "q": np.dtype(np.float64),
              "d": np.dtype(np.int32)}
    cols = {"c": ops.StringColumn.from_arrow(pa.array(strs)),
            "q": DevColumn.from_numpy(q), "d": DevColumn.from_numpy(d)}

    def m(p, exact=False):
        return L.oracle(p, strs, exact=exact).astype(bool)

    cases = [
        ("c like '%ab%' and q < 0.5", m("%ab%") & (q < 0.5)),
        ("not (c like 'a%' or d > 3)", ~(m("a%") | (d > 3))),
        ("c <> 'ab' and c not like '%b'", ~m("ab", True) & ~m("%b")),
    ]
    for pred, mask in cases:
        f = jit.JitFilter(pred, schema)
        idx, k = f.run(cols)
        got = idx.to_numpy(k)
        idx.free()
        f.free()
        want = np.nonzero(mask)[0]
        assert 0 < len(want) < n
        np.testing.assert_array_equal(got, want.astype(np.uint32))
    for c in cols.values():
        c.free()


@pytest.fixture(scope="module")
def orders():
    rng = np.random.default_rng(15)
    n = 4000
    comments = L.comments(rng, n, 19, 78, plant=("special", "requests"),
                          frac=0.02)
    keep = ~L.oracle("%special%requests%", comments).astype(bool)
    assert 20 < (~keep).sum() < 400
    t = pa.table({
        "o_orderkey": rng.permutation(n).astype(np.int64) + 1,
        "o_comment": pa.array(comments, pa.string()),
        "o_totalprice": rng.random(n) * 1e5,
        "o_flag": rng.integers(0, 4, n).astype(np.uint8)})
    return t, comments, keep


def test_gpu_partition_fn_like(gpu, orders):
    from quokka_amd.executors import gpu_partition_fn
    t, comments, keep = orders
    t3 = t.select(["o_orderkey", "o_comment", "o_totalprice"])
    out = gpu_partition_fn(
        t3, 0, 3, key="o_orderkey",
        predicate="o_comment not like '%special%requests%'")
    rows = []
    for ch, tab in out.items():
        assert tab.column_names == sorted(t3.column_names)
        ok = np.asarray(tab.column("o_orderkey"))
        assert np.all(ok % 3 == ch)
        rows += list(zip(ok.tolist(), tab.column("o_comment").to_pylist(),
                         np.asarray(tab.column("o_totalprice")).tolist()))
    want = [r for r, k in zip(zip(
        np.asarray(t.column("o_orderkey")).tolist(), comments,
        np.asarray(t.column("o_totalprice")).tolist()), keep) if k]
    assert sorted(rows) == sorted(want)


def test_gpu_partition_fn_like_batch_agg(gpu, orders):
    from quokka_amd.executors import gpu_partition_fn
    t, comments, keep = orders
    out = gpu_partition_fn(
        t, 0, 3, key="o_orderkey",
        predicate="o_comment not like '%special%requests%'",
        batch_agg=([("o_flag", 4)],
                   ["SUM(o_totalprice) as s", "COUNT(*) as n"]))
    flag = np.asarray(t.column("o_flag"))
    price = np.asarray(t.column("o_totalprice"))
    seen = {}
    for ch, tab in out.items():
        for g, s, c in zip(np.asarray(tab.column("o_flag")).tolist(),
                           np.asarray(tab.column("s")).tolist(),
                           np.asarray(tab.column("n")).tolist()):
            assert g % 3 == ch and g not in seen
            seen[g] = (s, c)
    assert sorted(seen) == [0, 1, 2, 3]
    for g in range(4):
        sel = keep & (flag == g)
        assert seen[g][1] == sel.sum()
        np.testing.assert_allclose(seen[g][0], price[sel].sum(), rtol=1e-9)


def test_q13_shaped(gpu):
    """customer LEFT JOIN (orders where o_comment not like ...) -> orders
    per customer -> distribution of the counts (apps/tpc-h/tpch.py:380)."""
    from quokka_amd import GPUBuildProbeJoinExecutor
    from quokka_amd.executors import gpu_partition_fn
    rng = np.random.default_rng(16)
    nc, no = 300, 3000
    comments = L.comments(rng, no, 19, 78, plant=("special", "requests"),
                          frac=0.05)
    custkey = rng.integers(1, 201, no).astype(np.int64)  # 100 without orders
    orders = pa.table({"o_orderkey": np.arange(1, no + 1, dtype=np.int64),
                       "o_custkey": custkey,
                       "o_comment": pa.array(comments)})
    customer = pa.table({"c_custkey": np.arange(1, nc + 1, dtype=np.int64)})
    parts = gpu_partition_fn(
        orders, 0, 1, key="o_custkey",
        predicate="o_comment not like '%special%requests%'",
        projection=["o_custkey", "o_orderkey"])
    ex = GPUBuildProbeJoinExecutor(left_on="c_custkey",
                                   right_on="o_custkey", how="left")
    ex.execute([parts[0]], 1, 0)
    joined = ex.execute([customer], 0, 0)
    ck = np.asarray(joined.column("c_custkey"))
    has = ~np.asarray(joined.column("o_orderkey").is_null())
    c_count = np.bincount(ck[has], minlength=nc + 1)[1:]
    got = np.bincount(c_count)

    keep = ~L.oracle("%special%requests%", comments).astype(bool)
    assert 50 < (~keep).sum() < 400
    w_count = np.bincount(custkey[keep], minlength=nc + 1)[1:]
    want = np.bincount(w_count)
    np.testing.assert_array_equal(got, want)
    assert want[0] >= 100
