"""GPU parity for group-by and distinct over any number of full-width key
columns: the device key dictionary (qk_keydict_encode: K 64-bit words per
row -> dense u32 code, all K words verified, no reserved key value), the
dense accumulate over its codes (qk_groupby_dense_acc), and the executor
paths built on them — GPUAggExecutor(device_keys=True) in place of
SQLAggExecutor's arbitrary groupby_keys list (sql_executors.py:556-599)
and GPUDistinctExecutor over a key list, the reference's
unique(subset=keys) (:517-554). Oracle: pyarrow's Table.group_by (Acero)
on the same inputs; keys exact, SUM at rtol 1e-9, MIN/MAX at rtol 0."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _check_against_acero(got, table, keys, aggs):
    """aggs: list of (column, 'sum'|'min'|'max', alias in `got`)."""
    want = table.group_by(keys, use_threads=False).aggregate(
        [(c, fn) for c, fn, _ in aggs])
    order = [(k, "ascending") for k in keys]
    g, w = got.sort_by(order), want.sort_by(order)
    assert g.num_rows == w.num_rows
    for k in keys:
        gk, wk = g.column(k).combine_chunks(), w.column(k).combine_chunks()
        assert gk.type == wk.type, (k, gk.type, wk.type)
        assert gk.equals(wk), k
    for c, fn, alias in aggs:
        np.testing.assert_allclose(
            np.asarray(g.column(alias)), np.asarray(w.column("%s_%s" % (c, fn))),
            rtol=1e-9 if fn == "sum" else 0, atol=0, err_msg=alias)


def _mixed_table(rng, n, nkeys):
    """nkeys of: int32, int64 (wide values), date32, string, float64, a
    second string, a second int64."""
    pool = np.array(["seg-%03d" % i for i in range(40)], dtype=object)
    pool2 = np.array(["p%d" % (i * i) for i in range(7)], dtype=object)
    cols = {
        "k_i32": pa.array(rng.integers(-5, 20, n).astype(np.int32)),
        "k_i64": pa.array((rng.integers(0, 30, n).astype(np.int64) - 15)
                          * (1 << 40)),
        "k_d32": pa.array(rng.integers(8035, 8045, n).astype(np.int32)
                          ).cast(pa.date32()),
        "k_str": pa.array(pool[rng.integers(0, len(pool), n)]),
        "k_f64": pa.array(rng.integers(0, 4, n) * 0.25 + 100.5),
        "k_str2": pa.array(pool2[rng.integers(0, len(pool2), n)]),
        "k_i64b": pa.array(rng.integers(0, 3, n).astype(np.int64)
                           + (1 << 62)),
    }
    keys = list(cols)[:nkeys]
    t = {k: cols[k] for k in keys}
    t["v"] = pa.array(rng.random(n))
    t["w"] = pa.array(rng.standard_normal(n))
    t["x"] = pa.array(rng.standard_normal(n))
    return pa.table(t), keys


@pytest.mark.parametrize("nkeys", [4, 7])
def test_many_mixed_keys_three_batches(gpu, nkeys):
    """4 and 7 mixed-type keys over 50k rows in three execute calls, SUM,
    MIN and MAX together. Without device_keys the executor refuses more
    than 3 keys."""
    from quokka_amd.executors import GPUAggExecutor
    rng = np.random.default_rng(100 + nkeys)
    t, keys = _mixed_table(rng, 50_000, nkeys)
    ex = GPUAggExecutor(keys, None,
                        "sum(v) as sv, min(w) as mn, max(x) as mx",
                        device_keys=True)
    for lo, hi in ((0, 20_000), (20_000, 20_001), (20_001, 50_000)):
        ex.execute([t.slice(lo, hi - lo)], 0, 0)
    out = ex.done(0)
    _check_against_acero(out, t, keys, [("v", "sum", "sv"),
                                        ("w", "min", "mn"),
                                        ("x", "max", "mx")])


@pytest.mark.parametrize("nkeys", [1, 16])
def test_one_and_sixteen_keys(gpu, nkeys):
    from quokka_amd.executors import GPUAggExecutor
    rng = np.random.default_rng(7 + nkeys)
    n = 5000
    keys = ["k%02d" % i for i in range(nkeys)]
    t = {k: pa.array(rng.integers(-2, 2 if nkeys > 1 else 300, n)
                     .astype(np.int64)) for k in keys}
    t["v"] = pa.array(rng.random(n))
    t = pa.table(t)
    ex = GPUAggExecutor(keys, [(keys[-1], "desc"), (keys[0], "asc")],
                        "sum(v) as sv", device_keys=True)
    ex.execute([t], 0, 0)
    out = ex.done(0)
    _check_against_acero(out, t, keys, [("v", "sum", "sv")])
    last = np.asarray(out.column(keys[-1]))
    assert np.all(np.diff(last) <= 0), "order-by desc on the last key"


def test_high_cardinality_key_column(gpu):
    """One of two key columns holds 2**21 + 5 distinct values, one or two
    rows per group: past the 21-bit field of the host codebook path."""
    from quokka_amd.executors import GPUAggExecutor
    nd = (1 << 21) + 5
    rng = np.random.default_rng(21)
    a = np.concatenate([np.arange(nd, dtype=np.int64),
                        np.arange(0, nd, 8, dtype=np.int64)])
    a = a * 1_000_003 - (1 << 40)
    perm = rng.permutation(len(a))
    a = a[perm]
    b = (a % 3).astype(np.int32)
    t = pa.table({"a": a, "b": b, "v": rng.random(len(a))})
    ex = GPUAggExecutor(["a", "b"], None, "sum(v) as sv", device_keys=True)
    half = len(a) // 2
    ex.execute([t.slice(0, half)], 0, 0)
    ex.execute([t.slice(half)], 0, 0)
    out = ex.done(0)
    assert out.num_rows == nd
    _check_against_acero(out, t, ["a", "b"], [("v", "sum", "sv")])


def test_former_sentinel_values_in_every_position(gpu):
    """INT64_MIN, -1, 0 and INT64_MAX are ordinary keys in every column:
    all 64 triples over them, so groups that differ only in the first
    column, only in the last, and (a, b, .) against (b, a, .)."""
    from quokka_amd.executors import GPUAggExecutor
    vals = np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64)
    g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1
                 ).reshape(-1, 3)
    rng = np.random.default_rng(64)
    rows = g[rng.permutation(np.repeat(np.arange(64), 5))]
    t = pa.table({"a": rows[:, 0], "b": rows[:, 1], "c": rows[:, 2],
                  "v": rng.random(len(rows)),
                  "w": rng.standard_normal(len(rows)),
                  "x": rng.standard_normal(len(rows))})
    ex = GPUAggExecutor(["a", "b", "c"], None,
                        "sum(v) as sv, min(w) as mn, max(x) as mx",
                        device_keys=True)
    ex.execute([t.slice(0, 100)], 0, 0)
    ex.execute([t.slice(100)], 0, 0)
    out = ex.done(0)
    assert out.num_rows == 64
    got = set(zip(*(out.column(k).to_pylist() for k in "abc")))
    assert got == set(map(tuple, g.tolist()))
    assert (int(I64_MIN), -1, 0) in got and (-1, int(I64_MIN), 0) in got
    _check_against_acero(out, t, ["a", "b", "c"],
                         [("v", "sum", "sv"), ("w", "min", "mn"),
                          ("x", "max", "mx")])


def _group_by_keys_vs_acero(ka, kb, v, expected_groups=1024):
    """ops.GroupByKeys over two int64 key columns, SUM/MIN/MAX of v, one
    update; compared with Acero."""
    from quokka_amd import ops, shim
    gb = ops.GroupByKeys(2, 3, agg_ops=[0, 1, 2],
                         expected_groups=expected_groups)
    kc = [shim.DevColumn.from_numpy(ka), shim.DevColumn.from_numpy(kb)]
    vc = shim.DevColumn.from_numpy(v)
    gb.update(kc, [vc, vc, vc])
    keys, sums = gb.extract()
    assert gb.n_groups == len(keys[0]) == sums.shape[1]
    for c in kc + [vc]:
        c.free()
    gb.free()
    got = pa.table({"a": keys[0], "b": keys[1], "s": sums[0], "mn": sums[1],
                    "mx": sums[2]})
    t = pa.table({"a": ka, "b": kb, "v": v})
    _check_against_acero(got, t, ["a", "b"], [("v", "sum", "s"),
                                              ("v", "min", "mn"),
                                              ("v", "max", "mx")])
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_edge_row_counts(gpu, n):
    rng = np.random.default_rng(n)
    ka = rng.integers(-3, 3, n).astype(np.int64)
    kb = rng.integers(0, 2, n).astype(np.int64) * I64_MAX
    _group_by_keys_vs_acero(ka, kb, rng.standard_normal(n))


def test_one_group_over_200k_rows(gpu):
    """One slot and one record take every atomic."""
    n = 200_000
    rng = np.random.default_rng(200)
    got = _group_by_keys_vs_acero(np.full(n, -1, dtype=np.int64),
                                  np.full(n, I64_MIN, dtype=np.int64),
                                  rng.standard_normal(n))
    assert got.num_rows == 1


def test_all_distinct_200k_rows(gpu):
    n = 200_000
    rng = np.random.default_rng(201)
    ka = rng.permutation(n).astype(np.int64) - n // 2
    got = _group_by_keys_vs_acero(ka, ka[::-1].copy(),
                                  rng.standard_normal(n), expected_groups=1)
    assert got.num_rows == n


def _new_tuples(rng, n, tag):
    """n distinct (a, b) pairs no other tag shares."""
    a = rng.permutation(n).astype(np.int64) * 7919 - 1000
    b = np.full(n, tag, dtype=np.int64) << 33
    return a, b


def test_key_dict_growth_keeps_codes(gpu):
    """Smallest capacity, then 8, 100 and 50k new tuples: every growth
    re-seats the slots and copies the store, and a code returned before a
    growth decodes to the same tuple after it."""
    from quokka_amd import ops, shim
    rng = np.random.default_rng(8)
    kd = ops.DeviceKeyDict(2, expected=1)
    seen = []           # (a, b, codes) per batch
    total = 0
    for tag, n_new in enumerate((8, 100, 50_000)):
        a, b = _new_tuples(rng, n_new, tag)
        # the batch repeats its own tuples and replays every earlier one
        a = np.concatenate([a, a] + [s[0] for s in seen])
        b = np.concatenate([b, b] + [s[1] for s in seen])
        cols = [shim.DevColumn.from_numpy(a), shim.DevColumn.from_numpy(b)]
        dcodes = kd.encode(cols, len(a))
        codes = dcodes.to_numpy(len(a))
        for c in cols + [dcodes]:
            c.free()
        assert kd.n_codes == total + n_new
        fresh = codes[:n_new]
        assert np.array_equal(np.sort(fresh),
                              np.arange(total, total + n_new)), "dense codes"
        assert np.array_equal(codes[n_new:2 * n_new], fresh)
        off = 2 * n_new
        for sa, sb, sc in seen:     # earlier tuples keep their codes
            assert np.array_equal(codes[off:off + len(sc)], sc)
            off += len(sc)
        seen.append((a[:n_new], b[:n_new], fresh))
        total += n_new
    ka, kb = kd.keys_host()
    assert len(ka) == len(kb) == total
    for sa, sb, sc in seen:
        assert np.array_equal(ka[sc], sa) and np.array_equal(kb[sc], sb)
    kd.free()


def test_sums_survive_growth(gpu):
    """GroupByKeys from the smallest capacity: sums, minima and maxima
    accumulated before each growth are still there after it."""
    from quokka_amd import ops, shim
    rng = np.random.default_rng(9)
    gb = ops.GroupByKeys(2, 3, agg_ops=[0, 1, 2], expected_groups=1)
    all_a, all_b, all_v = [], [], []
    for tag, n_new in enumerate((8, 100, 50_000)):
        a, b = _new_tuples(rng, n_new, tag)
        a = np.concatenate([a] + all_a)     # earlier groups get more rows
        b = np.concatenate([b] + all_b)
        v = rng.standard_normal(len(a))
        cols = [shim.DevColumn.from_numpy(x) for x in (a, b, v)]
        gb.update(cols[:2], [cols[2]] * 3)
        for c in cols:
            c.free()
        all_a.append(a), all_b.append(b), all_v.append(v)
    keys, sums = gb.extract()
    gb.free()
    assert len(keys[0]) == 8 + 100 + 50_000
    got = pa.table({"a": keys[0], "b": keys[1], "s": sums[0], "mn": sums[1],
                    "mx": sums[2]})
    t = pa.table({"a": np.concatenate(all_a), "b": np.concatenate(all_b),
                  "v": np.concatenate(all_v)})
    _check_against_acero(got, t, ["a", "b"], [("v", "sum", "s"),
                                              ("v", "min", "mn"),
                                              ("v", "max", "mx")])


def test_float_keys_zero_and_nan(gpu):
    """-0.0 and +0.0 are one group, returned as +0.0; NaNs of different
    payloads are one group. Expectation written here (Acero is only asked
    about inputs without -0.0 and NaN, below)."""
    from quokka_amd.executors import GPUAggExecutor
    nan_a = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    nan_b = np.array([0x7FF8000000000abc], dtype=np.uint64).view(np.float64)[0]
    f = np.array([0.0, -0.0, nan_a, nan_b, 1.5, -0.0, nan_b, 1.5, -1.5])
    k = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    v = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0])
    ex = GPUAggExecutor(["f", "k"], None, "sum(v) as sv", device_keys=True)
    ex.execute([pa.table({"f": f[:3], "k": k[:3], "v": v[:3]})], 0, 0)
    ex.execute([pa.table({"f": f[3:], "k": k[3:], "v": v[3:]})], 0, 0)
    out = ex.done(0)
    assert out.column("f").type == pa.float64()
    got = {}
    for fv, kv, sv in zip(out.column("f").to_pylist(),
                          out.column("k").to_pylist(),
                          out.column("sv").to_pylist()):
        if fv == 0:
            assert not np.signbit(fv), "zero group comes back as +0.0"
        got[("nan" if fv != fv else fv, kv)] = sv
    assert got == {(0.0, 1): 3.0, ("nan", 1): 12.0, (1.5, 1): 16.0,
                   (0.0, 2): 32.0, ("nan", 2): 64.0, (1.5, 2): 128.0,
                   (-1.5, 2): 256.0}


def test_float32_and_float64_keys_vs_acero(gpu):
    from quokka_amd.executors import GPUAggExecutor
    rng = np.random.default_rng(32)
    n = 20_000
    f32 = (rng.integers(1, 50, n) / 7).astype(np.float32)
    f64 = rng.integers(-20, 20, n) * 0.1 + 0.05      # never 0, never NaN
    t = pa.table({"f32": f32, "f64": f64, "v": rng.random(n),
                  "x": rng.standard_normal(n)})
    ex = GPUAggExecutor(["f32", "f64"], None, "sum(v) as sv, max(x) as mx",
                        device_keys=True)
    ex.execute([t], 0, 0)
    out = ex.done(0)
    assert out.column("f32").type == pa.float32()
    _check_against_acero(out, t, ["f32", "f64"], [("v", "sum", "sv"),
                                                  ("x", "max", "mx")])


def test_distinct_on_two_keys(gpu):
    """Three overlapping batches: exactly the first-seen (a, b) pairs come
    out, each once, rows sharing a but not b kept."""
    from quokka_amd.executors import GPUDistinctExecutor
    rng = np.random.default_rng(17)
    ex = GPUDistinctExecutor(["a", "b"])
    seen, emitted = set(), []
    for lo in (0, 300, 600):
        n = 4000
        a = rng.integers(lo, lo + 700, n).astype(np.int64)
        b = np.array(["b%d" % i for i in rng.integers(0, 3, n)], dtype=object)
        t = pa.table({"a": a, "b": pa.array(b), "row": np.arange(n) + lo * 100})
        out = ex.execute([t], 0, 0)
        want_rows = []
        for i, pair in enumerate(zip(a.tolist(), b.tolist())):
            if pair not in seen:
                seen.add(pair)
                want_rows.append(i + lo * 100)
        assert out.column("row").to_pylist() == want_rows
        emitted += list(zip(out.column("a").to_pylist(),
                            out.column("b").to_pylist()))
    assert len(emitted) == len(set(emitted)) == len(seen)
    assert set(emitted) == seen
    by_a = {}
    for a, b in emitted:
        by_a.setdefault(a, set()).add(b)
    assert max(len(s) for s in by_a.values()) == 3
    # a batch of pairs all seen before emits nothing
    assert ex.execute([pa.table({"a": np.array([emitted[0][0]]),
                                 "b": pa.array([emitted[0][1]]),
                                 "row": np.array([0])})], 0, 0) is None
    assert ex.done(0) is None


def test_default_path_unchanged(gpu):
    """Without the keyword the composite path answers as before; with it
    the device key dictionary gives the same table (input of
    test_string_plus_int_composite_groupby)."""
    from quokka_amd.executors import GPUAggExecutor
    rng = np.random.default_rng(36)
    n = 50_000
    pool = np.array(["s%0*d" % (int(rng.integers(1, 24)), i)
                     for i in range(800)], dtype=object)
    ks = pool[rng.integers(0, 800, n)]
    ki = rng.integers(0, 50, n).astype(np.int64)
    v = rng.random(n)
    t = pa.table({"ks": pa.array(ks), "ki": ki, "v": v, "w": -v})
    outs = []
    for kw in ({}, {"device_keys": True}):
        ex = GPUAggExecutor(["ks", "ki"], [("ks", "asc"), ("ki", "asc")],
                            "sum(v) as s, min(w) as mn", **kw)
        ex.execute([t], 0, 0)
        outs.append(ex.done(0))
    old, new = outs
    assert old.column_names == new.column_names
    assert old.column("ks").to_pylist() == new.column("ks").to_pylist()
    assert old.column("ki").to_pylist() == new.column("ki").to_pylist()
    np.testing.assert_allclose(np.asarray(new.column("s")),
                               np.asarray(old.column("s")), rtol=1e-9)
    np.testing.assert_allclose(np.asarray(new.column("mn")),
                               np.asarray(old.column("mn")), rtol=0)
    _check_against_acero(new, t, ["ks", "ki"], [("v", "sum", "s"),
                                                ("w", "min", "mn")])
