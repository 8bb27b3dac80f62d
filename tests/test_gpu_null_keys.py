"""Null keys on the device (DESIGN.md §3a'''): qk_key_null_words and
qk_nullword_to_valid against the numpy model of tests/_null_key_cases.py,
exact; the nullable DeviceKeyDict; JoinTable with validity against the
model's join rules; and the executors with null_keys=True against pyarrow
Acero, whose group_by makes one group of null keys per null pattern and
whose join never matches a null key (the semantics of the reference's
DuckDB GROUP BY, polars unique and polars join). Keys exact, SUM at rtol
1e-9, MIN/MAX at rtol 0, as tests/test_gpu_wide_keys.py."""
import numpy as np
import pytest

import _null_key_cases as C

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu

I64_MIN = C.I64_MIN


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _ptr_array(shim, items):
    ptrs = np.array([0 if x is None else x.ptr.value for x in items],
                    dtype=np.uint64)
    return shim.DevColumn.from_numpy(ptrs)


def _bitmap(shim, mask):
    return shim.DevColumn.from_numpy(C.pack_valid(mask))


# ---- 1. qk_key_null_words -------------------------------------------------
@pytest.mark.parametrize("k_n", C.NULL_WORD_K)
@pytest.mark.parametrize("n", C.NULL_WORD_N)
def test_key_null_words_matches_model(gpu, n, k_n):
    shim = gpu
    cols, masks = C.null_word_case(n, k_n)
    want_canon, want_nullw = C.null_words(cols, masks)
    fill = np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    dcols = [shim.DevColumn.from_numpy(c) for c in cols]
    dvalid = [None if m is None else _bitmap(shim, m) for m in masks]
    dcanon = [None if m is None else shim.DevColumn.from_numpy(fill)
              for m in masks]
    dnullw = [shim.DevColumn.from_numpy(fill) for _ in want_nullw]
    arrays = [_ptr_array(shim, x) for x in (dcols, dvalid, dcanon, dnullw)]
    shim.call("qk_key_null_words", None, shim.c_u64(n), k_n,
              *[a.ptr for a in arrays])
    shim.call("qk_stream_sync", None)
    for k in range(k_n):
        assert np.array_equal(dcols[k].to_numpy(n), cols[k]), "input kept"
        if masks[k] is not None:
            assert np.array_equal(dcanon[k].to_numpy(n), want_canon[k]), k
    for w, want in enumerate(want_nullw):
        assert np.array_equal(dnullw[w].to_numpy(n), want), w
    for c in dcols + dnullw + arrays + [x for x in dvalid + dcanon if x]:
        c.free()


# ---- 2. qk_nullword_to_valid ----------------------------------------------
@pytest.mark.parametrize("g", C.NULLWORD_TO_VALID_G)
def test_nullword_to_valid_matches_model(gpu, g):
    shim = gpu
    rng = np.random.default_rng(g)
    null_col = rng.integers(I64_MIN, -I64_MIN - 1, max(g, 1), dtype=np.int64,
                            endpoint=True)
    dcol = shim.DevColumn.from_numpy(null_col)
    nb = C.valid_nbytes(g)
    for bit in (0, 5, 63):
        want, want_nulls = C.nullword_to_valid(null_col, bit, g)
        out = shim.DevColumn.from_numpy(np.full(nb, 0xFF, dtype=np.uint8))
        cnt = shim.DevColumn.from_numpy(np.zeros(1, dtype=np.uint64))
        shim.call("qk_nullword_to_valid", None, shim.c_u64(g), dcol.ptr,
                  bit, out.ptr, cnt.ptr)
        shim.call("qk_stream_sync", None)
        got = out.to_numpy(nb)
        assert np.array_equal(got, want), (g, bit)
        assert not np.unpackbits(got, bitorder="little")[g:].any()
        assert int(cnt.to_numpy(1)[0]) == want_nulls
        out.free()
        cnt.free()
    dcol.free()


# ---- 3. DeviceKeyDict(nullable=True) --------------------------------------
def _encode(shim, kd, cols, masks):
    dcols = [shim.DevColumn.from_numpy(c) for c in cols]
    dcodes = kd.encode(dcols, len(cols[0]), valid=masks)
    codes = dcodes.to_numpy(len(cols[0]))
    for c in dcols + [dcodes]:
        c.free()
    return codes


def test_key_dict_four_tuples_are_four_codes(gpu):
    """(NULL, 0), (0, NULL), (0, 0), (NULL, NULL): four codes, and rows
    that differ only under a null share one."""
    from quokka_amd import ops
    cols, masks = C.GROUP_CASES["four_tuples"]
    kd = ops.DeviceKeyDict(2, expected=8, nullable=True)
    codes = _encode(gpu, kd, cols, masks)
    assert kd.n_codes == 4
    assert len(set(codes[:4].tolist())) == 4
    assert np.array_equal(codes[4:], codes[:4])
    ka, kb = kd.keys_host()
    va, vb = kd.keys_valid_host()
    got = {(None if not va[c] else int(ka[c]),
            None if not vb[c] else int(kb[c])) for c in range(4)}
    assert got == {(None, 0), (0, None), (0, 0), (None, None)}
    assert not ka[~va].any() and not kb[~vb].any(), "0 stored under a null"
    kd.free()


def test_key_dict_nullable_column_supplies_its_bitmap(gpu):
    from quokka_amd import ops, shim
    cols, masks = C.GROUP_CASES["four_tuples"]
    kd = ops.DeviceKeyDict(2, expected=8, nullable=True)
    want = _encode(gpu, kd, cols, masks)
    ncols = [ops.NullableColumn.from_numpy(c, m)
             for c, m in zip(cols, masks)]
    dcodes = kd.encode(ncols, 8)
    assert np.array_equal(dcodes.to_numpy(8), want)
    assert kd.n_codes == 4
    for c in ncols + [dcodes]:
        c.free()
    kd.free()


def test_key_dict_batches_with_and_without_nulls_share_codes(gpu):
    from quokka_amd import ops
    rng = np.random.default_rng(5)
    a = rng.integers(-3, 3, 500).astype(np.int64)
    b = rng.integers(0, 2, 500).astype(np.int64) * I64_MIN
    kd = ops.DeviceKeyDict(2, expected=16, nullable=True)
    c1 = _encode(gpu, kd, [a, b], None)               # valid=None
    n1 = kd.n_codes
    assert C.same_partition(
        c1, C.first_seen_codes(C.key_rows([a, b], [None, None]))[0])
    # batch 2: the same rows, all valid, behind rows with nulls
    ma = rng.random(500) > 0.3
    a2, b2 = np.concatenate([a, a]), np.concatenate([b, b])
    m2 = np.concatenate([ma, np.ones(500, dtype=bool)])
    a2[:500][~ma] = I64_MIN
    c2 = _encode(gpu, kd, [a2, b2], [m2, None])
    assert np.array_equal(c2[500:], c1), "codes of repeated keys are stable"
    assert np.array_equal(c2[:500][ma], c1[ma])
    assert (c2[:500][~ma] >= n1).all(), "a key with a NULL is a new key"
    model = C.first_seen_codes(C.key_rows([a2, b2], [m2, None]))[0]
    assert C.same_partition(c2, model)
    kd.free()


def test_key_dict_growth_keeps_codes_and_nulls(gpu):
    """expected=2, then 5000 distinct keys (every third NULL in key 0,
    distinguished by key 1): codes and keys_valid_host() before the growth
    still hold after it."""
    from quokka_amd import ops
    cols, masks = C.GROUP_CASES["four_tuples"]
    kd = ops.DeviceKeyDict(2, expected=2, nullable=True)
    first = _encode(gpu, kd, cols, masks)
    valid_before = kd.keys_valid_host()
    n = 5000
    a = np.arange(n, dtype=np.int64) + 100
    b = np.arange(n, dtype=np.int64) * 7 + 100
    ma = (np.arange(n) % 3) != 0
    a[~ma] = 0                                # only b tells these rows apart
    big = _encode(gpu, kd, [a, b], [ma, None])
    assert kd.n_codes == 4 + n
    assert np.array_equal(np.sort(big), np.arange(4, 4 + n)), "dense, new"
    again = _encode(gpu, kd, [np.concatenate([cols[0], a]),
                              np.concatenate([cols[1], b])],
                    [np.concatenate([masks[0], ma]),
                     np.concatenate([masks[1], np.ones(n, dtype=bool)])])
    assert np.array_equal(again[:8], first)
    assert np.array_equal(again[8:], big)
    va, vb = kd.keys_valid_host()
    assert np.array_equal(va[:4], valid_before[0])
    assert np.array_equal(vb[:4], valid_before[1])
    assert np.array_equal(va[big], ma) and vb[big].all()
    ka, kb = kd.keys_host()
    assert np.array_equal(ka[big], np.where(ma, a, 0))
    assert np.array_equal(kb[big], b)
    kd.free()


def test_valid_on_a_non_nullable_dictionary_raises(gpu):
    from quokka_amd import ops, shim
    kd = ops.DeviceKeyDict(1, expected=4)
    col = shim.DevColumn.from_numpy(np.arange(4, dtype=np.int64))
    with pytest.raises(TypeError, match="nullable=True"):
        kd.encode([col], 4, valid=[np.ones(4, dtype=bool)])
    with pytest.raises(TypeError, match="nullable=True"):
        kd.keys_valid_host()
    gb = ops.GroupByKeys(1, 0)
    with pytest.raises(TypeError, match="nullable=True"):
        gb.update([col], [], 4, key_valid=[None])
    col.free()
    gb.free()
    kd.free()


# ---- 4. GPUAggExecutor(device_keys=True, null_keys=True) ------------------
def _check_against_acero(got, table, keys, aggs):
    """As tests/test_gpu_wide_keys.py; sort_by places the null keys of both
    tables at the same end."""
    want = table.group_by(keys, use_threads=False).aggregate(
        [(c, fn) for c, fn, _ in aggs])
    order = [(k, "ascending") for k in keys]
    g, w = got.sort_by(order), want.sort_by(order)
    assert g.num_rows == w.num_rows
    for k in keys:
        gk, wk = g.column(k).combine_chunks(), w.column(k).combine_chunks()
        assert gk.type == wk.type, (k, gk.type, wk.type)
        assert gk.null_count == wk.null_count, k
        if pa.types.is_floating(gk.type):       # Array.equals: NaN != NaN
            assert gk.is_valid().equals(wk.is_valid()), k
            gv, wv = (np.asarray(a.fill_null(0.0)) for a in (gk, wk))
            assert np.array_equal(gv, wv, equal_nan=True), k
            assert not np.signbit(gv[gv == 0]).any(), "zero comes back +0.0"
        else:
            assert gk.equals(wk), k
    for c, fn, alias in aggs:
        np.testing.assert_allclose(
            np.asarray(g.column(alias)), np.asarray(w.column("%s_%s" % (c, fn))),
            rtol=1e-9 if fn == "sum" else 0, atol=0, err_msg=alias)


def _nullify(rng, arr, frac, first_clean):
    """~frac nulls, none among the first `first_clean` rows."""
    mask = rng.random(len(arr)) < frac
    mask[:first_clean] = False
    return pa.array(arr, mask=mask)


def _five_key_table(rng, n, first_clean, all_null=None):
    """-> (table for the executor, table for Acero, key names). The two
    differ in one thing: the float key holds -0.0, which the project
    groups with +0.0 and returns as +0.0 (DESIGN.md §3a''), while Acero
    groups by bit pattern; so Acero is asked about the column with -0.0
    written as +0.0. NaN (one payload) is one group for both."""
    pool = np.array(["seg-%03d" % i for i in range(12)], dtype=object)
    f = np.array([0.0, -0.0, np.nan, 100.5, -7.25])[rng.integers(0, 5, n)]
    cols = {
        "k_i32": rng.integers(-2, 3, n).astype(np.int32),
        "k_i64": (rng.integers(0, 4, n).astype(np.int64) - 2) * (1 << 40),
        "k_d32": rng.integers(8035, 8038, n).astype(np.int32),
        "k_str": pool[rng.integers(0, len(pool), n)],
        "k_f64": f,
    }
    t = {}
    for k, v in cols.items():
        a = pa.nulls(n, pa.array(v[:1]).type) if k == all_null \
            else _nullify(rng, v, 0.2, first_clean)
        t[k] = a.cast(pa.date32()) if k == "k_d32" else a
    t["v"] = pa.array(rng.random(n))
    t["w"] = pa.array(rng.standard_normal(n))
    t["x"] = pa.array(rng.standard_normal(n))
    t = pa.table(t)
    fk = t.column("k_f64").combine_chunks()
    oracle = t.set_column(
        t.column_names.index("k_f64"), "k_f64",
        pa.array(np.asarray(fk.fill_null(0.0)) + 0.0,
                 mask=np.asarray(fk.is_null())))
    return t, oracle, list(cols)


_AGGS = [("v", "sum", "sv"), ("w", "min", "mn"), ("x", "max", "mx")]
_BATCHES = ((0, 7000), (7000, 7001), (7001, 20_000))


@pytest.mark.parametrize("all_null", [None, "k_i64", "k_str"])
def test_agg_five_nullable_keys_vs_acero(gpu, all_null):
    """int32, wide int64, date32, string and float64 keys, ~20 % nulls
    each, 20 000 rows in three batches of which the first has no nulls;
    then the same with one key column entirely NULL."""
    from quokka_amd.executors import GPUAggExecutor
    rng = np.random.default_rng(41)
    t, oracle, keys = _five_key_table(rng, 20_000,
                                      0 if all_null else 7000, all_null)
    if not all_null:
        assert not any(t.slice(0, 7000).column(k).null_count for k in keys)
    fk = np.asarray(t.column("k_f64").combine_chunks().fill_null(1.0))
    assert np.isnan(fk).any() and np.signbit(fk[fk == 0]).any()
    ex = GPUAggExecutor(keys, None,
                        "sum(v) as sv, min(w) as mn, max(x) as mx",
                        device_keys=True, null_keys=True)
    for lo, hi in _BATCHES:
        ex.execute([t.slice(lo, hi - lo)], 0, 0)
    out = ex.done(0)
    assert out.column("k_d32").type == pa.date32()
    _check_against_acero(out, oracle, keys, _AGGS)
    if all_null:
        assert out.column(all_null).null_count == out.num_rows


def test_float_key_nan_zero_and_null(gpu):
    """-0.0 / +0.0 one group, NaNs one group, NULL a third kind of group:
    none of them meets the stored 0 of a null slot. Expectation written
    here, as in test_float_keys_zero_and_nan."""
    from quokka_amd.executors import GPUAggExecutor
    nan = float("nan")
    f = pa.array([0.0, -0.0, None, nan, None, 1.5, nan, 0.0])
    v = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])
    ex = GPUAggExecutor(["f"], None, "sum(v) as sv", device_keys=True,
                        null_keys=True)
    ex.execute([pa.table({"f": f.slice(0, 3), "v": v[:3]})], 0, 0)
    ex.execute([pa.table({"f": f.slice(3), "v": v[3:]})], 0, 0)
    out = ex.done(0)
    assert out.column("f").type == pa.float64()
    got = {}
    for fv, sv in zip(out.column("f").to_pylist(),
                      out.column("sv").to_pylist()):
        got["nan" if fv is not None and fv != fv else fv] = sv
    assert got == {0.0: 131.0, None: 20.0, "nan": 72.0, 1.5: 32.0}


@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_agg_order_by_nullable_key_nulls_last(gpu, direction):
    from quokka_amd.executors import GPUAggExecutor
    rng = np.random.default_rng(43)
    n = 3000
    g = _nullify(rng, rng.integers(-20, 20, n).astype(np.int64), 0.2, 0)
    s = _nullify(rng, np.array(["s%d" % i for i in rng.integers(0, 4, n)],
                               dtype=object), 0.2, 0)
    t = pa.table({"g": g, "s": s, "v": rng.random(n)})
    ex = GPUAggExecutor(["g", "s"], [("g", direction), ("s", "asc")],
                        "sum(v) as sv", device_keys=True, null_keys=True)
    ex.execute([t.slice(0, 1000)], 0, 0)
    ex.execute([t.slice(1000)], 0, 0)
    out = ex.done(0)
    _check_against_acero(out, t, ["g", "s"], [("v", "sum", "sv")])
    want = out.sort_by([("g", direction + "ending"), ("s", "ascending")])
    assert out.column("g").to_pylist() == want.column("g").to_pylist()
    assert out.column("s").to_pylist() == want.column("s").to_pylist()
    gl = out.column("g").to_pylist()
    assert gl[-1] is None and gl[0] is not None, "NULLs last"


# ---- 5. GPUDistinctExecutor(null_keys=True) --------------------------------
@pytest.mark.parametrize("keys", [["a"], ["a", "s", "d"]])
def test_distinct_null_keys_first_occurrences(gpu, keys):
    """Three batches; nulls equal each other. The emitted rows are the
    first occurrences in order, by the model and by pandas."""
    pd = pytest.importorskip("pandas")
    from quokka_amd.executors import GPUDistinctExecutor
    rng = np.random.default_rng(50 + len(keys))
    ex = GPUDistinctExecutor(keys[0] if len(keys) == 1 else keys,
                             null_keys=True)
    seen, tables, emitted = {}, [], []
    for b in range(3):
        n = 1500
        t = pa.table({
            "a": _nullify(rng, rng.integers(0, 40 + 20 * b, n)
                          .astype(np.int64), 0.2, 0),
            "s": _nullify(rng, np.array(
                ["s%d" % i for i in rng.integers(0, 3, n)], dtype=object),
                0.2, 0),
            "d": _nullify(rng, rng.integers(8000, 8003, n).astype(np.int32),
                          0.2, 0).cast(pa.date32()),
            "row": pa.array(np.arange(n) + 10_000 * b)})
        out = ex.execute([t], 0, 0)
        # the model over words built here, not by the executor
        word = {"a": int, "s": lambda v: int(v[1:]),
                "d": lambda v: v.toordinal()}
        cols, masks = [], []
        for k in keys:
            py = t.column(k).to_pylist()
            masks.append(np.array([v is not None for v in py]))
            cols.append(np.array([0 if v is None else word[k](v)
                                  for v in py], dtype=np.int64))
        before = len(seen)
        codes, seen = C.first_seen_codes(C.key_rows(cols, masks), seen)
        _, first = np.unique(codes, return_index=True)
        want_rows = sorted(int(i) + 10_000 * b for i in first
                           if codes[i] >= before)
        got_rows = [] if out is None else out.column("row").to_pylist()
        assert got_rows == want_rows
        tables.append(t)
        if out is not None:
            emitted.append(out)
            for k in keys:
                assert out.column(k).type == t.column(k).type
    every = pa.concat_tables(tables).to_pandas()
    want = every.drop_duplicates(subset=keys, keep="first")
    got = pa.concat_tables(emitted)
    assert got.column("row").to_pylist() == want["row"].tolist()
    assert got.column(keys[0]).null_count >= 1
    assert ex.done(0) is None


# ---- 6. JoinTable with validity --------------------------------------------
@pytest.mark.parametrize("n_probe", C.JOIN_N_PROBE)
def test_join_table_valid_matches_model(gpu, n_probe):
    from quokka_amd import ops, shim
    builds, (pk, pm) = C.join_case(n_probe)
    bk = np.concatenate([k for k, _ in builds])
    bm = np.concatenate([m for _, m in builds])
    assert (bk[~bm] == I64_MIN).any(), "INT64_MIN under a null build row"
    if n_probe > 1:
        assert np.isin(bk[~bm], pk[pm]).any(), "a probed key under another"
    assert np.isin(pk[~pm], bk[bm]).all(), "built keys under null probes"
    assert len(set(bk[bm].tolist())) < int(bm.sum()), "duplicate build keys"
    jt = ops.JoinTable(len(bk))
    for k, m in builds:                       # two build() calls
        col = shim.DevColumn.from_numpy(k)
        jt.build(col, valid=m)
        col.free()
    assert jt.n_build == len(bk), "null rows take their row number"
    # probed twice: as a plain column that still holds built keys under its
    # nulls with the mask beside it, and as a NullableColumn (0 under
    # nulls) that supplies its own bitmap
    kcol = ops.NullableColumn.from_numpy(pk, pm)
    raw = shim.DevColumn.from_numpy(pk)
    for mode in (0, 1, 2):
        want = C.join(bk, bm, pk, pm, mode)
        for col, valid in ((raw, pm), (kcol, None)):
            pidx, bidx, cnt = jt.probe(col, mode=mode, valid=valid,
                                       n=len(pk))
            p = pidx.to_numpy(cnt)
            if mode == 0:
                b = bidx.to_numpy(cnt)
                assert sorted(zip(p.tolist(), b.tolist())) == want
                # build indices address the payload: the key at the build
                # row is the probe row's key, and the row is valid
                assert np.array_equal(bk[b], pk[p]) and bm[b].all()
                bidx.free()
            else:
                assert sorted(p.tolist()) == want
            pidx.free()
    raw.free()
    kcol.free()
    jt.free()


def test_join_table_undersized_output_regrows_with_valid(gpu):
    """The count-then-regrow loop of probe() with a bitmap: 64 matches per
    valid probe row against the first guess of 1.5 n."""
    from quokka_amd import ops, shim
    bk = np.repeat(np.arange(4, dtype=np.int64), 64)
    bm = np.ones(len(bk), dtype=bool)
    bm[::2] = False
    pk = np.arange(4, dtype=np.int64).repeat(8)
    pm = np.arange(32) % 4 != 0
    jt = ops.JoinTable(len(bk))
    col = shim.DevColumn.from_numpy(bk)
    jt.build(col, valid=bm)
    col.free()
    pcol = shim.DevColumn.from_numpy(pk)
    pidx, bidx, cnt = jt.probe(pcol, mode=0, valid=pm)
    want = C.join(bk, bm, pk, pm, 0)
    assert cnt == len(want) == 24 * 32
    assert sorted(zip(pidx.to_numpy(cnt).tolist(),
                      bidx.to_numpy(cnt).tolist())) == want
    for c in (pcol, pidx, bidx):
        c.free()
    jt.free()


# ---- 7. GPUBuildProbeJoinExecutor(null_keys=True) ---------------------------
_ACERO_HOW = {"inner": "inner", "left": "left outer", "semi": "left semi",
              "anti": "left anti"}


def _join_tables(rng, string_keys):
    def key(n, hi):
        k = rng.integers(0, hi, n)
        if string_keys:
            return _nullify(rng, np.array(["k%d" % i for i in k],
                                          dtype=object), 0.2, 0)
        return _nullify(rng, k.astype(np.int64) * (1 << 33), 0.2, 0)
    nb, n_p = 300, 900
    build = pa.table({"k": key(nb, 60), "bv": rng.random(nb),
                      "bi": np.arange(nb, dtype=np.int64)})
    probe = pa.table({"k": key(n_p, 90), "pv": rng.random(n_p),
                      "pi": np.arange(n_p, dtype=np.int64)})
    return build, probe


def _rows(t, names):
    key = lambda r: tuple((v is None, v) for v in r)        # noqa: E731
    return sorted(zip(*(t.column(c).to_pylist() for c in names)), key=key)


@pytest.mark.parametrize("string_keys", [False, True])
@pytest.mark.parametrize("how", ["inner", "left", "semi", "anti"])
def test_join_executor_null_keys_vs_acero(gpu, how, string_keys):
    from quokka_amd.executors import GPUBuildProbeJoinExecutor
    rng = np.random.default_rng(70 + string_keys)
    build, probe = _join_tables(rng, string_keys)
    assert build.column("k").null_count and probe.column("k").null_count
    ex = GPUBuildProbeJoinExecutor(on="k", how=how, null_keys=True)
    ex.execute([build.slice(0, 120)], 1, 0)
    ex.execute([build.slice(120)], 1, 0)
    outs = [ex.execute([probe.slice(0, 400)], 0, 0),
            ex.execute([probe.slice(400)], 0, 0)]
    got = pa.concat_tables([o for o in outs if o is not None])
    want = probe.join(build, "k", join_type=_ACERO_HOW[how],
                      use_threads=False)
    names = want.column_names
    assert sorted(got.column_names) == sorted(names)
    assert got.num_rows == want.num_rows
    assert _rows(got, names) == _rows(want, names)
    for o in outs:
        assert o.column("k").type == probe.column("k").type
    if how in ("left", "anti"):
        assert got.column("k").null_count == probe.column("k").null_count
    else:
        assert got.column("k").null_count == 0


def test_broadcast_join_null_keys_vs_acero(gpu):
    from quokka_amd import GPUBroadcastJoinExecutor
    rng = np.random.default_rng(72)
    build, probe = _join_tables(rng, False)
    ex = GPUBroadcastJoinExecutor(build, on="k", null_keys=True)
    got = ex.execute([probe], 0, 0)
    want = probe.join(build, "k", join_type="inner", use_threads=False)
    assert _rows(got, want.column_names) == _rows(want, want.column_names)
