"""Join payloads that keep their NULLs (DESIGN.md §3a'''''), on the device:
qk_take_opt_* and JoinTable.probe(mode=3) against the plain-Python model of
tests/_join_payload_cases.py, exact; the join executors with
null_payloads=True against pyarrow Acero after sorting both on the row-id
columns, every value exact and float64 by bit pattern; and a chain of three
joins into GPUAggExecutor(null_values=True) against Acero's join +
group_by."""
import numpy as np
import pytest

import _join_payload_cases as C

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu

NO_ROW = C.NO_ROW


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _sizes():
    from quokka_amd import shim
    return shim.BLOCK_THREADS, shim.MAX_BLOCKS


# ---- 1. qk_take_opt_* -----------------------------------------------------
def _dirty_pool(shim, dtype, n):
    """Leave a 0xFF-filled value buffer and bitmap of exactly the sizes
    take_optional is about to ask for in the device pool, so that what the
    kernel and its caller do not write shows."""
    for nbytes in (n * np.dtype(dtype).itemsize, C.valid_nbytes(n)):
        buf = shim.DevBuffer(nbytes)
        shim.call("qk_dmemset", buf.ptr, 0xFF, shim.c_u64(max(1, nbytes)))
        buf.free()


@pytest.mark.parametrize("dtype", C.TAKE_DTYPES,
                         ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("size_i", range(12))
def test_take_optional_matches_model(gpu, size_i, dtype):
    from quokka_amd import ops
    shim = gpu
    n = C.take_sizes(*_sizes())[size_i]
    assert ops.NO_ROW == NO_ROW
    rng = np.random.default_rng([size_i, np.dtype(dtype).itemsize])
    for pattern in C.TAKE_PATTERNS:
        idx = C.take_idx(n, pattern, rng)
        didx = shim.DevColumn.from_numpy(idx)
        for bitmap in C.TAKE_BITMAPS:
            vals, mask = C.take_source(dtype, bitmap, idx, rng)
            # built directly: from_numpy would zero the slots under nulls
            src = shim.DevColumn.from_numpy(vals)
            if mask is not None:
                vb = shim.DevColumn.from_numpy(C.pack_valid(mask))
                src = ops.NullableColumn(src, vb, len(vals),
                                         int((~mask).sum()))
            no = idx == NO_ROW
            ok = ~no
            if mask is not None:
                ok[~no] = mask[idx[~no]]
            want = np.zeros(n, dtype=dtype)
            want[ok] = vals[idx[ok]]
            _dirty_pool(shim, dtype, n)
            got = ops.take_optional(src, didx, n)
            what = (n, pattern, bitmap)
            assert got.n == n and got.dtype == np.dtype(dtype), what
            gv = got.to_numpy(n)
            assert np.array_equal(gv.view(np.uint8), want.view(np.uint8)), \
                what                        # bit-exact, 0 under every null
            assert not gv[~ok].view(np.uint8).any(), what
            nb = C.valid_nbytes(n)
            raw = np.empty(nb, dtype=np.uint8)
            shim.call("qk_d2h", raw.ctypes.data_as(shim.c_vp),
                      got.valid.ptr, shim.c_u64(nb))
            assert np.array_equal(raw, C.pack_valid(ok)), what
            assert not np.unpackbits(raw, bitorder="little")[n:].any(), what
            assert got.null_count == int(n - ok.sum()), what
            got.free()
            src.free()
        didx.free()


def test_take_optional_small_case_against_the_list_model(gpu):
    """The numpy expectation above and the list model agree with the
    device on a case small enough to read."""
    from quokka_amd import ops
    shim = gpu
    vals = np.array([10, 20, 30, 40], dtype=np.int64)
    mask = np.array([True, False, True, True])
    idx = np.array([2, NO_ROW, 1, 0, 3, NO_ROW], dtype=np.uint32)
    want_v, want_ok, want_nulls = C.take_opt(vals.tolist(), mask.tolist(),
                                             idx.tolist())
    junk = vals.copy()
    junk[~mask] = C.JUNK[np.int64]
    src = ops.NullableColumn(shim.DevColumn.from_numpy(junk),
                             shim.DevColumn.from_numpy(C.pack_valid(mask)),
                             4, 1)
    didx = shim.DevColumn.from_numpy(idx)
    got = ops.take_optional(src, didx)
    assert got.to_numpy().tolist() == want_v
    assert got.valid_to_numpy().tolist() == want_ok
    assert got.null_count == want_nulls == 3
    for c in (got, src, didx):
        c.free()


def test_take_optional_refuses_unknown_dtype(gpu):
    from quokka_amd import ops
    col = gpu.DevColumn.from_numpy(np.zeros(4, dtype=np.uint64))
    idx = gpu.DevColumn.from_numpy(np.zeros(4, dtype=np.uint32))
    with pytest.raises(TypeError, match="uint64"):
        ops.take_optional(col, idx)
    col.free()
    idx.free()


# ---- 2. probe mode 3 ------------------------------------------------------------
def _probe_pairs(shim, table, keys, mask, mode, **kw):
    kcol = shim.DevColumn.from_numpy(keys)
    p, b, total = table.probe(kcol, mode=mode, valid=mask, **kw)
    pi = p.to_numpy(total).tolist()
    if b is None:
        got = sorted(pi)
    else:
        got = sorted(zip(pi, b.to_numpy(total).tolist()))
        b.free()
    p.free()
    kcol.free()
    return got, total


def _build_table(shim, build):
    from quokka_amd import ops
    table = ops.JoinTable(max(16, len(build)))
    if len(build):
        bcol = shim.DevColumn.from_numpy(build)
        table.build(bcol)
        bcol.free()
    return table


@pytest.mark.parametrize("with_bitmap", [False, True],
                         ids=["no bitmap", "bitmap"])
@pytest.mark.parametrize("size_i,kind", [
    (i, k) for i in range(4) for k in ("unique", "chains", "empty")
] + [(4, "chains")])    # beyond one grid round: once, the model is a loop
def test_probe_left_matches_model(gpu, size_i, kind, with_bitmap):
    shim = gpu
    n = C.probe_sizes(*_sizes())[size_i]
    rng = np.random.default_rng([size_i, len(kind), with_bitmap])
    build, keys, mask = C.probe_case(kind, n, rng)
    if not with_bitmap:
        mask = None
    elif n == 1:
        mask[:] = False                  # the one row is a NULL key
    table = _build_table(shim, build)
    bl, kl = build.tolist(), keys.tolist()
    ml = None if mask is None else mask.tolist()
    want = C.probe(bl, None, kl, ml, 3)
    got, total = _probe_pairs(shim, table, keys, mask, 3)
    assert got == want
    by_key = {}
    for k in bl:
        by_key[k] = by_key.get(k, 0) + 1
    matches = [by_key.get(k, 0) if ml is None or ml[i] else 0
               for i, k in enumerate(kl)]
    assert total == sum(max(1, m) for m in matches)
    assert {p for p, _ in got} == set(range(n)), "every probe row emitted"
    if kind == "empty":
        assert got == [(i, NO_ROW) for i in range(n)]
    # the other modes did not move
    for mode in (0, 1, 2):
        got_m, _ = _probe_pairs(shim, table, keys, mask, mode)
        assert got_m == C.probe(bl, None, kl, ml, mode), mode
    table.free()


@pytest.mark.parametrize("with_bitmap", [False, True],
                         ids=["no bitmap", "bitmap"])
def test_probe_left_reprobe_gives_the_same_pairs(gpu, with_bitmap):
    """An output guess of 16 pairs for 1000 probe rows: the cursor counts
    past the capacity and the second pass emits everything."""
    shim = gpu
    rng = np.random.default_rng(7)
    build, keys, mask = C.probe_case("chains", 1000, rng)
    if not with_bitmap:
        mask = None
    table = _build_table(shim, build)
    first, total = _probe_pairs(shim, table, keys, mask, 3)
    again, total2 = _probe_pairs(shim, table, keys, mask, 3,
                                 out_factor=0.001)
    assert total > 16 and total2 == total
    assert again == first == C.probe(
        build.tolist(), None, keys.tolist(),
        None if mask is None else mask.tolist(), 3)
    table.free()


def test_probe_left_null_build_keys(gpu):
    """NULL keys on the build side take no slot: their probe partners are
    misses and come out once with NO_ROW."""
    from quokka_amd import ops
    shim = gpu
    build = np.array([5, 7, 5, 9, 7, 5], dtype=np.int64)
    bvalid = np.array([True, True, True, False, True, True])
    keys = np.array([5, 6, 7, 9, 5], dtype=np.int64)
    pvalid = np.array([True, True, True, True, False])
    table = ops.JoinTable(16)
    bcol = shim.DevColumn.from_numpy(build)
    table.build(bcol, valid=bvalid)
    got, total = _probe_pairs(shim, table, keys, pvalid, 3)
    assert got == C.probe(build.tolist(), bvalid.tolist(), keys.tolist(),
                          pvalid.tolist(), 3)
    assert total == 8
    bcol.free()
    table.free()


def test_probe_valid_entry_point_checks_mode_3_arguments(gpu):
    shim = gpu
    table = _build_table(shim, np.arange(4, dtype=np.int64))
    keys = shim.DevColumn.from_numpy(np.arange(4, dtype=np.int64))
    bits = shim.DevColumn.from_numpy(C.pack_valid(np.ones(4, dtype=bool)))
    out = shim.DevColumn(np.uint32, 16)
    cur = shim.DevColumn.from_numpy(np.zeros(1, dtype=np.uint64))
    args = (table.slot_keys.ptr, table.slot_head.ptr, table.chain_next.ptr,
            shim.c_u64(table.cap))
    for name, head in (("qk_join_probe", (keys.ptr,)),
                       ("qk_join_probe_valid", (keys.ptr, bits.ptr))):
        with pytest.raises(shim.QkError):     # mode 3 needs out_build
            shim.call(name, None, shim.c_u64(4), *head, *args, 3, out.ptr,
                      None, shim.c_u64(16), cur.ptr)
    with pytest.raises(shim.QkError):
        shim.call("qk_join_probe_valid", None, shim.c_u64(4), keys.ptr,
                  bits.ptr, *args, 4, out.ptr, out.ptr, shim.c_u64(16),
                  cur.ptr)
    for c in (keys, bits, out, cur):
        c.free()
    table.free()


# ---- 3. executors -----------------------------------------------------------------
def _run_join(c, how, **kw):
    from quokka_amd.executors import GPUBuildProbeJoinExecutor
    ex = GPUBuildProbeJoinExecutor(
        left_on=c["left_on"], right_on=c["right_on"], how=how,
        key_to_keep=c["key_to_keep"], null_keys=c["null_keys"],
        null_payloads=True, **kw)
    for b in c["build_batches"]:
        ex.execute([b], 1, 0)
    return ex.execute([c["probe"]], 0, 0)


@pytest.mark.parametrize("how", C.HOWS)
@pytest.mark.parametrize("name", sorted(C.EXECUTOR_CASES))
def test_join_null_payloads_matches_acero(gpu, name, how):
    """Every payload type on both sides, NULLs kept, every column in the
    type it arrived in, names and order as the default path's."""
    c = C.executor_case(pa, name)
    got = _run_join(c, how)
    want = C.acero_join(c["probe"], c["build"], how, c["left_on"],
                        c["right_on"], c["key_to_keep"])
    C.assert_tables_equal(got, want, ["pid", "bid"])
    if how == "left":
        assert got.column("bid").null_count > 0
        assert got.column("b_str").null_count > got.column("bid").null_count


def test_join_null_payloads_probe_in_batches(gpu):
    """Two probe batches against one build state: each is its own join."""
    from quokka_amd.executors import GPUBuildProbeJoinExecutor
    c = C.executor_case(pa, "int key")
    ex = GPUBuildProbeJoinExecutor(on="k", how="left", null_payloads=True)
    ex.execute([c["build"]], 1, 0)
    for part in (c["probe"].slice(0, 77), c["probe"].slice(77)):
        got = ex.execute([part], 0, 0)
        want = C.acero_join(part, c["build"], "left", "k", "k")
        C.assert_tables_equal(got, want, ["pid", "bid"])


@pytest.mark.parametrize("how", C.HOWS)
def test_broadcast_join_null_payloads(gpu, how):
    from quokka_amd.executors import GPUBroadcastJoinExecutor
    c = C.executor_case(pa, "null int keys")
    ex = GPUBroadcastJoinExecutor(c["build"], on="k", how=how,
                                  null_keys=True, null_payloads=True)
    got = ex.execute([c["probe"]], 0, 0)
    want = C.acero_join(c["probe"], c["build"], how, "k", "k")
    C.assert_tables_equal(got, want, ["pid", "bid"])


def test_decimal_payload_raises_naming_the_column(gpu):
    import decimal
    from quokka_amd.executors import GPUBuildProbeJoinExecutor
    dec = pa.array([decimal.Decimal("1.50"), None], type=pa.decimal128(9, 2))
    k = pa.array([1, 2], type=pa.int64())
    ex = GPUBuildProbeJoinExecutor(on="k", how="inner", null_payloads=True)
    with pytest.raises(TypeError, match="b_dec"):
        ex.execute([pa.table({"k": k, "b_dec": dec})], 1, 0)
    ex = GPUBuildProbeJoinExecutor(on="k", how="inner", null_payloads=True)
    ex.execute([pa.table({"k": k, "b": k})], 1, 0)
    with pytest.raises(TypeError, match="p_dec"):
        ex.execute([pa.table({"k": k, "p_dec": dec})], 0, 0)
    ts = pa.array([1, None], type=pa.timestamp("us"))
    with pytest.raises(TypeError, match="p_ts"):
        ex.execute([pa.table({"k": k, "p_ts": ts})], 0, 0)


def test_empty_build_rule_unchanged(gpu):
    from quokka_amd.executors import GPUBuildProbeJoinExecutor
    c = C.executor_case(pa, "int key")
    for how in C.HOWS:
        ex = GPUBuildProbeJoinExecutor(on="k", how=how, null_payloads=True)
        got = ex.execute([c["probe"]], 0, 0)
        if how == "anti":
            C.assert_tables_equal(got, c["probe"], ["pid"])
        else:
            assert got is None


@pytest.mark.parametrize("how", ["inner", "left"])
def test_default_path_unchanged(gpu, how):
    """null_payloads=False: int64 key, int64 and float64 payloads, no
    NULLs, as the existing join tests; the expectation is Acero's."""
    from quokka_amd.executors import GPUBuildProbeJoinExecutor
    rng = np.random.default_rng(11)
    build = pa.table({"k": rng.integers(0, 120, 200).astype(np.int64),
                      "bid": np.arange(200, dtype=np.int64),
                      "b_f64": rng.standard_normal(200)})
    probe = pa.table({"pid": np.arange(300, dtype=np.int64),
                      "k": rng.integers(0, 240, 300).astype(np.int64),
                      "p_f64": rng.standard_normal(300)})
    ex = GPUBuildProbeJoinExecutor(on="k", how=how)
    ex.execute([build.slice(0, 90)], 1, 0)
    ex.execute([build.slice(90)], 1, 0)
    got = ex.execute([probe], 0, 0)
    want = C.acero_join(probe, build, how, "k", "k")
    assert got.column_names == want.column_names
    order = [("pid", "ascending"), ("bid", "ascending")]
    g, w = got.sort_by(order), want.sort_by(order)
    for name in w.column_names:
        assert g.column(name).to_pylist() == w.column(name).to_pylist(), name
    if how == "left":
        assert g.column("bid").null_count > 0


# ---- 4. a chain of joins into the aggregate -----------------------------------
def test_left_join_output_feeds_joins_and_aggregate(gpu):
    """Q13's shape: a left join, whose NULL build payloads then travel as
    the probe of a second join, as the build of a third, and into
    GPUAggExecutor(null_values=True). Every join is compared with Acero's,
    the end with Acero's group_by."""
    from quokka_amd.executors import (GPUBuildProbeJoinExecutor,
                                      GPUAggExecutor)
    rng = np.random.default_rng(13)

    def ints(n, hi):
        return rng.integers(0, hi, n).astype(np.int64)

    def nullable_vals(n):
        v = rng.integers(-50, 50, n).astype(np.float64).tolist()
        return pa.array([None if rng.random() < 0.25 else x for x in v],
                        type=pa.float64())
    p = pa.table({"pid": np.arange(200, dtype=np.int64), "k": ints(200, 60),
                  "p_i64": pa.array([None, 2 ** 53 + 1] * 100,
                                    type=pa.int64())})
    b1 = pa.table({"bid": np.arange(40, dtype=np.int64), "k": ints(40, 30),
                   "b_val": nullable_vals(40),
                   "b_str": pa.array(["", None, "x", "yy"] * 10)})
    b2 = pa.table({"cid": np.arange(50, dtype=np.int64), "k": ints(50, 45),
                   "c_val": nullable_vals(50),
                   "c_d32": pa.array([None, 7, 8, 9, 10] * 10,
                                     type=pa.int32()).cast(pa.date32())})
    p3 = pa.table({"qid": np.arange(80, dtype=np.int64), "k": ints(80, 60)})

    def join(probe, build, how):
        ex = GPUBuildProbeJoinExecutor(on="k", how=how, null_payloads=True)
        ex.execute([build], 1, 0)
        got = ex.execute([probe], 0, 0)
        C.assert_tables_equal(got, C.acero_join(probe, build, how, "k", "k"),
                              ["qid", "pid", "bid", "cid"])
        return got
    t1 = join(p, b1, "left")
    assert t1.column("b_val").null_count > t1.column("bid").null_count > 0
    t2 = join(t1, b2, "left")            # t1 as the probe
    t3 = join(p3, t2, "inner")           # t2 as the build
    assert t3.num_rows and t3.column("c_d32").type == pa.date32()
    agg = GPUAggExecutor(["k"], None,
                         "sum(b_val) as s, min(c_val) as mn, max(b_val) as mx",
                         device_keys=True, null_values=True)
    vals = t3.select(["k", "b_val", "c_val"])
    agg.execute([vals.slice(0, t3.num_rows // 2)], 0, 0)
    agg.execute([vals.slice(t3.num_rows // 2)], 0, 0)
    got = agg.done(0).sort_by("k")
    want = p3.join(p.join(b1, "k", join_type="left outer")
                   .join(b2, "k", join_type="left outer"), "k",
                   join_type="inner") \
        .group_by("k", use_threads=False) \
        .aggregate([("b_val", "sum"), ("c_val", "min"), ("b_val", "max")]) \
        .sort_by("k")
    assert got.column("k").to_pylist() == want.column("k").to_pylist()
    # integer-valued float64 inputs: the sums are exact in any order
    for alias, col in (("s", "b_val_sum"), ("mn", "c_val_min"),
                       ("mx", "b_val_max")):
        assert got.column(alias).to_pylist() == \
            want.column(col).to_pylist(), alias
    assert None in got.column("s").to_pylist()
