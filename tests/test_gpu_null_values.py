"""Null values in the aggregate on the device (DESIGN.md §3a''''):
qk_groupby_dense_acc_valid against the numpy model of
tests/_null_value_cases.py, ops.GroupByKeys(nullable_vals=True) across
batches and growth, and GPUAggExecutor(null_values=True) against pyarrow
Acero, whose sum / min / max skip nulls and give NULL for a group without
a value (the rules of the reference's DuckDB GROUP BY). Values are small
integers in doubles: SUM at rtol 1e-9 (the project's gate), MIN / MAX and
validity exact."""
import numpy as np
import pytest

import _null_value_cases as C

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _check(got, want, ops):
    (acc, valid), (wacc, wvalid) = got, want
    assert np.array_equal(valid, wvalid)
    for c, op in enumerate(ops):
        np.testing.assert_allclose(acc[c], wacc[c],
                                   rtol=1e-9 if op == C.SUM else 0, atol=0,
                                   err_msg="column %d" % c)


def _run_kernel(shim, codes, vals, masks, ops, ngroups, pad_rows=0):
    """One qk_groupby_dense_acc_valid call over fresh records. The input
    buffers hold pad_rows more rows than n is told: code 0, garbage values
    and, in the bitmaps, 1 bits. -> (acc, valid, inputs unchanged)."""
    n, nvals = len(codes), len(vals)
    rstride = 1
    while rstride < nvals:
        rstride *= 2
    host_codes = np.concatenate([codes, np.zeros(pad_rows, dtype=np.uint32)])
    host_vals = [np.concatenate([v, np.full(pad_rows, C.JUNK[op])])
                 for v, op in zip(vals, ops)]
    host_bits = [None if m is None else C.pack_valid(m, tail=1)
                 for m in masks]
    dcodes = shim.DevColumn.from_numpy(host_codes)
    dvals = [shim.DevColumn.from_numpy(v) for v in host_vals]
    dbits = [None if b is None else shim.DevColumn.from_numpy(b)
             for b in host_bits]
    vptrs = shim.DevColumn.from_numpy(
        np.array([d.ptr.value for d in dvals], dtype=np.uint64))
    bptrs = shim.DevColumn.from_numpy(
        np.array([0 if d is None else d.ptr.value for d in dbits],
                 dtype=np.uint64))
    inits = shim.DevColumn.from_numpy(
        np.array([C.AGG_INIT[op] for op in ops], dtype=np.float64))
    dops = shim.DevColumn.from_numpy(np.array(ops, dtype=np.int32))
    acc = shim.DevColumn(np.float64, ngroups * rstride)
    seen = shim.DevColumn.from_numpy(np.zeros(ngroups, dtype=np.uint64))
    err = shim.DevColumn.from_numpy(np.zeros(1, dtype=np.uint32))
    shim.call("qk_groupby_dense_init", None, acc.ptr, shim.c_u64(0),
              shim.c_u64(ngroups), rstride, nvals, inits.ptr)
    shim.call("qk_groupby_dense_acc_valid", None, shim.c_u64(n), dcodes.ptr,
              shim.c_u32(ngroups), vptrs.ptr, bptrs.ptr, dops.ptr, nvals,
              rstride, acc.ptr, seen.ptr, err.ptr)
    shim.call("qk_stream_sync", None)
    assert int(err.to_numpy(1)[0]) == 0
    recs = acc.to_numpy().reshape(ngroups, rstride)
    assert not recs[:, nvals:].any(), "pad words stay 0"
    words = seen.to_numpy()
    assert not (words >> np.uint64(nvals)).any(), "no bit past nvals"
    valid = ((words[None, :] >> np.arange(nvals, dtype=np.uint64)[:, None])
             & np.uint64(1)).astype(bool)
    kept = np.array_equal(dcodes.to_numpy(), host_codes)
    for d, h in zip(dvals, host_vals):
        kept = kept and np.array_equal(d.to_numpy(), h, equal_nan=True)
    for d, h in zip(dbits, host_bits):
        kept = kept and (d is None or np.array_equal(d.to_numpy(), h))
    for d in [dcodes, vptrs, bptrs, inits, dops, acc, seen, err] + dvals + \
            [d for d in dbits if d is not None]:
        d.free()
    return np.ascontiguousarray(recs[:, :nvals].T), valid, kept


# ---- 1. the kernel against the model ---------------------------------------
@pytest.fixture(scope="module")
def grid_rows(gpu):
    return gpu.BLOCK_THREADS * gpu.MAX_BLOCKS


@pytest.mark.parametrize("nvals", C.KERNEL_NVALS)
@pytest.mark.parametrize("n", C.KERNEL_N + ["grid+65"])
def test_kernel_matches_model(gpu, grid_rows, n, nvals):
    """n = grid + 65 is the smallest at which the grid-stride loop takes a
    second trip with a ragged tail."""
    n = grid_rows + 65 if n == "grid+65" else n
    codes, vals, masks, ops, ngroups = C.kernel_case(n, nvals)
    acc, valid, kept = _run_kernel(gpu, codes, vals, masks, ops, ngroups,
                                   pad_rows=(-n) % 64 + 64)
    _check((acc, valid), C.aggregate(codes, vals, masks, ops, ngroups), ops)
    assert kept, "input buffers unchanged"
    assert not valid[0, min(1, ngroups - 1)], "the all-NULL group"


def test_kernel_code_out_of_range_writes_nothing(gpu):
    """A code >= ncodes sets bit 4 of the error word and reaches neither
    the records nor seen (the records here end at ncodes)."""
    shim = gpu
    codes = shim.DevColumn.from_numpy(np.array([0, 2, 1], dtype=np.uint32))
    val = shim.DevColumn.from_numpy(np.array([1.0, 2.0, 4.0]))
    vptrs = shim.DevColumn.from_numpy(np.array([val.ptr.value],
                                               dtype=np.uint64))
    bptrs = shim.DevColumn.from_numpy(np.zeros(1, dtype=np.uint64))
    acc = shim.DevColumn.from_numpy(np.zeros(4))
    seen = shim.DevColumn.from_numpy(np.zeros(4, dtype=np.uint64))
    err = shim.DevColumn.from_numpy(np.zeros(1, dtype=np.uint32))
    shim.call("qk_groupby_dense_acc_valid", None, shim.c_u64(3), codes.ptr,
              shim.c_u32(2), vptrs.ptr, bptrs.ptr, None, 1, 1, acc.ptr,
              seen.ptr, err.ptr)
    shim.call("qk_stream_sync", None)
    assert int(err.to_numpy(1)[0]) == 4
    assert acc.to_numpy().tolist() == [1.0, 4.0, 0.0, 0.0]
    assert seen.to_numpy().tolist() == [1, 1, 0, 0]
    for d in (codes, val, vptrs, bptrs, acc, seen, err):
        d.free()


# ---- 2. identity against NULL ----------------------------------------------
def test_identity_is_a_value_and_all_null_is_not(gpu):
    codes, vals, masks, ops, ngroups = C.identity_case()
    acc, valid, _ = _run_kernel(gpu, codes, vals, masks, ops, ngroups)
    _check((acc, valid), C.aggregate(codes, vals, masks, ops, ngroups), ops)
    assert valid[:, 0].all()
    assert acc[:, 0].tolist() == [0.0, np.inf, -np.inf], "+-inf were inputs"
    assert not valid[:, 1].any(), "every input NULL"
    assert acc[:, 1].tolist() == [0.0, np.inf, -np.inf], "identities"
    assert valid[0, 2] and acc[0, 2] == 0.0, "a SUM of zeros is 0, not NULL"


# ---- 3. seen survives batches and growth -----------------------------------
def test_seen_survives_batches_and_growth(gpu):
    from quokka_amd import ops, shim
    batches, agg_ops = C.batch_case()
    gb = ops.GroupByKeys(1, 3, agg_ops=agg_ops, expected_groups=1,
                         nullable_vals=True)
    caps = [gb.acc_cap]
    for i, (keys, vals, masks) in enumerate(batches):
        kcol = shim.DevColumn.from_numpy(keys)
        vcols = [shim.DevColumn.from_numpy(v) for v in vals]
        # host masks, device bitmaps and NullableColumns in turn
        if i == 0:
            gb.update([kcol], vcols, val_valid=masks)
        elif i == 1:
            bits = [shim.DevColumn.from_numpy(C.pack_valid(m, tail=1))
                    for m in masks]
            gb.update([kcol], vcols, val_valid=bits)
            for b in bits:
                b.free()
        else:
            ncols = [ops.NullableColumn.from_numpy(v, m)
                     for v, m in zip(vals, masks)]
            gb.update([kcol], ncols)
            for c in ncols:
                c.free()
        for c in [kcol] + vcols:
            c.free()
        if gb.acc_cap != caps[-1]:
            caps.append(gb.acc_cap)
    assert len(caps) >= 3, "the records moved at least twice: %r" % caps
    (gkeys,), sums = gb.extract()
    valid = gb.extract_vals_valid()
    gb.free()
    keys = np.concatenate([k for k, _, _ in batches])
    uniq, codes = np.unique(keys, return_inverse=True)
    vals = [np.concatenate([v[c] for _, v, _ in batches]) for c in range(3)]
    masks = [np.concatenate([m[c] for _, _, m in batches]) for c in range(3)]
    want = C.aggregate(codes, vals, masks, agg_ops, len(uniq))
    assert sorted(gkeys.tolist()) == uniq.tolist()
    at = np.searchsorted(uniq, gkeys)           # code g -> model group
    _check((sums, valid), (want[0][:, at], want[1][:, at]), agg_ops)
    for key in (C.LATE, C.EARLY):
        assert valid[:, gkeys == key].all(), key


# ---- 4. no bitmap at all; refusals -----------------------------------------
def test_nullable_table_without_bitmaps_equals_plain(gpu):
    from quokka_amd import ops, shim
    rng = np.random.default_rng(3)
    n = 5000
    keys = rng.integers(0, 300, n).astype(np.int64)
    vals = [rng.integers(-50, 51, n).astype(np.float64) for _ in range(3)]
    kcol = shim.DevColumn.from_numpy(keys)
    vcols = [shim.DevColumn.from_numpy(v) for v in vals]
    outs = []
    for kw in ({}, {"nullable_vals": True}):
        gb = ops.GroupByKeys(1, 3, agg_ops=[0, 1, 2], expected_groups=16,
                             **kw)
        gb.update([kcol], vcols, **({"val_valid": [None] * 3} if kw else {}))
        gb.update([kcol], vcols)
        (gk,), sums = gb.extract()
        order = np.argsort(gk)
        outs.append((gk[order], sums[:, order]))
        if kw:
            assert gb.extract_vals_valid().all()
            assert gb.extract_vals_valid().shape == (3, len(gk))
        gb.free()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]), "integers: exact"
    for c in [kcol] + vcols:
        c.free()


def test_val_valid_refusals(gpu):
    from quokka_amd import ops, shim
    col = shim.DevColumn.from_numpy(np.arange(4, dtype=np.int64))
    val = shim.DevColumn.from_numpy(np.ones(4))
    gb = ops.GroupByKeys(1, 1)
    with pytest.raises(TypeError, match="nullable_vals=True"):
        gb.update([col], [val], 4, val_valid=[np.ones(4, dtype=bool)])
    nval = ops.NullableColumn.from_numpy(np.ones(4), np.ones(4, dtype=bool))
    with pytest.raises(TypeError, match="nullable_vals=True"):
        gb.update([col], [nval], 4)
    with pytest.raises(TypeError, match="nullable_vals=True"):
        gb.extract_vals_valid()
    assert gb.n_groups == 0, "refused before any device work"
    gb.free()
    with pytest.raises(ValueError, match="64"):
        ops.GroupByKeys(1, 65, nullable_vals=True)
    ops.GroupByKeys(1, 65).free()
    gb = ops.GroupByKeys(1, 64, nullable_vals=True)
    gb.update([col], [val] * 64, 4,
              val_valid=[None] * 63 + [np.array([1, 0, 1, 1], dtype=bool)])
    valid = gb.extract_vals_valid()
    assert valid[:63].all() and int(valid[63].sum()) == 3, "bit 63"
    gb.free()
    for c in (col, val, nval):
        c.free()


# ---- 5. GPUAggExecutor(device_keys=True, null_values=True) ------------------
def _check_agg(got, want, keys):
    order = [(k, "ascending") for k in keys]
    g, w = got.sort_by(order), want.sort_by(order)
    assert g.num_rows == w.num_rows
    for k in keys:
        assert g.column(k).combine_chunks().equals(
            w.column(k).combine_chunks()), k
    for alias, rtol in (("sa", 1e-9), ("lo", 0), ("hi", 0), ("r", 1e-9)):
        gc, wc = g.column(alias).combine_chunks(), \
            w.column(alias).combine_chunks()
        assert gc.type == pa.float64(), alias
        assert gc.is_valid().equals(wc.is_valid()), alias
        np.testing.assert_allclose(
            np.asarray(gc.fill_null(0.0)),
            np.asarray(wc.fill_null(0)).astype(np.float64), rtol=rtol,
            atol=0, err_msg=alias)


@pytest.mark.parametrize("null_keys", [False, True])
def test_agg_executor_null_values_vs_acero(gpu, null_keys):
    from quokka_amd.executors import GPUAggExecutor
    t = C.agg_table(null_keys)
    keys = ["ki", "ks"]
    assert t.column("a").null_count and t.column("b").null_count
    assert not t.column("c").null_count
    assert pa.types.is_int64(t.column("b").type)
    assert min(v for v in t.column("b").to_pylist() if v is not None) > 2**31
    if null_keys:
        assert t.column("ki").null_count and t.column("ks").null_count
    ex = GPUAggExecutor(keys, None, C.AGG_SQL, device_keys=True,
                        null_values=True, null_keys=null_keys)
    for lo, hi in C.AGG_BATCHES:
        ex.execute([t.slice(lo, hi - lo)], 0, 0)
    out = ex.done(0)
    want = C.agg_want(t, keys)
    assert 45 <= want.num_rows <= 80
    assert want.column("sa").null_count >= 1, "a group all-NULL in a"
    assert want.column("lo").null_count >= 1, "a group all-NULL in b"
    assert want.column("r").null_count == want.column("sa").null_count
    _check_agg(out, want, keys)


def test_agg_executor_order_by_null_alias_last(gpu):
    from quokka_amd.executors import GPUAggExecutor
    t = C.agg_table()
    ex = GPUAggExecutor(["ki", "ks"], [("sa", "desc")], C.AGG_SQL,
                        device_keys=True, null_values=True)
    for lo, hi in C.AGG_BATCHES:
        ex.execute([t.slice(lo, hi - lo)], 0, 0)
    out = ex.done(0)
    _check_agg(out, C.agg_want(t, ["ki", "ks"]), ["ki", "ks"])
    sa = out.column("sa").to_pylist()
    k = out.column("sa").null_count
    assert k >= 1 and sa[-k:] == [None] * k, "NULLs last"
    head = sa[:-k]
    assert None not in head and head == sorted(head, reverse=True)


# ---- 6. grand aggregate -----------------------------------------------------
def test_grand_aggregate_null_values(gpu):
    import pyarrow.compute as pc
    from quokka_amd.executors import GPUAggExecutor
    t = C.agg_table()
    t = t.append_column("z", pa.nulls(t.num_rows, pa.float64()))
    ex = GPUAggExecutor([], None, "sum(a) as sa, min(b) as lo, max(b) as hi, "
                        "sum(a) / sum(c) as r, max(z) as mz, "
                        "sum(c) + sum(z) as cz", null_values=True)
    for lo, hi in C.AGG_BATCHES:
        ex.execute([t.slice(lo, hi - lo)], 0, 0)
    out = ex.done(0)
    assert out.num_rows == 1
    sa, sc = pc.sum(t.column("a")).as_py(), pc.sum(t.column("c")).as_py()
    row = {c: out.column(c).to_pylist()[0] for c in out.column_names}
    assert row["sa"] == pytest.approx(sa, rel=1e-9)
    assert row["lo"] == float(pc.min(t.column("b")).as_py())
    assert row["hi"] == float(pc.max(t.column("b")).as_py())
    assert row["r"] == pytest.approx(sa / sc, rel=1e-9)
    assert row["mz"] is None and row["cz"] is None, "all-NULL column"
    assert out.column("mz").type == pa.float64()


# ---- 7. left join, then aggregate -------------------------------------------
def test_left_join_feeds_the_aggregate(gpu):
    from quokka_amd.executors import (GPUAggExecutor,
                                      GPUBuildProbeJoinExecutor)
    build = pa.table({"k": pa.array([10, 10, 30, 50, 50, 50],
                                    type=pa.int64()),
                      "pay": pa.array([1.0, 2.0, 8.0, 16.0, -32.0, 64.0])})
    probe = pa.table({"k": pa.array([10, 20, 30, 40, 50], type=pa.int64())})
    join = GPUBuildProbeJoinExecutor(on="k", how="left")
    join.execute([build], 1, 0)
    joined = join.execute([probe], 0, 0)
    assert joined.column("pay").null_count == 2
    ex = GPUAggExecutor(["k"], [("k", "asc")],
                        "sum(pay) as s, max(pay) as m", device_keys=True,
                        null_values=True)
    ex.execute([joined], 0, 0)
    out = ex.done(0)
    want = probe.join(build, "k", join_type="left outer", use_threads=False
                      ).group_by(["k"], use_threads=False).aggregate(
        [("pay", "sum"), ("pay", "max")]).sort_by("k")
    assert out.column("k").to_pylist() == [10, 20, 30, 40, 50]
    assert out.column("s").to_pylist() == want.column("pay_sum").to_pylist()
    assert out.column("m").to_pylist() == want.column("pay_max").to_pylist()
    assert out.column("s").to_pylist() == [3.0, None, 8.0, None, 48.0]
    assert out.column("m").to_pylist() == [2.0, None, 8.0, None, 64.0]
