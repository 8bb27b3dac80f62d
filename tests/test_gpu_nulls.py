"""GPU tests of nullable columns: Parquet with nulls -> validity bitmap in
HBM (qk_pq_def_pages, qk_valid_expand) -> WHERE with SQL NULL semantics
(JitFilter nullable=) -> aggregates that skip nulls -> Arrow out with the
nulls intact. pyarrow's decode and Acero's filter / group_by are the
reference, as polars / DuckDB are null-transparent in the original.

Files are written with small pages (500..4500 rows) and 7001-row row
groups over 20,011 rows, so almost every page starts in the middle of a
64-row bitmap word."""
import io

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402

pytestmark = pytest.mark.gpu

N = 20_011
EDGES = [1, 63, 64, 65, 8191, 8192, 8193]       # 8192 == parquet_gpu._TILE
KINDS = ["i64", "f64", "i32", "dict_i64", "dict_str"]
PATTERNS = ["bernoulli", "blocks", "allnull", "lastnull", "none"]
FORMATS = [("NONE", "1.0"), ("NONE", "2.0"), ("SNAPPY", "1.0"),
           ("SNAPPY", "2.0"), ("GZIP", "2.0"), ("GZIP", "1.0")]


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def null_mask(pattern, n, rng):
    """True = valid."""
    if pattern == "bernoulli":          # levels come out bit-packed
        return rng.random(n) > 0.5
    if pattern == "blocks":             # RLE runs across page + word edges
        return (np.arange(n) // 777) % 2 == 0
    if pattern == "allnull":
        return np.zeros(n, dtype=bool)
    if pattern == "lastnull":
        m = np.ones(n, dtype=bool)
        m[-1] = False
        return m
    assert pattern == "none"
    return np.ones(n, dtype=bool)


def make_array(kind, n, mask, rng):
    if kind == "i64":
        return pa.array(rng.integers(-1 << 40, 1 << 40, n), mask=~mask,
                        type=pa.int64())
    if kind == "f64":
        return pa.array(rng.random(n) + 1.0, mask=~mask, type=pa.float64())
    if kind == "i32":
        return pa.array(rng.integers(1, 1 << 30, n).astype(np.int32),
                        mask=~mask, type=pa.int32())
    if kind == "dict_i64":
        return pa.array(rng.integers(1, 40, n) * 1000, mask=~mask,
                        type=pa.int64())
    assert kind == "dict_str"
    words = np.asarray(["w%02d" % i for i in range(23)], dtype=object)
    return pa.array(words[rng.integers(0, 23, n)], mask=~mask,
                    type=pa.string())


def write(table, compression="NONE", version="1.0"):
    buf = io.BytesIO()
    pq.write_table(table, buf, compression=compression,
                   data_page_version=version,
                   use_dictionary=[c for c in table.column_names
                                   if c.startswith("dict")],
                   data_page_size=2048, write_batch_size=500,
                   row_group_size=7001)
    return buf.getvalue()


def free_cols(cols):
    for c in cols.values():
        (c[0] if isinstance(c, tuple) else c).free()


def check_column(got, want, expect_nulls):
    """got: read_table(nulls='mask') entry; want: pyarrow Array."""
    from quokka_amd.ops import NullableColumn, valid_nbytes
    from quokka_amd.shim import DevColumn
    vals = None
    if isinstance(got, tuple):
        got, vals = got
    n = len(want)
    wmask = want.is_valid().to_numpy(zero_copy_only=False)
    if not expect_nulls:
        assert isinstance(got, DevColumn), type(got)
        host, mask = got.to_numpy(n), np.ones(n, dtype=bool)
    else:
        assert isinstance(got, NullableColumn), type(got)
        assert got.n == n and got.null_count == want.null_count
        assert got.valid.nbytes == valid_nbytes(n)
        host, mask = got.to_numpy(n), got.valid_to_numpy()
        assert np.array_equal(mask, wmask)
        assert not host[~mask].any()            # null slots hold 0
        # every bit at an index >= n is 0, slack included
        raw = np.empty(valid_nbytes(n), dtype=np.uint8)
        from quokka_amd import shim
        shim.call("qk_d2h", raw.ctypes.data_as(shim.c_vp), got.valid.ptr,
                  shim.c_u64(raw.nbytes))
        assert not np.unpackbits(raw, bitorder="little")[n:].any()
    if vals is not None:
        wv = np.asarray(want.to_pylist(), dtype=object)[wmask]
        assert np.array_equal(np.asarray(vals, dtype=object)[host[mask]], wv)
    else:
        wv = want.fill_null(0).to_numpy(zero_copy_only=False)
        assert host.dtype == wv.dtype
        assert np.array_equal(host[mask], wv[wmask])


@pytest.mark.parametrize("codec,version", FORMATS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_decode_matrix(gpu, pattern, codec, version):
    """All five encodings as the columns of one file per (null pattern,
    codec, page version)."""
    from quokka_amd import parquet_gpu as P
    rng = np.random.default_rng(11)
    arrays = {}
    for kind in KINDS:
        arrays[kind] = make_array(kind, N, null_mask(pattern, N, rng), rng)
    raw = write(pa.table(arrays), codec, version)
    ref = pq.read_table(io.BytesIO(raw))
    assert pq.ParquetFile(io.BytesIO(raw)).metadata.num_row_groups == 3
    cols = P.read_table(raw, nulls="mask")
    try:
        for kind in KINDS:
            check_column(cols[kind], ref.column(kind).combine_chunks(),
                         expect_nulls=pattern != "none")
    finally:
        free_cols(cols)


@pytest.mark.parametrize("n", EDGES)
def test_decode_row_count_edges(gpu, n):
    from quokka_amd import parquet_gpu as P
    rng = np.random.default_rng(n)
    mask = null_mask("bernoulli", n, rng)
    mask[-1] = False
    arr = make_array("i64", n, mask, rng)
    raw = write(pa.table({"x": arr}))
    cols = P.read_table(raw, nulls="mask")
    try:
        check_column(cols["x"], arr, expect_nulls=True)
    finally:
        free_cols(cols)


# ---- bitmap kernels against numpy ---------------------------------------

def upload_valid(mask):
    from quokka_amd import ops, shim
    bits = ops.pack_valid(mask)
    buf = shim.DevBuffer(len(bits))
    shim.call("qk_h2d", buf.ptr, bits.ctypes.data_as(shim.c_vp),
              shim.c_u64(len(bits)))
    return buf


@pytest.mark.parametrize("dtype", [np.int64, np.float64, np.int32,
                                   np.uint32])
@pytest.mark.parametrize("n", EDGES + [N, 600_001])
def test_valid_expand(gpu, n, dtype):
    """600,001 rows: more than one 256-row step per block."""
    import ctypes
    from quokka_amd.shim import DevColumn, c_u64
    rng = np.random.default_rng(n)
    for mask in (rng.random(n) > 0.5, np.zeros(n, dtype=bool),
                 np.ones(n, dtype=bool)):
        dense = rng.integers(1, 1 << 30, int(mask.sum())).astype(dtype)
        valid = upload_valid(mask)
        d = DevColumn.from_numpy(dense)
        out = DevColumn(dtype, n)
        gpu.call("qk_valid_expand", None, c_u64(n), valid.ptr, d.ptr,
                 out.ptr, ctypes.c_uint32(np.dtype(dtype).itemsize))
        want = np.zeros(n, dtype=dtype)
        want[mask] = dense
        assert np.array_equal(out.to_numpy(n), want)
        for b in (valid, d, out):
            b.free()


@pytest.mark.parametrize("n", EDGES + [N])
def test_valid_to_u8(gpu, n):
    from quokka_amd import ops
    rng = np.random.default_rng(n)
    mask = rng.random(n) > 0.3
    col = ops.NullableColumn.from_numpy(np.arange(n, dtype=np.int64), mask)
    flags = col.valid_flags()
    assert np.array_equal(flags.to_numpy(n), mask.astype(np.uint8))
    assert np.array_equal(col.valid_to_numpy(), mask)
    assert np.array_equal(col.to_numpy(n),
                          np.where(mask, np.arange(n), 0))
    flags.free()
    col.free()


@pytest.mark.parametrize("n", EDGES + [N])
def test_valid_gather(gpu, n):
    from quokka_amd import ops
    from quokka_amd.shim import DevColumn
    rng = np.random.default_rng(n)
    mask = rng.random(n) > 0.4
    mask[0] = False
    vals = rng.integers(1, 1 << 40, n)
    col = ops.NullableColumn.from_numpy(vals, mask)
    picks = [np.sort(rng.choice(n, size=max(1, n // 3), replace=False)),
             np.arange(n),
             np.nonzero(~mask)[0],              # only null rows
             np.zeros(0, dtype=np.int64)]       # nothing selected
    for sel in picks:
        idx = DevColumn.from_numpy(sel.astype(np.uint32))
        got = ops.take_nullable(col, idx, len(sel))
        assert got.n == len(sel)
        assert got.null_count == int((~mask[sel]).sum())
        assert np.array_equal(got.valid_to_numpy(), mask[sel])
        assert np.array_equal(got.to_numpy(len(sel)),
                              np.where(mask[sel], vals[sel], 0))
        arr = bridge_arrow(got)
        assert arr.null_count == got.null_count
        assert arr.equals(pa.array(vals[sel], mask=~mask[sel],
                                   type=pa.int64()))
        idx.free()
        got.free()
    col.free()


def bridge_arrow(col):
    from quokka_amd import bridge
    return bridge.column_to_arrow(col)


# ---- WHERE with SQL NULL semantics --------------------------------------

@pytest.fixture(scope="module")
def filter_data(gpu):
    from quokka_amd import staging
    rng = np.random.default_rng(5)
    a = pa.array(rng.integers(0, 12, N), mask=rng.random(N) < 0.35,
                 type=pa.int64())
    b = pa.array(np.round(rng.uniform(0, 8, N), 1), mask=rng.random(N) < 0.35,
                 type=pa.float64())
    c = pa.array(rng.integers(0, 12, N), type=pa.int64())
    table = pa.table({"a": a, "b": b, "c": c})
    cols = staging.stage_columns(table, nulls="mask")
    yield table, cols
    free_cols(cols)


SCHEMA = {"a": np.dtype(np.int64), "b": np.dtype(np.float64),
          "c": np.dtype(np.int64)}
F = pc.field
PREDICATES = [
    ("a > 5 OR b < 3", (F("a") > 5) | (F("b") < 3)),
    ("NOT (a > 5)", ~(F("a") > 5)),
    ("a IS NULL AND b IS NOT NULL", F("a").is_null() & F("b").is_valid()),
    ("a BETWEEN 3 AND 7", (F("a") >= 3) & (F("a") <= 7)),
    ("a IN (1, 4, 9)", F("a").isin([1, 4, 9])),
    ("a < c", F("a") < F("c")),
]


@pytest.mark.parametrize("sql,expr", PREDICATES,
                         ids=[p[0] for p in PREDICATES])
def test_jit_filter_three_valued(gpu, filter_data, sql, expr):
    from quokka_amd import bridge, jit, ops
    table, cols = filter_data
    assert isinstance(cols["a"], ops.NullableColumn)
    assert isinstance(cols["b"], ops.NullableColumn)
    assert not isinstance(cols["c"], ops.NullableColumn)
    want = table.filter(expr)
    f = jit.JitFilter(sql, SCHEMA, nullable=("a", "b"))
    idx, k = f.run(cols)
    assert k == want.num_rows and 0 < k < N
    taken = {name: ops.take_nullable(cols[name], idx, k) for name in cols}
    got = bridge.table_to_arrow(taken)
    for name in table.column_names:
        w = want.column(name).combine_chunks()
        g = got.column(name).combine_chunks()
        assert g.null_count == w.null_count, name
        assert g.equals(w), name
    free_cols(taken)
    idx.free()
    f.free()


def test_jit_filter_needs_nullable_columns(gpu, filter_data):
    from quokka_amd import jit
    table, cols = filter_data
    f = jit.JitFilter("c > 3 AND a > 1", SCHEMA, nullable=("a", "c"))
    with pytest.raises(TypeError, match="NullableColumn"):
        f.run(cols)                     # c was staged as a plain column
    f.free()


# ---- aggregates that skip nulls -----------------------------------------

def test_jit_aggregate_skips_nulls(gpu):
    from quokka_amd import jit, staging
    rng = np.random.default_rng(6)
    key = rng.integers(0, 4, N).astype(np.uint8)
    xmask = rng.random(N) < 0.3                  # True = null
    xmask[key == 2] = True                       # group 2: all null
    x = pa.array(np.round(rng.uniform(-50, 50, N), 3), mask=xmask,
                 type=pa.float64())
    table = pa.table({"k": pa.array(key, type=pa.uint8()), "x": x})
    cols = staging.stage_columns(table, nulls="mask")
    schema = {"k": np.dtype(np.uint8), "x": np.dtype(np.float64)}
    agg = jit.JitAggregate(
        schema, [("k", 4)],
        ["SUM(x)", "MIN(x)", "MAX(x)", "COUNT(x)", "COUNT(*)"],
        nullable=("x",))
    acc = agg.make_acc()
    agg.run(cols, acc)
    got = agg.read(acc)
    ref = table.group_by("k").aggregate(
        [("x", "sum"), ("x", "min"), ("x", "max"), ("x", "count"),
         ([], "count_all")]).sort_by("k").to_pydict()
    assert ref["k"] == [0, 1, 2, 3]
    for g in range(4):
        s, mn, mx, cnt, call = got[g]
        assert cnt == ref["x_count"][g] and call == ref["count_all"][g]
        if g == 2:
            # the documented identities, where SQL says NULL; COUNT(x)
            # tells the caller
            assert ref["x_sum"][g] is None and cnt == 0
            assert (s, mn, mx) == (0.0, np.inf, -np.inf)
            continue
        assert abs(s - ref["x_sum"][g]) <= 1e-9 * abs(ref["x_sum"][g])
        assert mn == ref["x_min"][g] and mx == ref["x_max"][g]
    acc.free()
    agg.free()
    with pytest.raises(TypeError, match="group key"):
        jit.JitAggregate(schema, [("k", 4)], ["COUNT(*)"], nullable=("k",))
    free_cols(cols)


# ---- end to end ----------------------------------------------------------

def test_parquet_filter_arrow_end_to_end(gpu):
    from quokka_amd import bridge, jit, ops, parquet_gpu as P
    rng = np.random.default_rng(8)
    a = make_array("dict_i64", N, null_mask("bernoulli", N, rng), rng)
    b = make_array("f64", N, null_mask("blocks", N, rng), rng)
    c = pa.array(rng.integers(0, 50_000, N), type=pa.int64())
    raw = write(pa.table({"dict_a": a, "b": b, "c": c}), "SNAPPY", "1.0")
    want = pq.read_table(io.BytesIO(raw)).filter(
        (F("dict_a") > 20_000) | (F("b") < 1.5) | F("b").is_null())
    cols = P.read_table(raw, nulls="mask")
    schema = {"dict_a": np.dtype(np.int64), "b": np.dtype(np.float64),
              "c": np.dtype(np.int64)}
    f = jit.JitFilter("dict_a > 20000 OR b < 1.5 OR b IS NULL", schema,
                      nullable=("dict_a", "b"))
    idx, k = f.run(cols)
    assert k == want.num_rows and 0 < k < N
    taken = {name: ops.take_nullable(cols[name], idx, k) for name in cols}
    got = bridge.table_to_arrow(taken)
    assert got.equals(want.combine_chunks())
    free_cols(taken)
    free_cols(cols)
    idx.free()
    f.free()


# ---- default mode is unchanged -------------------------------------------

@pytest.mark.parametrize("codec,version", FORMATS[:5])
def test_default_mode_still_raises_on_nulls(gpu, codec, version):
    from quokka_amd import parquet_gpu as P
    rng = np.random.default_rng(9)
    arr = make_array("i64", 3001, null_mask("bernoulli", 3001, rng), rng)
    raw = write(pa.table({"x": arr}), codec, version)
    with pytest.raises(P.QkParquetError, match="nulls"):
        P.read_table(raw)


def test_default_stage_columns_unchanged(gpu):
    """The default still turns an int64 column with nulls into float64
    with NaN."""
    from quokka_amd import staging
    from quokka_amd.shim import DevColumn
    t = pa.table({"x": pa.array([1, None, 3], type=pa.int64())})
    cols = staging.stage_columns(t)
    assert type(cols["x"]) is DevColumn
    assert cols["x"].dtype == np.dtype(np.float64)
    got = cols["x"].to_numpy(3)
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == 3.0
    free_cols(cols)
