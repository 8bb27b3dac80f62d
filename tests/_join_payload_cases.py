"""Join payloads that keep their NULLs (DESIGN.md §3a'''''): a plain-Python
host model of the left probe (JoinTable.probe(mode=3): dict of lists ->
(probe row, build row) pairs, NO_ROW for a miss) and of the optional take
(qk_take_opt_*: values, bool mask, null count), the kernel case lists, and
the executor cases the CPU and GPU tests share. The CPU tests hold the model
against pyarrow Acero on every executor case; the GPU tests hold the kernels
against the model and the executors against Acero."""
import numpy as np

I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
NO_ROW = 0xFFFFFFFF
ACERO_HOW = {"inner": "inner", "left": "left outer", "semi": "left semi",
             "anti": "left anti"}
HOWS = ("inner", "left", "semi", "anti")


def valid_nbytes(n):
    return ((int(n) + 63) // 64) * 8 + 8


def pack_valid(mask):
    """bool mask -> bitmap bytes, bits past the end 0, whole words + 8."""
    out = np.zeros(valid_nbytes(len(mask)), dtype=np.uint8)
    bits = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    out[:len(bits)] = bits
    return out


# ---- the model ------------------------------------------------------------
def probe(build_keys, build_valid, probe_keys, probe_valid, mode):
    """Model of JoinTable.probe. Keys are Python lists, the valid lists
    bools (True = valid) or None. mode 0 inner / 3 left -> sorted (probe
    row, build row) pairs, a miss in mode 3 paired once with NO_ROW;
    mode 1 semi / 2 anti -> sorted probe rows. A NULL key matches nothing
    on either side and the value under it is never looked at."""
    by_key = {}
    for b, k in enumerate(build_keys):
        if build_valid is None or build_valid[b]:
            by_key.setdefault(k, []).append(b)
    pairs, hit, miss = [], [], []
    for p, k in enumerate(probe_keys):
        ok = probe_valid is None or probe_valid[p]
        rows = by_key.get(k, []) if ok else []
        (hit if rows else miss).append(p)
        pairs += [(p, b) for b in rows]
        if mode == 3 and not rows:
            pairs.append((p, NO_ROW))
    if mode in (0, 3):
        return sorted(pairs)
    return hit if mode == 1 else miss


def take_opt(values, mask, idx):
    """Model of qk_take_opt_*: values a Python list, mask a bool list or
    None (every source row valid), idx row numbers or NO_ROW. -> (values
    with 0 under every null, bool mask, null count). The source value under
    a null is never used."""
    out, ok = [], []
    for r in idx:
        good = r != NO_ROW and (mask is None or bool(mask[r]))
        ok.append(good)
        out.append(values[r] if good else 0)
    return out, ok, len(ok) - sum(ok)


# ---- qk_take_opt_* cases ----------------------------------------------------
TAKE_DTYPES = (np.int64, np.float64, np.int32, np.uint8)
TAKE_SMALL_N = (0, 1, 63, 64, 65, 127, 128, 129)
TAKE_PATTERNS = ("none", "all", "lane0", "lane63", "last", "alternating")
TAKE_BITMAPS = ("no bitmap", "random bitmap", "gathered rows all null")
TAKE_N_SRC = 1000
# what the source holds under its nulls: the output must show 0 instead
JUNK = {np.int64: 0x5A5A5A5A5A5A5A5A, np.float64: -1234.5,
        np.int32: 0x5A5A5A5A, np.uint8: 0xA5}


def take_sizes(block_threads, max_blocks):
    """Every n_idx of the kernel tests: the wave and block edges, and one
    size at which the grid-stride loop takes a second round."""
    return list(TAKE_SMALL_N) + [
        block_threads - 1, block_threads, block_threads + 1,
        max_blocks * block_threads + 65]


def take_idx(n, pattern, rng):
    """u32 index array of n rows into TAKE_N_SRC source rows with NO_ROW
    placed by `pattern`."""
    idx = rng.integers(0, TAKE_N_SRC, n).astype(np.uint32)
    i = np.arange(n)
    sel = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool),
           "lane0": i % 64 == 0, "lane63": i % 64 == 63,
           "last": i == n - 1, "alternating": i % 2 == 1}[pattern]
    idx[sel] = NO_ROW
    return idx


def take_source(dtype, bitmap, idx, rng):
    """-> (source values with JUNK under its nulls, bool mask or None)."""
    if dtype == np.float64:
        vals = rng.standard_normal(TAKE_N_SRC)
        vals[:4] = [np.nan, -0.0, np.inf, 5e-324]
    else:
        info = np.iinfo(dtype)
        vals = rng.integers(info.min, info.max, TAKE_N_SRC, dtype=dtype,
                            endpoint=True)
        vals[:3] = [info.min, info.max, 0]
    if bitmap == "no bitmap":
        return vals, None
    if bitmap == "random bitmap":
        mask = rng.random(TAKE_N_SRC) < 0.7
    else:
        mask = np.ones(TAKE_N_SRC, dtype=bool)
        mask[idx[idx != NO_ROW]] = False
    vals[~mask] = JUNK[dtype]
    return vals, mask


# ---- probe mode 3 cases -------------------------------------------------------
def probe_sizes(block_threads, max_blocks):
    return [1, 63, 64, 65, max_blocks * block_threads + 65]


def probe_case(kind, n_probe, rng):
    """-> (build keys i64, probe keys i64, probe bool mask). Kinds: 'unique'
    build keys, 'chains' of length 1, 2 and 7, 'empty' build table. The
    probe mixes hits, misses, NULL keys (with a build key under the null)
    and the key INT64_MIN (QK_JOIN_EMPTY), which is a miss."""
    if kind == "unique":
        build = np.arange(0, 400, 2, dtype=np.int64)
    elif kind == "chains":
        build = np.concatenate([np.arange(0, 100), np.repeat(
            np.arange(100, 150), 2), np.repeat(np.arange(150, 170), 7)])
        build = rng.permutation(build).astype(np.int64)
    else:
        build = np.zeros(0, dtype=np.int64)
    keys = rng.integers(-20, 420, n_probe).astype(np.int64)
    keys[rng.random(n_probe) < 0.05] = I64_MIN
    mask = rng.random(n_probe) >= 0.15
    keys[~mask] = 150        # a chain-7 build key under the null
    return build, keys, mask


# ---- executor cases -------------------------------------------------------------
def _nullify(rng, values, frac, start=0):
    out = list(values)
    for i in range(start, len(out)):
        if rng.random() < frac:
            out[i] = None
    return out


_STRS = ["", "a", "é", "日本語", "a much longer string payload value", "b\0c"]


def _payloads(pa, rng, prefix, n, null_from):
    """The payload columns of one side: every type the flag supports, with
    the values that a pass through float64, NaT or an object array would
    damage, NULLs from row null_from on."""
    pick = rng.integers(0, 6, n)
    i64 = np.where(pick == 0, 2 ** 53 + 1, np.where(
        pick == 1, I64_MIN, np.where(pick == 2, I64_MAX, rng.integers(
            -10 ** 18, 10 ** 18, n)))).astype(np.int64)
    f64 = rng.standard_normal(n)
    f64[pick == 3] = np.nan
    f64[pick == 4] = -0.0
    cols = {
        "i64": pa.array(_nullify(rng, i64.tolist(), 0.2, null_from),
                        type=pa.int64()),
        "i32": pa.array(rng.integers(-2 ** 31, 2 ** 31 - 1, n)
                        .astype(np.int32)),
        "d32": pa.array(_nullify(rng, rng.integers(-30000, 30000, n)
                                 .tolist(), 0.2, null_from),
                        type=pa.int32()).cast(pa.date32()),
        "bool": pa.array(_nullify(rng, (rng.random(n) < 0.5).tolist(), 0.2,
                                  null_from), type=pa.bool_()),
        "f64": pa.array(_nullify(rng, f64.tolist(), 0.2, null_from),
                        type=pa.float64()),
        "str": pa.array(_nullify(rng, [_STRS[j] for j in rng.integers(
            0, len(_STRS), n)], 0.2, null_from), type=pa.string()),
    }
    return {prefix + k: v for k, v in cols.items()}


def _keys(pa, rng, n, kind, lo, hi, null_frac):
    k = rng.integers(lo, hi, n)
    if kind == "str":
        vals = ["" if v == lo else "key%d" % v for v in k.tolist()]
        return pa.array(_nullify(rng, vals, null_frac), type=pa.string())
    return pa.array(_nullify(rng, k.tolist(), null_frac), type=pa.int64())


# name -> how the tables of a case are made; every case runs with every how
EXECUTOR_CASES = {
    "int key": dict(),
    "build nulls only in the second batch": dict(build_null_from=100,
                                                 build_split=100),
    "left_on != right_on, keep left": dict(left_on="pk", right_on="bk"),
    "left_on != right_on, keep right": dict(left_on="pk", right_on="bk",
                                            key_to_keep="right"),
    "null int keys": dict(null_keys=True),
    "null string keys": dict(null_keys=True, key_kind="str"),
}


def executor_case(pa, name, seed=0):
    """-> dict(probe, build, build_batches, left_on, right_on, key_to_keep,
    null_keys). About half the probe keys are present; build keys repeat
    (chains); `pid` and `bid` number the rows of each side."""
    c = dict(EXECUTOR_CASES[name])
    rng = np.random.default_rng([seed, sorted(EXECUTOR_CASES).index(name)])
    n_probe, n_build = 300, 200
    kind = c.get("key_kind", "int")
    knull = 0.15 if c.get("null_keys") else 0.0
    left_on, right_on = c.get("left_on", "k"), c.get("right_on", "k")
    probe = {"pid": pa.array(np.arange(n_probe, dtype=np.int64)),
             left_on: _keys(pa, rng, n_probe, kind, 0, 240, knull)}
    probe.update(_payloads(pa, rng, "p_", n_probe, 0))
    build = {"bid": pa.array(np.arange(n_build, dtype=np.int64)),
             right_on: _keys(pa, rng, n_build, kind, 0, 120, knull)}
    build.update(_payloads(pa, rng, "b_", n_build,
                           c.get("build_null_from", 0)))
    build = pa.table(build)
    split = c.get("build_split")
    batches = [build] if split is None else \
        [build.slice(0, split), build.slice(split)]
    return dict(probe=pa.table(probe), build=build, build_batches=batches,
                left_on=left_on, right_on=right_on,
                key_to_keep=c.get("key_to_keep", "left"),
                null_keys=bool(c.get("null_keys")))


def output_names(probe, build, how, left_on, right_on, key_to_keep):
    """Names and order of the executor's output: the probe columns, then
    (inner, left) the build's numeric payloads, then its string payloads;
    a key renamed by key_to_keep='right' goes last."""
    import pyarrow as pa
    names = list(probe.column_names)
    if how in ("inner", "left"):
        pay = [c for c in build.column_names if c != right_on]
        is_str = {c: pa.types.is_string(build.schema.field(c).type)
                  for c in pay}
        names += [c for c in pay if not is_str[c]]
        names += [c for c in pay if is_str[c]]
    if key_to_keep == "right" and left_on != right_on:
        names.remove(left_on)
        names.append(left_on)       # renamed below
    return names


def acero_join(probe, build, how, left_on, right_on, key_to_keep="left"):
    """The expected table: pyarrow Acero's join (a NULL key matches
    nothing), columns in the executor's order and names."""
    want = probe.join(build, keys=left_on, right_keys=right_on,
                      join_type=ACERO_HOW[how], use_threads=False)
    want = want.select(output_names(probe, build, how, left_on, right_on,
                                    key_to_keep))
    if key_to_keep == "right" and left_on != right_on:
        want = want.rename_columns(
            [right_on if c == left_on else c for c in want.column_names])
    return want


def model_join(probe_t, build, how, left_on, right_on, key_to_keep="left"):
    """The same table from the model: probe() over the key lists, then
    take_opt() over every column."""
    import pyarrow as pa
    mode = {"inner": 0, "left": 3, "semi": 1, "anti": 2}[how]
    pk = probe_t.column(left_on).to_pylist()
    bk = build.column(right_on).to_pylist()
    res = probe(bk, [k is not None for k in bk], pk,
                [k is not None for k in pk], mode)
    pidx = [p for p, _ in res] if mode in (0, 3) else res
    bidx = [b for _, b in res] if mode in (0, 3) else None

    def taken(table, name, idx):
        vals = table.column(name).to_pylist()
        out, ok, _ = take_opt(vals, [v is not None for v in vals], idx)
        return pa.array([v if good else None for v, good in zip(out, ok)],
                        type=table.schema.field(name).type)
    cols = {}
    for name in output_names(probe_t, build, how, left_on, right_on,
                             key_to_keep):
        if name in probe_t.column_names:
            cols[name] = taken(probe_t, name, pidx)
        else:
            cols[name] = taken(build, name, bidx)
    out = pa.table(cols)
    if key_to_keep == "right" and left_on != right_on:
        out = out.rename_columns(
            [right_on if c == left_on else c for c in out.column_names])
    return out


def assert_tables_equal(got, want, sort_keys):
    """Schema (names, order, types) equal, then every column exact after
    sorting both on the row-id columns: NULLs in the same rows, float64 by
    bit pattern so that NaN, -0.0 and NULL stay three different things."""
    import pyarrow as pa
    assert got.schema.names == want.schema.names
    assert got.schema.types == want.schema.types, \
        list(zip(got.schema.names, got.schema.types, want.schema.types))
    assert got.num_rows == want.num_rows
    order = [(k, "ascending") for k in sort_keys if k in got.column_names]
    g, w = got.sort_by(order), want.sort_by(order)
    for name in g.column_names:
        gc, wc = g.column(name).combine_chunks(), \
            w.column(name).combine_chunks()
        gv = np.asarray(gc.is_valid())
        assert np.array_equal(gv, np.asarray(wc.is_valid())), name
        if pa.types.is_float64(gc.type):
            gb = np.asarray(gc.fill_null(0.0)).view(np.uint64)
            wb = np.asarray(wc.fill_null(0.0)).view(np.uint64)
            assert np.array_equal(gb[gv], wb[gv]), name
        else:
            assert gc.to_pylist() == wc.to_pylist(), name
