"""Null values in the aggregate (DESIGN.md §3a''''): a pure-numpy model of
qk_groupby_dense_acc_valid (SUM / MIN / MAX skip NULLs, an aggregate that
met no value is NULL) and the case builders the CPU and GPU tests share.
The CPU tests hold the model against pyarrow Acero; the GPU tests hold the
kernel, ops.GroupByKeys and GPUAggExecutor against the model and Acero.

Values are small integers held in doubles, so a SUM is exact whatever the
order of the atomics. Under every NULL stands a value that would show in
the result if it were read: NaN under a SUM column's nulls, 1e300 under a
MAX column's and -1e300 under a MIN column's (NaN loses every comparison
and +1e300 can never win a MIN, so those two alone would hide a read
there)."""
import numpy as np

SUM, MIN, MAX = 0, 1, 2
AGG_INIT = {SUM: 0.0, MIN: np.inf, MAX: -np.inf}
JUNK = {SUM: np.nan, MIN: -1e300, MAX: 1e300}
ACERO_FN = {SUM: "sum", MIN: "min", MAX: "max"}

# rows of one grid-stride trip today (qk_block_threads() * qk_max_blocks());
# the GPU test takes the live figure from the library
GRID_ROWS = 256 * 2048


def valid_nbytes(n):
    return ((int(n) + 63) // 64) * 8 + 8


def pack_valid(mask, tail=0):
    """bool mask -> bitmap bytes, whole words + 8; every bit at an index
    >= len(mask) is `tail`."""
    n = len(mask)
    bits = np.full(valid_nbytes(n) * 8, bool(tail))
    bits[:n] = np.asarray(mask, dtype=bool)
    return np.packbits(bits, bitorder="little")


def aggregate(codes, vals, masks, ops, ngroups):
    """The model. codes: n ints < ngroups; vals: nvals f64 arrays; masks:
    nvals bool arrays (True = valid) or None; ops: nvals of SUM/MIN/MAX.
    -> (acc f64 [nvals, G], valid bool [nvals, G]): the op over the valid
    rows of each group, the op identity and False where there were none."""
    nvals = len(vals)
    acc = np.empty((nvals, ngroups), dtype=np.float64)
    valid = np.zeros((nvals, ngroups), dtype=bool)
    codes = np.asarray(codes, dtype=np.int64)
    for c, (v, m, op) in enumerate(zip(vals, masks, ops)):
        acc[c] = AGG_INIT[op]
        keep = np.ones(len(codes), dtype=bool) if m is None else m
        g, x = codes[keep], np.asarray(v, dtype=np.float64)[keep]
        if op == SUM:
            np.add.at(acc[c], g, x)
        elif op == MIN:
            np.minimum.at(acc[c], g, x)
        else:
            np.maximum.at(acc[c], g, x)
        valid[c, g] = True
    return acc, valid


def ops_for(nvals):
    return [(SUM, MIN, MAX)[c % 3] for c in range(nvals)]


# ---- kernel cases: every n against every nvals ---------------------------
KERNEL_N = [1, 63, 64, 65, 127, 129, 257]      # + GRID_ROWS + 65
KERNEL_NVALS = [1, 3, 5]
# column c is of kind c % 5: 0-pointers and real bitmaps in one call
KINDS = ("random nulls", "no bitmap", "random nulls", "all null",
         "all valid")


def kernel_case(n, nvals, seed=0):
    """-> (codes u32 [n], vals, masks, ops, ngroups). About 8 rows per
    group. A "random nulls" column is NULL at rows 0, 63, 64 and n - 1
    wherever they exist and in every row of group 1, so that group's
    aggregate is NULL (with n == 1 that is group 0)."""
    rng = np.random.default_rng(100_000 * nvals + n + seed)
    ngroups = max(1, min(n // 8, 4000))
    codes = rng.integers(0, ngroups, n).astype(np.uint32)
    ops = ops_for(nvals)
    vals, masks = [], []
    for c in range(nvals):
        v = rng.integers(-50, 51, n).astype(np.float64)
        kind = KINDS[c % 5]
        if kind == "no bitmap":
            m = None
        elif kind == "all null":
            m = np.zeros(n, dtype=bool)
        elif kind == "all valid":
            m = np.ones(n, dtype=bool)
        else:
            m = rng.random(n) > 0.3
            for r in (0, 63, 64, n - 1):
                if 0 <= r < n:
                    m[r] = False
            m[codes == min(1, ngroups - 1)] = False
        if m is not None:
            v[~m] = JUNK[ops[c]]
        vals.append(v)
        masks.append(m)
    return codes, vals, masks, ops, ngroups


def identity_case():
    """Identity against NULL, one column per op, four groups:
    group 0: its only valid MIN input is +inf, MAX -inf, SUM 0.0
    group 1: every input NULL
    group 2: valid SUM inputs all 0.0 (three of them), MIN / MAX finite
    group 3: ordinary values beside NULLs."""
    inf = np.inf
    codes = np.array([0, 0, 1, 1, 2, 2, 2, 3, 3, 3], dtype=np.uint32)
    m = np.array([1, 0, 0, 0, 1, 1, 1, 1, 0, 1], dtype=bool)
    ops = [SUM, MIN, MAX]
    s = np.array([0.0, 9, 9, 9, 0.0, 0.0, 0.0, 4, 9, 5])
    lo = np.array([inf, 9, 9, 9, 7, -2, 3, 4, 9, 5])
    hi = np.array([-inf, 9, 9, 9, 7, -2, 3, 4, 9, 5])
    vals = [s, lo, hi]
    for v, op in zip(vals, ops):
        v[~m] = JUNK[op]
    return codes, vals, [m, m.copy(), m.copy()], ops, 4


# ---- batches: seen must survive batches and growth -----------------------
LATE, EARLY = 1_000_000, 1_000_001


def batch_case():
    """Three batches of (keys i64, vals, masks) for a table that starts
    with room for one group, ops SUM / MIN / MAX over three columns.
    Group LATE is all-NULL in batches 1 and 2 and gets one value in batch
    3; group EARLY gets its value in batch 1 and only NULLs afterwards;
    batch 2 brings 300 new groups and batch 3 another 2000, so the records
    and the seen words move at least twice with both groups in them."""
    rng = np.random.default_rng(7)
    ops = [SUM, MIN, MAX]
    out = []
    for b, fresh in enumerate((2, 300, 2000)):
        base = 10_000 * b
        keys = np.concatenate([
            np.array([LATE, EARLY, LATE, EARLY], dtype=np.int64),
            rng.integers(base, base + fresh, 4 * fresh).astype(np.int64),
            np.arange(base, base + fresh, dtype=np.int64)])
        n = len(keys)
        vals = [rng.integers(-50, 51, n).astype(np.float64)
                for _ in ops]
        masks = [rng.random(n) > 0.4 for _ in ops]
        for m in masks:
            m[keys == LATE] = False
            m[keys == EARLY] = False
        if b == 0:
            for m in masks:
                m[1] = True                 # EARLY's one value
        if b == 2:
            for m in masks:
                m[2] = True                 # LATE's one value
        for v, m, op in zip(vals, masks, ops):
            v[~m] = JUNK[op]
        out.append((keys, vals, masks))
    return out, ops


# ---- executor case --------------------------------------------------------
AGG_SQL = "sum(a) as sa, min(b) as lo, max(b) as hi, sum(a) / sum(c) as r"
AGG_BATCHES = ((0, 700), (700, 701), (701, 2000))


def agg_table(null_keys=False, seed=11):
    """About 2000 rows and 50 groups over an int and a string key. a:
    float64 with nulls; b: int64 with nulls and values above 2**31; c:
    float64 >= 1 without nulls. Group (0, 's0') is all-NULL in a and group
    (1, 's1') all-NULL in b. null_keys: ~10 % nulls in both keys."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    n = 2000
    ki = rng.integers(0, 10, n).astype(np.int64)
    ks_i = rng.integers(0, 5, n)
    ks = np.array(["s%d" % i for i in ks_i], dtype=object)
    a = rng.integers(-50, 51, n).astype(np.float64)
    b = (1 << 31) + rng.integers(1, 1 << 20, n).astype(np.int64) * 4099
    c = rng.integers(1, 10, n).astype(np.float64)
    na = rng.random(n) < 0.3
    nb = rng.random(n) < 0.3
    na[(ki == 0) & (ks_i == 0)] = True
    nb[(ki == 1) & (ks_i == 1)] = True
    a[na] = np.nan
    cols = {"ki": pa.array(ki), "ks": pa.array(ks)}
    if null_keys:
        cols = {"ki": pa.array(ki, mask=rng.random(n) < 0.1),
                "ks": pa.array(ks, mask=rng.random(n) < 0.1)}
    cols.update(a=pa.array(a, mask=na), b=pa.array(b, mask=nb),
                c=pa.array(c))
    return pa.table(cols)


def agg_want(table, keys):
    """Acero's answer to AGG_SQL grouped by `keys`: columns sa, lo, hi, r
    beside the keys (r NULL where either sum is)."""
    import pyarrow.compute as pc
    w = table.group_by(keys, use_threads=False).aggregate(
        [("a", "sum"), ("b", "min"), ("b", "max"), ("c", "sum")])
    return w.append_column(
        "r", pc.divide(w.column("a_sum"), w.column("c_sum"))).rename_columns(
        [{"a_sum": "sa", "b_min": "lo", "b_max": "hi"}.get(c, c)
         for c in w.column_names] + ["r"])
