"""Adversarial keys and pass counts for the generic operators: radix sort,
hash join, i64 group-by, hash and range partition.

Every case compares the device result with a plain Python / numpy
reference (tests/_key_cases.py), exactly: sorts against np.sort /
np.argsort(kind="stable"), joins against a dict of lists, group-bys over
integer-valued doubles with ==. The sweep threshold T (rows above which a
sort or partition-scatter block loops over several tiles) comes from the
library, and the collision clusters that wrap the table end assert the
slots they occupy, so a change of the hash or the probe sequence fails
loudly instead of silently losing the adversarial property."""
import ctypes
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _key_cases as K  # noqa: E402

from quokka_amd import ops, shim  # noqa: E402
from quokka_amd.shim import DevBuffer, DevColumn, c_u32, c_u64  # noqa: E402

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = K.I64_MIN, K.I64_MAX
U64_MAX = K.M64
# rows of one full single-tile grid: above it blocks loop over tiles
T = shim.BLOCK_THREADS * shim.MAX_BLOCKS


@pytest.fixture(scope="module")
def gpu():
    shim.init(0)
    return shim


def dev(arr, dtype=None):
    return DevColumn.from_numpy(np.ascontiguousarray(arr, dtype=dtype))


def i64(vals):
    return np.array(vals, dtype=np.int64)


# ---- sort ------------------------------------------------------------------

def sort_pairs(keys, npasses=-1):
    """qk_sort_pairs_u64 on a copy of `keys` with an iota payload ->
    (sorted keys, payload). The scratch buffers start as whatever the
    allocator hands out."""
    n = len(keys)
    k = dev(keys, np.uint64)
    p = dev(np.arange(n, dtype=np.uint32))
    kt, pt = DevColumn(np.uint64, n), DevColumn(np.uint32, n)
    shim.call("qk_sort_pairs_u64", None, c_u64(n), k.ptr, p.ptr, kt.ptr,
              pt.ptr, int(npasses))
    shim.call("qk_stream_sync", None)
    out = k.to_numpy(n), p.to_numpy(n)
    for c in (k, p, kt, pt):
        c.free()
    return out


def check_sort(keys, npasses=-1):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    got_k, got_p = sort_pairs(keys, npasses)
    assert np.array_equal(got_k, np.sort(keys))
    assert np.array_equal(got_p, np.argsort(keys, kind="stable"))


# max key M -> passes the library derives (one per non-zero byte position)
PASS_CASES = [(0, 1), (1, 1), (255, 1), (256, 2), (65535, 2), (65536, 3),
              ((1 << 24) - 1, 3), (1 << 24, 4), ((1 << 56) - 1, 7),
              (1 << 56, 8), (U64_MAX, 8)]


@pytest.mark.parametrize("M,passes", PASS_CASES)
def test_sort_pass_count_boundaries(gpu, M, passes):
    """Keys in [0, M] with M present; odd counts end in the scratch
    buffers and take the copy-back."""
    assert max(1, (M.bit_length() + 7) // 8) == passes
    rng = np.random.default_rng(M % 9973)
    keys = rng.integers(0, M, 1000, dtype=np.uint64, endpoint=True)
    keys[500] = M
    check_sort(keys)


def test_sort_explicit_npasses(gpu):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 24, 1000, dtype=np.uint64)
    keys[7] = (1 << 24) - 1
    want = sort_pairs(keys, -1)
    for npasses in (3, 8):
        got = sort_pairs(keys, npasses)
        assert np.array_equal(got[0], want[0]), npasses
        assert np.array_equal(got[1], want[1]), npasses
    check_sort(keys, 3)
    check_sort(keys, 8)


SORT_SIZES = [2, 63, 64, 65, 255, 256, 257, 511, 512, 513,
              T - 1, T, T + 1, 2 * T + 7]


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_sizes(gpu, n):
    """Up to T rows one tile per block; above it the LDS cursors carry
    over from tile to tile. Heavy duplicates check stability."""
    rng = np.random.default_rng(n)
    check_sort(rng.integers(0, 4, n, dtype=np.uint64))
    check_sort(rng.integers(0, U64_MAX, n, dtype=np.uint64, endpoint=True))


@pytest.mark.parametrize("n", [257, T + 1])
def test_sort_real_digit_255_keys_in_a_partial_tile(gpu, n):
    """The padded lanes of a partial tile carry key ~0; real ~0 keys next
    to them must keep their rows."""
    got_k, got_p = sort_pairs(np.full(n, U64_MAX, dtype=np.uint64))
    assert np.all(got_k == np.uint64(U64_MAX))
    assert np.array_equal(got_p, np.arange(n, dtype=np.uint32))


def check_sort_permutation(vals, want_asc, want_desc):
    col = dev(vals)
    for desc, want in ((False, want_asc), (True, want_desc)):
        perm = ops.sort_permutation(col, descending=desc)
        got = perm.to_numpy(perm.n)
        perm.free()
        want = np.asarray(want, dtype=np.uint32)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (
            "descending=%s: first difference at position %d: row %d (%r) "
            "where row %d (%r) belongs"
            % (desc, bad[0], got[bad[0]], vals[got[bad[0]]], want[bad[0]],
               vals[want[bad[0]]]))
    col.free()


def int_sort_refs(vals):
    lst = [int(v) for v in vals]
    asc = sorted(range(len(lst)), key=lst.__getitem__)
    desc = sorted(range(len(lst)), key=lst.__getitem__, reverse=True)
    return asc, desc


def test_sort_permutation_odd_pass_count(gpu):
    """INT64_MIN + r maps to r < 2^24: three passes, copy-back."""
    rng = np.random.default_rng(6)
    vals = i64(I64_MIN) + rng.integers(0, 70000, 5000).astype(np.int64)
    asc, desc = int_sort_refs(vals)
    assert np.array_equal(asc, np.argsort(vals, kind="stable"))
    check_sort_permutation(vals, asc, desc)


def test_sort_permutation_i64_extremes(gpu):
    rng = np.random.default_rng(7)
    pool = i64([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX])
    vals = pool[rng.integers(0, len(pool), 600)]
    vals[:6] = pool
    check_sort_permutation(vals, *int_sort_refs(vals))


def test_sort_permutation_f64_specials(gpu):
    """Every NaN, of either sign and any payload, sorts last ascending and
    first descending, stable among themselves; -0.0 < +0.0.

    On the parent commit's kernel the sign-bit-set NaNs (0xFFF8..., all
    ones) sorted before -inf ascending and last descending."""
    vals = K.f64_specials(3000, 8)
    check_sort_permutation(vals, K.f64_sort_reference(vals),
                           K.f64_sort_reference(vals, descending=True))


# ---- join ------------------------------------------------------------------

class RawJoinTable:
    """The join table as JoinTable.__init__ prepares it, with cap and the
    chain length chosen by the test; build/probe call the C ABI directly."""

    def __init__(self, cap, chain_cap):
        self.cap = cap
        self.slot_keys = DevColumn(np.int64, cap)
        self.slot_head = DevColumn(np.int32, cap)
        self.chain_cap = chain_cap
        self.chain_next = DevColumn(np.int32, chain_cap)
        shim.call("qk_fill_i64", None, self.slot_keys.ptr,
                  ctypes.c_int64(I64_MIN), c_u64(cap))
        shim.call("qk_dmemset", self.slot_head.ptr, 0xFF, c_u64(cap * 4))

    def build(self, keys, row_offset):
        keys = i64(keys)
        assert row_offset + len(keys) <= self.chain_cap
        kc = dev(keys)
        shim.call("qk_join_build", None, c_u64(len(keys)), kc.ptr,
                  c_u32(row_offset), self.slot_keys.ptr, self.slot_head.ptr,
                  self.chain_next.ptr, c_u64(self.cap))
        shim.call("qk_stream_sync", None)
        kc.free()

    def probe(self, keys, mode, out_cap):
        keys = i64(keys)
        kc = dev(keys)
        pidx = DevColumn(np.uint32, out_cap)
        bidx = DevColumn(np.uint32, out_cap) if mode == 0 else None
        cur = ops._count_buf()
        shim.call("qk_join_probe", None, c_u64(len(keys)), kc.ptr,
                  self.slot_keys.ptr, self.slot_head.ptr,
                  self.chain_next.ptr, c_u64(self.cap), mode, pidx.ptr,
                  bidx.ptr if bidx else None, c_u64(out_cap), cur.ptr)
        total = ops._read_u64(cur)
        assert total <= out_cap
        p = pidx.to_numpy(total).tolist()
        b = bidx.to_numpy(total).tolist() if bidx else None
        for c in (kc, pidx, bidx, cur):
            if c is not None:
                c.free()
        return p, b

    def occupied(self):
        sk = self.slot_keys.to_numpy(self.cap)
        slots = np.nonzero(sk != I64_MIN)[0]
        return set(slots.tolist()), sk

    def free(self):
        for c in (self.slot_keys, self.slot_head, self.chain_next):
            c.free()


def check_join_all_modes(table, build_keys, probe_keys):
    inner, semi, anti = K.join_reference(build_keys, probe_keys)
    out_cap = len(inner) + len(probe_keys) + 16
    p, b = table.probe(probe_keys, 0, out_cap)
    assert sorted(zip(p, b)) == inner
    p, _ = table.probe(probe_keys, 1, out_cap)
    assert len(p) == len(semi) and set(p) == semi
    p, _ = table.probe(probe_keys, 2, out_cap)
    assert len(p) == len(anti) and set(p) == anti


WRAP_SLOTS = {62, 63} | set(range(18))


@pytest.mark.parametrize("dup", [1, 3])
def test_join_cluster_wrapping_the_table_end(gpu, dup):
    """20 keys homed at slot 62 of 64: the cluster runs 62, 63, 0..17.
    Absent cluster keys walk the whole wrap before they miss. dup=3 puts a
    chain of three rows behind every slot of the cluster."""
    cap = 64
    cluster = K.cluster_keys(cap, 62, 20)
    rng = np.random.default_rng(20 + dup)
    build = i64(cluster * dup)[rng.permutation(20 * dup)]
    t = RawJoinTable(cap, len(build))
    t.build(build, 0)
    slots, sk = t.occupied()
    assert slots == WRAP_SLOTS == K.linear_probe_slots(cluster, cap)
    assert sorted(sk[sorted(slots)].tolist()) == sorted(cluster)
    absent = K.cluster_keys(cap, 62, 10, start=1000)
    assert not set(absent) & set(cluster)
    unrelated = [k for k in rng.integers(-10**12, 10**12, 40).tolist()
                 if k not in cluster][:10]
    probe = i64(cluster + absent + unrelated)[rng.permutation(40)]
    check_join_all_modes(t, build, probe)
    t.free()


def test_join_key_extremes(gpu):
    """A probe for INT64_MIN (the empty marker) stops at the first free
    slot, whose head is -1: absent from inner and semi, present in anti."""
    pool = [I64_MIN + 1, -1, 0, 1, I64_MAX]
    rng = np.random.default_rng(31)
    build = i64(pool * 4)[rng.permutation(20)]
    probe = i64(pool * 3 + [I64_MIN, I64_MIN, 2, -2, I64_MAX - 1])
    probe = probe[rng.permutation(len(probe))]
    t = RawJoinTable(64, len(build))
    t.build(build, 0)
    check_join_all_modes(t, build, probe)
    inner, semi, anti = K.join_reference(build, probe)
    sentinel_rows = set(np.nonzero(probe == I64_MIN)[0].tolist())
    assert len(sentinel_rows) == 2 and sentinel_rows <= anti
    assert not sentinel_rows & semi
    t.free()


def test_join_build_in_three_calls(gpu):
    """build_row_offset: chains index the concatenated build side."""
    rng = np.random.default_rng(32)
    parts = [rng.integers(-40, 40, n).astype(np.int64)
             for n in (1, 255, 300)]
    allk = np.concatenate(parts)
    t = RawJoinTable(2048, len(allk))
    off = 0
    for part in parts:
        t.build(part, off)
        off += len(part)
    probe = rng.integers(-50, 50, 400).astype(np.int64)
    check_join_all_modes(t, allk, probe)
    t.free()


def test_join_table_exactly_half_load(gpu):
    rng = np.random.default_rng(33)
    keys = rng.permutation(np.arange(-512, 512, dtype=np.int64) * 7919)
    t = ops.JoinTable(1024)
    assert t.cap // 2 == 1024
    kc = dev(keys)
    t.build(kc)                                   # n == cap // 2: allowed
    one = dev(i64([5]))
    with pytest.raises(RuntimeError, match="JoinTable overflow"):
        t.build(one)
    probe = np.concatenate([keys, keys + 1])
    pc = dev(probe)
    pidx, bidx, nm = t.probe(pc, mode=0)
    got = sorted(zip(pidx.to_numpy(nm).tolist(), bidx.to_numpy(nm).tolist()))
    assert got == K.join_reference(keys, probe)[0]
    assert nm == 1024
    for c in (kc, one, pc, pidx, bidx):
        c.free()
    t.free()


def _tbl(**cols):
    return pa.table({k: pa.array(np.asarray(v)) for k, v in cols.items()})


def test_join_executor_sentinel_and_neighbour(gpu):
    from quokka_amd import GPUBuildProbeJoinExecutor
    bad = GPUBuildProbeJoinExecutor(on="k", how="inner")
    bad.execute([_tbl(k=i64([1, I64_MIN]), b=np.array([1.0, 2.0]))], 1, 0)
    with pytest.raises(ValueError, match="INT64_MIN"):
        bad.execute([_tbl(k=i64([1]), p=np.array([1.0]))], 0, 0)

    ex = GPUBuildProbeJoinExecutor(on="k", how="inner")
    ex.execute([_tbl(k=i64([I64_MIN + 1, 5, 5, 9]),
                     b=np.array([10.0, 20.0, 30.0, 40.0]))], 1, 0)
    # probe keys are not rejected: INT64_MIN simply finds no match
    out = ex.execute([_tbl(k=i64([5, I64_MIN + 1, I64_MIN, 7]),
                           p=np.array([1.0, 2.0, 3.0, 4.0]))], 0, 0)
    got = sorted(zip(out.column("k").to_pylist(),
                     out.column("p").to_pylist(),
                     out.column("b").to_pylist()))
    assert got == [(I64_MIN + 1, 2.0, 10.0), (5, 1.0, 20.0), (5, 1.0, 30.0)]


# ---- group-by --------------------------------------------------------------

def gb_table_slots(gb):
    tab = gb.table.to_numpy(gb.cap * gb.rstride).reshape(gb.cap, gb.rstride)
    slots = np.nonzero(tab[:, 0] != I64_MIN)[0]
    return set(slots.tolist()), tab[:, 0]


def gb_update(gb, keys, vals, **kw):
    kc = dev(i64(keys))
    vcs = [dev(v, np.float64) for v in vals]
    gb.update(kc, vcs, **kw)
    kc.free()
    for v in vcs:
        v.free()


def assert_groups_equal(got, want, nvals):
    """got = (keys, sums) of extract(); want = {key: [agg...]}; exact."""
    gk, gs = got
    assert len(gk) == len(set(gk.tolist())) == len(want)
    assert set(gk.tolist()) == set(want)
    for j, k in enumerate(gk.tolist()):
        for c in range(nvals):
            assert gs[c][j] == want[k][c], (k, c, gs[c][j], want[k][c])


def cluster_rows(rng, cluster):
    """Each cluster key 1 to 50 times, shuffled."""
    reps = rng.integers(1, 51, len(cluster))
    reps[0], reps[1] = 1, 50
    keys = np.repeat(i64(cluster), reps)
    return keys[rng.permutation(len(keys))]


@pytest.mark.parametrize("nvals", [3, 7, 15])
def test_groupby_cluster_wrapping_the_table_end(gpu, nvals):
    """20 groups homed at slot 62 of 64 (records 62, 63, 0..17); nvals 7
    and 15 give record strides 8 and 16."""
    cluster = K.cluster_keys(64, 62, 20)
    rng = np.random.default_rng(40 + nvals)
    keys = cluster_rows(rng, cluster)
    agg_ops = [c % 3 for c in range(nvals)]               # SUM, MIN, MAX, ...
    vals = [rng.integers(-1000, 1000, len(keys)).astype(np.float64)
            for _ in range(nvals)]
    gb = ops.GroupByI64(32, nvals, agg_ops=agg_ops)
    assert gb.cap == 64 and gb.rstride == {3: 4, 7: 8, 15: 16}[nvals]
    gb_update(gb, keys, vals, max_new_groups=20)
    assert gb.cap == 64                                   # did not grow
    slots, slot_keys = gb_table_slots(gb)
    assert slots == WRAP_SLOTS
    assert sorted(slot_keys[sorted(slots)].tolist()) == sorted(cluster)
    assert gb.n_groups == 20
    assert_groups_equal(gb.extract(), K.groupby_reference(keys, vals,
                                                          agg_ops), nvals)
    gb.free()


def test_groupby_one_hot_key(gpu):
    n = 100_000
    keys = np.full(n, I64_MAX, dtype=np.int64)
    ones = np.ones(n)
    mod = (np.arange(n) % 1000).astype(np.float64)
    gb = ops.GroupByI64(16, 3, agg_ops=[0, 1, 2])
    gb_update(gb, keys, [ones, mod, mod])
    assert gb.n_groups == 1
    gk, gs = gb.extract()
    assert gk.tolist() == [I64_MAX]
    assert gs[0][0] == 100_000.0 and gs[1][0] == 0.0 and gs[2][0] == 999.0
    gb.free()


@pytest.mark.parametrize("n", [1, 64, 257, 5000])
def test_groupby_n_inserted_is_exact(gpu, n):
    rng = np.random.default_rng(50 + n)
    gb = ops.GroupByI64(16, 1)
    seen = set()
    allk, allv = [], []
    for _ in range(3):
        keys = rng.integers(-n, n, n).astype(np.int64)
        vals = rng.integers(0, 100, n).astype(np.float64)
        gb_update(gb, keys, [vals])
        seen |= set(keys.tolist())
        allk.append(keys)
        allv.append(vals)
        assert gb.n_groups == len(seen)
    allk, allv = np.concatenate(allk), np.concatenate(allv)
    assert_groups_equal(gb.extract(),
                        K.groupby_reference(allk, [allv], [0]), 1)
    gb.free()


def test_groupby_growth_keeps_everything(gpu):
    """From 16 slots through several rebuilds; the first batch holds a
    cluster built for the first capacity, wrapping its end."""
    rng = np.random.default_rng(60)
    agg_ops = [1, 2, 0]
    gb = ops.GroupByI64(8, 3, agg_ops=agg_ops)
    assert gb.cap == 16
    cluster = K.cluster_keys(16, 15, 6)
    assert K.linear_probe_slots(cluster, 16) == {15, 0, 1, 2, 3, 4}
    pool = np.concatenate([i64(cluster), i64([I64_MAX, I64_MIN + 1, -1]),
                           rng.integers(-10**15, 10**15, 3991)])
    assert len(set(pool.tolist())) == 4000
    batches = [np.concatenate([i64(cluster), i64(cluster[:3])]),
               pool[rng.integers(0, 300, 700)],
               np.concatenate([pool, pool[rng.integers(0, 4000, 2000)]])]
    allk, allv = [], [[], [], []]
    for b, keys in enumerate(batches):
        vals = [rng.integers(-500, 500, len(keys)).astype(np.float64)
                for _ in range(3)]
        if b == 0:
            # the known bound keeps the first batch in the 16-slot table
            gb_update(gb, keys, vals, max_new_groups=6)
            assert gb.cap == 16
            assert gb_table_slots(gb)[0] == {15, 0, 1, 2, 3, 4}
        else:
            gb_update(gb, keys, vals)
        allk.append(keys)
        for c in range(3):
            allv[c].append(vals[c])
        assert gb.n_groups == len(set(np.concatenate(allk).tolist()))
    assert gb.cap > 16 and gb.n_groups == 4000
    allk = np.concatenate(allk)
    allv = [np.concatenate(v) for v in allv]
    assert_groups_equal(gb.extract(),
                        K.groupby_reference(allk, allv, agg_ops), 3)
    gb.free()


def test_groupby_min_max_identities_and_specials(gpu):
    inf = float("inf")
    #        key  SUM   MIN    MAX
    rows = [(1, 2.0, inf, -inf),      # group 1: only +inf / only -inf
            (1, 3.0, inf, -inf),
            (2, 5.0, -inf, inf),      # group 2: both infinities
            (2, 0.0, inf, -inf),
            (2, -1.0, 7.0, 7.0),
            (3, 4.0, 4.0, 4.0),       # group 3: ties
            (3, 1.0, 4.0, 4.0),
            (3, 0.0, 9.0, -9.0),
            (I64_MAX, 5.0, -0.0, 1.0),
            (-1, 6.0, 2.0, 2.0)]
    keys = i64([r[0] for r in rows])
    vals = [np.array([r[c] for r in rows]) for c in (1, 2, 3)]
    agg_ops = [0, 1, 2]
    gb = ops.GroupByI64(16, 3, agg_ops=agg_ops)
    gb_update(gb, keys, vals)
    want = K.groupby_reference(keys, vals, agg_ops)
    assert want[1] == [5.0, inf, -inf] and want[2] == [4.0, -inf, inf]
    assert_groups_equal(gb.extract(), want, 3)

    # HAVING is strict: sums 5 (groups 1, 3, I64_MAX) do not pass "> 5"
    gk, gs = gb.extract_where_gt(0, 5.0, out_guess=16)
    assert gk.tolist() == [-1] and gs[:, 0].tolist() == want[-1]
    gk, _ = gb.extract_where_gt(0, 4.0, out_guess=16)
    assert set(gk.tolist()) == {1, 3, I64_MAX, -1}
    # a MAX column still at its -inf identity never qualifies
    gk, _ = gb.extract_where_gt(2, -inf, out_guess=16)
    assert set(gk.tolist()) == {2, 3, I64_MAX, -1}
    gb.free()


def test_agg_and_distinct_executors_sentinel_and_neighbour(gpu):
    from quokka_amd import GPUAggExecutor
    from quokka_amd.executors import GPUDistinctExecutor
    bad = GPUAggExecutor(["k"], None, "sum(x) as sx")
    with pytest.raises(ValueError, match="INT64_MIN"):
        bad.execute([_tbl(k=i64([0, I64_MIN]), x=np.array([1.0, 2.0]))], 0, 0)
    ex = GPUAggExecutor(["k"], [("k", "asc")], "sum(x) as sx")
    ex.execute([_tbl(k=i64([I64_MIN + 1, 5, I64_MIN + 1, I64_MAX]),
                     x=np.array([1.0, 2.0, 3.0, 4.0]))], 0, 0)
    out = ex.done(0)
    assert out.column("k").to_pylist() == [I64_MIN + 1, 5, I64_MAX]
    assert out.column("sx").to_pylist() == [4.0, 2.0, 4.0]

    bad = GPUDistinctExecutor("k")
    with pytest.raises(ValueError, match="INT64_MIN"):
        bad.execute([_tbl(k=i64([I64_MIN, 4]))], 0, 0)
    ex = GPUDistinctExecutor("k")
    a = ex.execute([_tbl(k=i64([I64_MIN + 1, 4, I64_MIN + 1, -1]))], 0, 0)
    assert a.column("k").to_pylist() == [I64_MIN + 1, 4, -1]
    b = ex.execute([_tbl(k=i64([4, I64_MAX, I64_MIN + 1, I64_MAX]))], 0, 0)
    assert b.column("k").to_pylist() == [I64_MAX]


# ---- partition -------------------------------------------------------------

def partition_keys(n, nparts, seed):
    rng = np.random.default_rng(seed)
    special = [I64_MIN, I64_MIN + 1, -nparts, -1, 0, nparts - 1, nparts,
               I64_MAX]
    keys = np.concatenate([
        i64(special),
        rng.integers(I64_MIN, 0, max(0, (n - 8) // 2), dtype=np.int64),
        rng.integers(-5 * nparts, 5 * nparts + 1, n, dtype=np.int64)])[:n]
    if n > 8:
        head = keys[:8].copy()
        keys = keys[rng.permutation(n)]
        keys[:: max(1, n // 8)][:8] = head     # specials stay, spread out
    return keys


def check_partition(keys, nparts):
    n = len(keys)
    want = np.mod(keys, nparts)                # mathematical mod, >= 0
    assert want.min() >= 0 and want.max() < nparts
    kc = dev(keys)
    offsets, idx = ops.partition_i64(kc, nparts)
    sel = idx.to_numpy(n)
    kc.free()
    idx.free()
    hist = np.bincount(want, minlength=nparts)
    assert np.array_equal(np.diff(offsets.astype(np.int64)), hist)
    assert int(offsets[0]) == 0 and int(offsets[-1]) == n
    assert np.array_equal(np.sort(sel), np.arange(n, dtype=np.uint32))
    assert np.array_equal(want[sel], np.repeat(np.arange(nparts), hist))


@pytest.mark.parametrize("n", [1, 257, T - 1, T, T + 1])
def test_hash_partition_negative_and_extreme_keys(gpu, n):
    """Above T rows a scatter block takes several tiles per chunk."""
    for nparts in (1, 2, 3, 7, 64, 511, 512):
        check_partition(partition_keys(n, nparts, n + nparts), nparts)


def test_hash_partition_all_rows_in_one_partition(gpu):
    rng = np.random.default_rng(70)
    keys = rng.integers(-10**15, 10**15, T + 1, dtype=np.int64) * 7 + 3
    assert np.all(np.mod(keys, 7) == 3)
    check_partition(keys, 7)


def test_partition_refuses_bad_nparts_without_a_launch(gpu):
    """nparts 0 (key % 0 on the device) is refused by both entry points,
    nparts 513 by the scatter; the outputs stay as they were."""
    n = 1000
    kc = dev(np.arange(n, dtype=np.int64))
    hist0 = np.full(513, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    idx0 = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    hist, cursors, idx = dev(hist0), dev(hist0), dev(idx0)
    with pytest.raises(shim.QkError, match="qk_partition_hist.nparts"):
        shim.call("qk_partition_hist", None, c_u64(n), kc.ptr, c_u32(0),
                  hist.ptr)
    for bad in (0, 513):
        with pytest.raises(shim.QkError,
                           match="qk_partition_scatter.nparts"):
            shim.call("qk_partition_scatter", None, c_u64(n), kc.ptr,
                      c_u32(bad), cursors.ptr, idx.ptr)
    shim.call("qk_stream_sync", None)
    assert np.array_equal(hist.to_numpy(), hist0)
    assert np.array_equal(cursors.to_numpy(), hist0)
    assert np.array_equal(idx.to_numpy(), idx0)
    for c in (kc, hist, cursors, idx):
        c.free()


def range_ids(keys, per_range, nparts):
    kc = dev(i64(keys))
    out = DevColumn(np.int64, len(keys))
    shim.call("qk_range_part_ids", None, c_u64(len(keys)), kc.ptr,
              ctypes.c_int64(per_range), c_u32(nparts), out.ptr)
    shim.call("qk_stream_sync", None)
    got = out.to_numpy(len(keys))
    kc.free()
    out.free()
    return got


def test_range_part_ids_extremes(gpu):
    """INT64_MIN routes to range 0 (the parent commit's key - 1 wrapped
    it to the last range)."""
    keys = [I64_MIN, I64_MIN + 1, -1, 0, 1, 10, 11, 40, 41, I64_MAX]
    want = K.range_part_reference(keys, 10, 4)
    assert want == [0, 0, 0, 0, 0, 0, 1, 3, 3, 3]
    assert range_ids(keys, 10, 4).tolist() == want


def test_range_part_ids_are_monotone_over_the_i64_range(gpu):
    rng = np.random.default_rng(80)
    keys = np.sort(np.concatenate([
        rng.integers(I64_MIN, I64_MAX, 4990, dtype=np.int64, endpoint=True),
        i64([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX, I64_MAX - 1, 2, 3,
             1 << 62])]))
    for per_range, nparts in ((10, 4), (1 << 61, 4), (I64_MAX, 2), (1, 512)):
        got = range_ids(keys, per_range, nparts)
        assert got.tolist() == K.range_part_reference(keys, per_range,
                                                      nparts)
        assert np.all(np.diff(got) >= 0)
        assert got[0] == 0
