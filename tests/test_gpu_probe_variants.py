"""Every probe variant of the fused Q3 and Q5 paths at the row counts where
their code takes another path: n = 0, fewer rows than one lane takes
(1..3), one lane's group plus a tail (4, 5, 7, 8), around one block
(255..257) and several blocks with a tail (1027). Each run is compared
with a numpy group-by of the same rows.

Prices and discounts are small multiples of 1/4, so price * (1 - disc) is a
multiple of 1/16 and every sum is exact in f64 in whatever order the
atomics land: sums are compared with array_equal, not a tolerance.

The reference is computed once per module and never written to; the device
tables are built once and only their sums are reset between runs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_VALUES = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1027]
N_MAX = max(N_VALUES)
ASIA = (8, 9, 12, 18, 21)          # nationkeys of region ASIA


def _tables():
    """64 orders, 16 customers (half BUILDING, 10 of 16 in ASIA), 8
    suppliers and a 1027-row lineitem pool; tests probe its prefixes."""
    from quokka_amd import queries as DQ
    rng = np.random.default_rng(20260117)
    cust = {
        "c_custkey": np.arange(1, 17, dtype=np.int64),
        "c_mktsegment": (np.arange(16) % 2).astype(np.uint8),  # 1 = BUILDING
        "c_nationkey": np.array([8, 9, 0, 12, 18, 1, 21, 8, 2, 9, 12, 3,
                                 18, 21, 4, 5], dtype=np.int32),
    }
    dates = np.array([8700, 8800, 9130, 9131, DQ.Q3_DATE - 1, DQ.Q3_DATE,
                      9300, 8766], dtype=np.int32)
    orders = {
        "o_orderkey": 3 * np.arange(64, dtype=np.int64) + 1,
        "o_custkey": rng.integers(1, 17, 64).astype(np.int64),
        "o_orderdate": dates[np.arange(64) % len(dates)],
        "o_shippriority": np.zeros(64, np.int32),
    }
    supp = {
        "s_suppkey": np.arange(1, 9, dtype=np.int64),
        "s_nationkey": np.array([8, 9, 12, 18, 21, 8, 0, 9], dtype=np.int32),
    }
    # keys: every order key (hits, repeated many times over 1027 rows) and
    # the keys between them (misses)
    pool = np.concatenate([orders["o_orderkey"], orders["o_orderkey"] + 1])
    li = {
        "l_orderkey": rng.choice(pool, N_MAX).astype(np.int64),
        "l_suppkey": rng.integers(1, 9, N_MAX).astype(np.int64),
        "l_shipdate": (DQ.Q3_DATE + rng.integers(-1, 3, N_MAX)).astype(
            np.int32),
        "l_extendedprice": rng.integers(1, 40, N_MAX) / 4.0,
        "l_discount": rng.integers(0, 3, N_MAX) / 4.0,
    }
    return cust, orders, supp, li


def _force_head_rows(li, hit_key, hit_supp, miss_key, q3_date):
    """Rows 0..7 are fixed so that the smallest prefixes are not empty by
    luck: row 0 and 1 hit the same order (a duplicate), row 2 misses, row 3
    hits again but ships too early for Q3, rows 4..7 hit."""
    li["l_orderkey"][:8] = [hit_key, hit_key, miss_key, hit_key, hit_key,
                            hit_key, miss_key, hit_key]
    li["l_suppkey"][:8] = hit_supp
    li["l_shipdate"][:8] = q3_date + 1
    li["l_shipdate"][3] = q3_date


@pytest.fixture(scope="module")
def world():
    from quokka_amd import shim, staging, queries as DQ
    shim.init(0)
    cust, orders, supp, li = _tables()
    building = set(cust["c_custkey"][cust["c_mktsegment"] == DQ.MKT_BUILDING])
    cnat = dict(zip(cust["c_custkey"], cust["c_nationkey"]))
    snat = dict(zip(supp["s_suppkey"], supp["s_nationkey"]))
    # an order that survives BOTH builds, and a supplier of its nation
    both = [i for i in range(64)
            if orders["o_custkey"][i] in building
            and orders["o_orderdate"][i] < DQ.Q3_DATE
            and DQ.Q5_LO <= orders["o_orderdate"][i] < DQ.Q5_HI
            and cnat[orders["o_custkey"][i]] in ASIA]
    assert both, "test data: no order survives both the Q3 and Q5 builds"
    hit = both[0]
    hit_nat = cnat[orders["o_custkey"][hit]]
    hit_supp = [k for k, v in snat.items() if v == hit_nat][0]
    _force_head_rows(li, orders["o_orderkey"][hit], hit_supp,
                     orders["o_orderkey"][hit] + 1, DQ.Q3_DATE)

    q3_build = {k for k, c, d in zip(orders["o_orderkey"],
                                     orders["o_custkey"],
                                     orders["o_orderdate"])
                if c in building and d < DQ.Q3_DATE}
    q5_build = {k: cnat[c] for k, c, d in zip(orders["o_orderkey"],
                                              orders["o_custkey"],
                                              orders["o_orderdate"])
                if cnat[c] in ASIA and DQ.Q5_LO <= d < DQ.Q5_HI}
    rev = li["l_extendedprice"] * (1.0 - li["l_discount"])
    q3_row = np.array([k in q3_build for k in li["l_orderkey"]]) & \
        (li["l_shipdate"] > DQ.Q3_DATE)
    q5_nat = np.array([q5_build.get(k, -1) if q5_build.get(k, -1) == snat[s]
                       else -1
                       for k, s in zip(li["l_orderkey"], li["l_suppkey"])])
    for a in (rev, q3_row, q5_nat, *li.values()):
        a.setflags(write=False)

    ocols = staging.stage_columns(orders)
    ccols = staging.stage_columns(cust)
    scols = staging.stage_columns(supp)
    q3 = DQ.Q3Fused(ocols, ccols)
    q5 = DQ.Q5Fused(ocols, ccols, scols)
    assert q3.n_build == len(q3_build) and q5.n_build == len(q5_build)
    yield {"li": li, "rev": rev, "q3_row": q3_row, "q5_nat": q5_nat,
           "q3": q3, "q5": q5}
    q3.free()
    q5.free()
    for cs in (ocols, ccols, scols):
        for c in cs.values():
            c.free()


def _stage_prefix(li, n, names):
    """Fresh allocations, so every base pointer is allocation-aligned (the
    vector loads of the nt kernels need 16 B / 32 B alignment)."""
    from quokka_amd import staging
    return staging.stage_columns({k: li[k][:n] for k in names})


@pytest.mark.parametrize("nt", [False, True, 4])
@pytest.mark.parametrize("n", N_VALUES)
def test_q3_probe_variants(world, n, nt):
    from quokka_amd import ops
    q3 = world["q3"]
    row = world["q3_row"][:n]
    want_keys, inv = np.unique(world["li"]["l_orderkey"][:n][row],
                               return_inverse=True)
    want_sums = np.zeros(len(want_keys))
    np.add.at(want_sums, inv, world["rev"][:n][row])
    if n:
        assert len(want_keys) > 0        # the forced head rows hit

    lcols = _stage_prefix(world["li"], n, ["l_orderkey", "l_shipdate",
                                           "l_extendedprice", "l_discount"])
    mc = ops._count_buf()
    try:
        q3.reset_sums()
        q3.probe(lcols, mc, nt=nt)
        full, _ = q3.extract()
        got_matches = ops._read_u64(mc)
    finally:
        mc.free()
        for c in lcols.values():
            c.free()
    order = np.argsort(full["l_orderkey"])
    print("n=%d nt=%r groups=%d/%d matches=%d/%d"
          % (n, nt, len(order), len(want_keys), got_matches, int(row.sum())))
    assert np.array_equal(full["l_orderkey"][order], want_keys)
    assert np.array_equal(full["revenue"][order], want_sums)
    assert got_matches == int(row.sum())


@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("n", N_VALUES)
def test_q5_probe_variants(world, n, nt):
    from quokka_amd import ops, shim
    q5 = world["q5"]
    nat = world["q5_nat"][:n]
    want = np.zeros(32)
    np.add.at(want, nat[nat >= 0], world["rev"][:n][nat >= 0])
    if n:
        assert (nat >= 0).any()          # the forced head rows hit

    lcols = _stage_prefix(world["li"], n, ["l_orderkey", "l_suppkey",
                                           "l_extendedprice", "l_discount"])
    mc = ops._count_buf()
    got = np.zeros(32)
    try:
        q5.reset_sums()
        q5.probe(lcols, mc, nt=nt)
        got_matches = ops._read_u64(mc)
        shim.call("qk_d2h", got.ctypes.data_as(ctypes.c_void_p),
                  q5.out25.ptr, ctypes.c_uint64(32 * 8))
    finally:
        mc.free()
        for c in lcols.values():
            c.free()
    print("n=%d nt=%r matches=%d/%d" % (n, nt, got_matches,
                                        int((nat >= 0).sum())))
    assert np.array_equal(got, want)
    assert got_matches == int((nat >= 0).sum())
