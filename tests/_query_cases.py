"""Degenerate inputs for the 22 composed TPC-H pipelines: mutators over the
generated tables and the (query, mutator) case table. CPU only; nothing here
imports the device package.

Conventions, followed by oracle.queries, the Acero restatements and the
device pipelines alike:

* An SQL aggregate over no rows is NULL; the scalar queries (Q6, Q14, Q17,
  Q19) and the per-year shares of Q8 report it as 0.0.
* A query that returns rows returns NO rows when nothing qualifies (Q15 over
  an empty window has no winners). The fixed-domain reports are the
  exception: Q5 (the five ASIA nations), Q7 (the four nation/year cells), Q8
  (two years) and Q12 (two ship modes) always list their whole domain and a
  cell no row reached reads 0; for them "empty" means every cell is zero.
* Groups exist because a row reached them, not because their sum is
  non-zero.

Every mutator takes the dict of tables and returns a deep copy with some
columns rewritten: row counts, column sets and dtypes never change (so the
per-process JIT cache keeps hitting), dense keys stay dense, and the result
is marked read-only.

SF: 0.01 (seed 42) is the smallest of {0.01, 0.02, 0.03, 0.05} at which every
table is non-empty and all 22 oracle answers on the unmutated data are
non-empty (Q18 has exactly one qualifying order there); checked on the CPU
by test_query_cases_cpu.test_base_answers_nonempty. Q21's tie_at_limit alone
needs more than 4*100+64 suppliers and runs at SF 0.05.

Two bases: RAW is the generator's output (Q6's discount band and Q19's
quantity bands need the generator's values); EXACT rewrites prices, costs and
balances to multiples of 1/4 and discounts and taxes to {0, 1/4, 1/2}, so that
every product and sum is exact in f64 in any order and device sums can be
compared with array_equal.
"""
import numpy as np

from oracle import tpch_gen as G, queries as OQ

SF, SEED = 0.01, 42
SF_Q21_TIE = 0.05
LIMITS = {"q2": 100, "q3": 10, "q10": 20, "q18": 100, "q21": 100}
FIXED_DOMAIN = ("q5", "q7", "q8", "q12")
SCALAR = ("q6", "q14", "q17", "q19")
RAW_QUERIES = ("q6", "q19")

_BASES = {}


def _copy(d):
    return {t: ({c: (a.copy() if isinstance(a, np.ndarray) else a)
                 for c, a in cols.items()} if isinstance(cols, dict) else cols)
            for t, cols in d.items()}


def _freeze(d):
    for cols in d.values():
        if isinstance(cols, dict):
            for a in cols.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return d


def _quarter(a):
    return np.round(a * 4.0) / 4.0


def base(kind="exact", sf=SF):
    """The frozen unmutated tables: 'raw' or 'exact' (module docstring)."""
    key = (kind, sf)
    if key not in _BASES:
        d = G.gen_all(sf, SEED)
        d["customer_s"] = G.gen_customer(sf, SEED, strings=True)
        d["_sf"], d["_seed"] = sf, SEED
        if kind == "exact":
            li = d["lineitem"]
            li["l_extendedprice"] = _quarter(li["l_extendedprice"])
            li["l_discount"] = (np.round(li["l_discount"] * 100) % 3) / 4.0
            li["l_tax"] = (np.round(li["l_tax"] * 100) % 3) / 4.0
            d["partsupp"]["ps_supplycost"] = _quarter(
                d["partsupp"]["ps_supplycost"])
            d["supplier"]["s_acctbal"] = _quarter(d["supplier"]["s_acctbal"])
            d["customer"]["c_acctbal"] = _quarter(d["customer"]["c_acctbal"])
        _BASES[key] = _freeze(d)
    return _BASES[key]


# ---- the oracle's answer, and one summary shape over all 22 ---------------

def run_oracle(q, d, limit=None):
    li, od, cu, su = d["lineitem"], d["orders"], d["customer"], d["supplier"]
    pa, ps, na, re = d["part"], d["partsupp"], d["nation"], d["region"]
    kw = {} if limit is None else {"limit": limit}
    if q == "q1": return OQ.q1(li)
    if q == "q2": return OQ.q2(pa, su, ps, na, re, **kw)
    if q == "q3": return OQ.q3(li, od, cu, **kw)
    if q == "q4": return OQ.q4(li, od)
    if q == "q5": return OQ.q5(li, od, cu, su, na, re)
    if q == "q6": return OQ.q6(li)
    if q == "q7": return OQ.q7(li, od, cu, su, na)
    if q == "q8": return OQ.q8(li, od, cu, su, pa, na, re)
    if q == "q9": return OQ.q9(li, od, su, pa, ps, na)
    if q == "q10": return OQ.q10(li, od, d["customer_s"], na, **kw)
    if q == "q11": return OQ.q11(ps, su, na)
    if q == "q12": return OQ.q12(li, od)
    if q == "q13": return OQ.q13(od, cu)
    if q == "q14": return OQ.q14(li, pa)
    if q == "q15": return OQ.q15(li, su)
    if q == "q16": return OQ.q16(pa, ps, su)
    if q == "q17": return OQ.q17(li, pa)
    if q == "q18": return OQ.q18(li, od, d["customer_s"], **kw)
    if q == "q19": return OQ.q19(li, pa)
    if q == "q20": return OQ.q20(li, pa, ps, su, na)
    if q == "q21": return OQ.q21(li, od, su, na, **kw)
    if q == "q22": return OQ.q22(cu, od)
    raise KeyError(q)


def values(q, ans):
    """The answer's rows as one f64 array of their aggregated value (for the
    LIMIT queries: of their primary sort value), in output order."""
    if q == "q1": v = ans["sum_disc_price"]
    elif q == "q2": v = ans["s_acctbal"]
    elif q == "q3": v = ans[1]["revenue"]
    elif q == "q5": v = [r for _, r in ans]
    elif q == "q6": v = [ans["revenue"]] if ans["rows_passed"] else []
    elif q == "q10": v = ans["revenue"]
    elif q in ("q11", ): v = ans[1]
    elif q == "q12": v = [a + b for a, b in ans.values()]
    elif q == "q13": v = [c * n for c, n in ans.items() if c]
    elif q == "q15": v = [ans[1]] * len(ans[0])
    elif q == "q18": v = ans["o_totalprice"]
    elif q == "q20": v = np.ones(len(ans))
    elif q == "q22": v = [t for _, t in ans.values()]
    elif q in SCALAR: v = [ans]
    else: v = list(ans.values())            # q4 q7 q8 q9 q16 q21: dicts
    return np.asarray(v, dtype=np.float64)


def n_groups(q, ans):
    """Rows in the answer; for scalars and fixed-domain reports, the cells
    that hold a non-zero value."""
    v = values(q, ans)
    if q in FIXED_DOMAIN or q in SCALAR and q != "q6":
        return int(np.count_nonzero(v))
    return len(v)


def revalued(d, q=None):
    """The same rows with every contribution forced non-zero (price 1,
    discount 0, cost 0): tells 'no row arrived' from 'rows summing to 0'.
    Q6 filters on the discount and sums price * discount, so keeps it."""
    b = _copy(d)
    b["lineitem"]["l_extendedprice"][:] = 1.0
    if q != "q6":
        b["lineitem"]["l_discount"][:] = 0.0
    b["partsupp"]["ps_supplycost"][:] = 0.0
    return b


# ---- helpers for the mutators ------------------------------------------

def _orow(b, keys):
    """orders row of each (existing) order key; o_orderkey is ascending."""
    return np.searchsorted(b["orders"]["o_orderkey"], keys)


def _sides(n, lo, hi):
    """Just outside a [.., ..] window on both sides, alternating by row."""
    return np.where(np.arange(n) % 2 == 0, lo, hi).astype(np.int32)


def _q3_rows(b):
    """lineitem rows that reach Q3's aggregate."""
    full, _ = OQ.q3(b["lineitem"], b["orders"], b["customer"])
    li = b["lineitem"]
    return np.isin(li["l_orderkey"], full["l_orderkey"]) & \
        (li["l_shipdate"] > G.Q3_DATE)


def _q5_rows(b):
    li, od, cu, su = b["lineitem"], b["orders"], b["customer"], b["supplier"]
    asia = b["nation"]["n_regionkey"][cu["c_nationkey"]] == 2
    o = _orow(b, li["l_orderkey"])
    oc = od["o_custkey"][o] - 1
    return ((od["o_orderdate"][o] >= G.Q5_LO) & (od["o_orderdate"][o] < G.Q5_HI)
            & asia[oc]
            & (cu["c_nationkey"][oc] == su["s_nationkey"][li["l_suppkey"] - 1]))


def _q10_rows(b):
    li, od = b["lineitem"], b["orders"]
    o = _orow(b, li["l_orderkey"])
    return ((li["l_returnflag"] == 2) & (od["o_orderdate"][o] >= OQ.Q10_LO)
            & (od["o_orderdate"][o] < OQ.Q10_HI))


def _q7_rows(b):
    li, od, cu, su = b["lineitem"], b["orders"], b["customer"], b["supplier"]
    cn = cu["c_nationkey"][od["o_custkey"][_orow(b, li["l_orderkey"])] - 1]
    sn = su["s_nationkey"][li["l_suppkey"] - 1]
    return ((li["l_shipdate"] >= OQ.Q7_LO) & (li["l_shipdate"] <= OQ.Q7_HI)
            & (((sn == 6) & (cn == 7)) | ((sn == 7) & (cn == 6))))


def _q8_rows(b):
    li, od, cu = b["lineitem"], b["orders"], b["customer"]
    o = _orow(b, li["l_orderkey"])
    amer = b["nation"]["n_regionkey"][
        cu["c_nationkey"][od["o_custkey"][o] - 1]] == 1
    return ((b["part"]["p_type"][li["l_partkey"] - 1] == 3) & amer
            & (od["o_orderdate"][o] >= OQ.Q7_LO)
            & (od["o_orderdate"][o] <= OQ.Q7_HI))


def _q12_rows(b):
    li = b["lineitem"]
    return (np.isin(li["l_shipmode"], [2, 5])
            & (li["l_commitdate"] < li["l_receiptdate"])
            & (li["l_shipdate"] < li["l_commitdate"])
            & (li["l_receiptdate"] >= OQ.Q12_LO)
            & (li["l_receiptdate"] < OQ.Q12_HI))


def _q19_rows(b):
    li, pa = b["lineitem"], b["part"]
    p = li["l_partkey"] - 1
    m = np.zeros(len(p), dtype=bool)
    for bname, conts, qlo, qhi, slo, shi in OQ.Q19_BRANCHES:
        m |= ((pa["p_brand"][p] == G.brand_code(bname))
              & np.isin(pa["p_container"][p],
                        [G.container_code(c) for c in conts])
              & (li["l_quantity"] >= qlo) & (li["l_quantity"] <= qhi)
              & (pa["p_size"][p] >= slo) & (pa["p_size"][p] <= shi))
    return m & np.isin(li["l_shipmode"], [0, 4]) & (li["l_shipinstruct"] == 1)


def _first_per_group(keys, rows):
    """Among the row indices `rows`, the first one of each distinct key."""
    _, first = np.unique(keys[rows], return_index=True)
    return rows[first]


def _flat_groups(b, rows, keys, n_high):
    """Every group of `rows` (by `keys`) gets revenue exactly 8.0, carried by
    its first row, except the n_high smallest keys, which get 16.0."""
    li = b["lineitem"]
    li["l_discount"][rows] = 0.0
    li["l_extendedprice"][rows] = 0.0
    first = _first_per_group(keys, rows)
    li["l_extendedprice"][first] = 8.0
    li["l_extendedprice"][first[:n_high]] = 16.0


# ---- mutators, per query ----------------------------------------------

def q1_window_miss(b):
    b["lineitem"]["l_shipdate"][:] = G.Q1_CUTOFF + 1


def q1_one_survivor(b):
    q1_window_miss(b)
    b["lineitem"]["l_shipdate"][5] = G.Q1_CUTOFF         # <= is inclusive


def q1_zero_sum(b):
    for c in ("l_quantity", "l_extendedprice", "l_discount"):
        b["lineitem"][c][:] = 0.0


def q1_hot_key(b):
    b["lineitem"]["l_returnflag"][:] = 2
    b["lineitem"]["l_linestatus"][:] = 0


def q6_window_miss(b):
    li = b["lineitem"]
    li["l_shipdate"][:] = _sides(len(li["l_shipdate"]), G.Q5_LO - 1, G.Q5_HI)


def q6_one_survivor(b):
    li = b["lineitem"]
    m = ((li["l_discount"] >= 0.06 - 0.01) & (li["l_discount"] <= 0.06 + 0.01)
         & (li["l_quantity"] < 24.0))
    q6_window_miss(b)
    li["l_shipdate"][np.nonzero(m)[0][0]] = G.Q5_LO      # >= is inclusive


def q6_zero_sum(b):
    b["lineitem"]["l_extendedprice"][:] = 0.0


def q3_window_miss(b):
    b["orders"]["o_orderdate"][:] = G.Q3_DATE            # < is exclusive


def q3_join_miss(b):
    seg = b["customer"]["c_mktsegment"]
    seg[seg == 1] = 0


def q3_one_survivor(b):
    li = b["lineitem"]
    rows = np.nonzero(_q3_rows(b))[0]
    li["l_shipdate"][rows[1:]] = G.Q3_DATE               # > is exclusive


def q3_hot_key(b):
    li = b["lineitem"]
    rows = _q3_rows(b)
    key = li["l_orderkey"][np.nonzero(rows)[0][0]]
    li["l_orderkey"][li["l_shipdate"] > G.Q3_DATE] = key


def q3_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q3_tie_at_limit(b):
    rows = np.nonzero(_q3_rows(b))[0]
    _flat_groups(b, rows, b["lineitem"]["l_orderkey"], 3)


def q3_short_result(b):
    li = b["lineitem"]
    rows = np.nonzero(_q3_rows(b))[0]
    keep = np.unique(li["l_orderkey"][rows])[:4]
    li["l_shipdate"][rows[~np.isin(li["l_orderkey"][rows], keep)]] = G.Q3_DATE


def q5_window_miss(b):
    od = b["orders"]["o_orderdate"]
    od[:] = _sides(len(od), G.Q5_LO - 1, G.Q5_HI)


def q5_join_miss(b):
    b["supplier"]["s_nationkey"][:] = 0                  # ALGERIA: not ASIA


def q5_one_survivor(b):
    li = b["lineitem"]
    r = np.nonzero(_q5_rows(b))[0][0]
    key = li["l_orderkey"][r]
    q5_window_miss(b)
    b["orders"]["o_orderdate"][_orow(b, key)] = G.Q5_LO  # >= is inclusive
    other = np.nonzero(li["l_orderkey"] == key)[0]
    other = other[other != r]
    li["l_orderkey"][other] = b["orders"]["o_orderkey"][
        (_orow(b, key) + 1) % len(b["orders"]["o_orderkey"])]


def q5_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q5_hot_key(b):
    li = b["lineitem"]
    r = np.nonzero(_q5_rows(b))[0][0]
    li["l_orderkey"][:] = li["l_orderkey"][r]
    li["l_suppkey"][:] = li["l_suppkey"][r]


def q4_window_miss(b):
    od = b["orders"]["o_orderdate"]
    od[:] = _sides(len(od), OQ.Q4_LO - 1, OQ.Q4_HI)


def q4_join_miss(b):
    li = b["lineitem"]
    d = b["orders"]["o_orderdate"][_orow(b, li["l_orderkey"])]
    inw = (d >= OQ.Q4_LO) & (d < OQ.Q4_HI)
    li["l_commitdate"][inw] = li["l_receiptdate"][inw]   # < is exclusive


def q4_one_survivor(b):
    li = b["lineitem"]
    r = np.nonzero(li["l_commitdate"] < li["l_receiptdate"])[0][0]
    q4_window_miss(b)
    b["orders"]["o_orderdate"][_orow(b, li["l_orderkey"][r])] = OQ.Q4_LO


def q4_hot_key(b):
    q4_window_miss(b)
    key = b["orders"]["o_orderkey"][77]
    b["orders"]["o_orderdate"][77] = OQ.Q4_HI - 1
    b["lineitem"]["l_orderkey"][:] = key     # the build side repeats the key


def q10_window_miss(b):
    od = b["orders"]["o_orderdate"]
    od[:] = _sides(len(od), OQ.Q10_LO - 1, OQ.Q10_HI)


def q10_join_miss(b):
    b["lineitem"]["l_returnflag"][_q10_rows(b)] = 1


def q10_one_survivor(b):
    rows = np.nonzero(_q10_rows(b))[0]
    b["lineitem"]["l_returnflag"][rows[1:]] = 1


def q10_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def _q10_cust(b):
    return b["orders"]["o_custkey"][_orow(b, b["lineitem"]["l_orderkey"])]


def q10_tie_at_limit(b):
    _flat_groups(b, np.nonzero(_q10_rows(b))[0], _q10_cust(b), 5)


def q10_short_result(b):
    rows = np.nonzero(_q10_rows(b))[0]
    cust = _q10_cust(b)[rows]
    b["lineitem"]["l_returnflag"][
        rows[~np.isin(cust, np.unique(cust)[:5])]] = 1


def q10_hot_key(b):
    li = b["lineitem"]
    rows = _q10_rows(b)
    key = li["l_orderkey"][np.nonzero(rows)[0][0]]
    li["l_orderkey"][li["l_returnflag"] == 2] = key


def _orders_with_lines(b, nlines, count):
    """Keys of the first `count` orders that have exactly `nlines` lines."""
    k, c = np.unique(b["lineitem"]["l_orderkey"], return_counts=True)
    return k[c == nlines][:count]


def q18_window_miss(b):
    li = b["lineitem"]
    li["l_quantity"][:] = 1.0
    key = _orders_with_lines(b, 6, 1)[0]
    li["l_quantity"][li["l_orderkey"] == key] = 50.0     # 300: > is exclusive


def _q18_plant(b, count):
    li = b["lineitem"]
    li["l_quantity"][:] = 1.0
    keys = _orders_with_lines(b, 7, count)
    assert len(keys) == count
    li["l_quantity"][np.isin(li["l_orderkey"], keys)] = 43.0     # 301
    return keys


def q18_one_survivor(b):
    _q18_plant(b, 1)


def q18_short_result(b):
    _q18_plant(b, 5)


def q18_tie_at_limit(b):
    keys = _q18_plant(b, 500)
    tp = b["orders"]["o_totalprice"]
    rows = _orow(b, keys)
    tp[rows] = 1000.0
    tp[rows[::13]] = 2000.0                   # 39 orders above the tie


def q18_join_miss(b):
    keys = _q18_plant(b, 3)
    li = b["lineitem"]
    m = np.isin(li["l_orderkey"], keys)
    li["l_orderkey"][m] += 8                  # a hole of the sparse key space


def q18_hot_key(b):
    b["lineitem"]["l_orderkey"][:] = b["orders"]["o_orderkey"][123]


def q2_window_miss(b):
    sz = b["part"]["p_size"]
    sz[:] = np.where(np.arange(len(sz)) % 2 == 0, 14, 16)


def q2_join_miss(b):
    b["supplier"]["s_nationkey"][:] = 0       # no EUROPE supplier


def _q2_plant(b, nparts):
    pa, ps = b["part"], b["partsupp"]
    pa["p_size"][:] = 14
    pa["p_size"][:nparts] = 15
    pa["p_type"][:nparts] = 0                 # ECONOMY ANODIZED BRASS
    first = np.arange(nparts) * 4             # four ps rows per part
    b["supplier"]["s_nationkey"][ps["ps_suppkey"][first] - 1] = 6    # FRANCE
    ps["ps_supplycost"][first] = 0.25         # below the generator's minimum


def q2_one_survivor(b):
    _q2_plant(b, 1)


def q2_short_result(b):
    _q2_plant(b, 7)


def q2_tie_at_limit(b):
    b["part"]["p_size"][:] = 15
    b["part"]["p_type"][:] = 0
    b["partsupp"]["ps_supplycost"][:] = 1.0   # every EUROPE row is a minimum
    ab = b["supplier"]["s_acctbal"]
    ab[:] = 100.0
    ab[::9] = 200.0


def _q21_clear(b):
    li = b["lineitem"]
    li["l_receiptdate"][:] = li["l_commitdate"]          # > is exclusive


def q21_window_miss(b):
    _q21_clear(b)


def q21_join_miss(b):
    nk = b["supplier"]["s_nationkey"]
    nk[nk == 20] = 0                          # no SAUDI ARABIA supplier


def _q21_plant(b, nsupp, extra):
    """Supplier s (1..nsupp) is the only late supplier of one two-supplier
    F order; suppliers 1..extra of a second one."""
    _q21_clear(b)
    li, od = b["lineitem"], b["orders"]
    keys = _orders_with_lines(b, 2, nsupp + extra)
    assert len(keys) == nsupp + extra
    od["o_orderstatus"][_orow(b, keys)] = 0
    first = np.searchsorted(li["l_orderkey"], keys)      # lines are by order
    s = np.concatenate([np.arange(nsupp), np.arange(extra)]) + 1
    nall = len(b["supplier"]["s_suppkey"])
    li["l_suppkey"][first] = s
    li["l_suppkey"][first + 1] = s % nall + 1
    li["l_receiptdate"][first] = li["l_commitdate"][first] + 1
    b["supplier"]["s_nationkey"][:nsupp] = 20


def q21_one_survivor(b):
    _q21_plant(b, 1, 0)


def q21_short_result(b):
    _q21_plant(b, 5, 2)


def q21_tie_at_limit(b):
    _q21_plant(b, 480, 30)


def q7_window_miss(b):
    sd = b["lineitem"]["l_shipdate"]
    sd[:] = _sides(len(sd), OQ.Q7_LO - 1, OQ.Q7_HI + 1)


def q7_join_miss(b):
    b["supplier"]["s_nationkey"][:] = 0


def q7_one_survivor(b):
    rows = np.nonzero(_q7_rows(b))[0]
    sd = b["lineitem"]["l_shipdate"]
    sd[rows[1:]] = OQ.Q7_HI + 1
    sd[rows[0]] = OQ.Q7_HI                    # BETWEEN is inclusive


def q7_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q8_window_miss(b):
    od = b["orders"]["o_orderdate"]
    od[:] = _sides(len(od), OQ.Q7_LO - 1, OQ.Q7_HI + 1)


def q8_join_miss(b):
    t = b["part"]["p_type"]
    t[t == 3] = 4


def q8_one_survivor(b):
    li = b["lineitem"]
    rows = np.nonzero(_q8_rows(b))[0]
    other = b["part"]["p_partkey"][b["part"]["p_type"] != 3][0]
    li["l_partkey"][rows[1:]] = other
    b["supplier"]["s_nationkey"][li["l_suppkey"][rows[0]] - 1] = 2   # BRAZIL


def q8_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q9_window_miss(b):
    b["part"]["p_name_green"][:] = 0


def q9_join_miss(b):
    """Green lines whose (part, supplier) pair is not in partsupp."""
    li, ps = b["lineitem"], b["partsupp"]
    S = len(b["supplier"]["s_suppkey"]) + 1
    have = ps["ps_partkey"] * S + ps["ps_suppkey"]
    rows = np.nonzero(b["part"]["p_name_green"][li["l_partkey"] - 1] == 1)[0]
    todo = rows
    for s in range(1, 6):                     # a part has four suppliers
        li["l_suppkey"][todo] = s
        todo = todo[np.isin(li["l_partkey"][todo] * S + s, have)]
    assert len(todo) == 0


def q9_one_survivor(b):
    li, pa = b["lineitem"], b["part"]
    r = np.nonzero(pa["p_name_green"][li["l_partkey"] - 1] == 1)[0][0]
    p = li["l_partkey"][r]
    pa["p_name_green"][:] = 0
    pa["p_name_green"][p - 1] = 1
    other = np.nonzero(li["l_partkey"] == p)[0]
    li["l_partkey"][other[other != r]] = p % len(pa["p_partkey"]) + 1


def q9_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0
    b["partsupp"]["ps_supplycost"][:] = 0.0


def q11_window_miss(b):
    b["partsupp"]["ps_supplycost"][:] = 0.0   # 0 > 0: the HAVING is exclusive


def q11_join_miss(b):
    nk = b["supplier"]["s_nationkey"]
    nk[nk == 7] = 6                           # no GERMANY supplier


def q11_one_survivor(b):
    ps = b["partsupp"]
    german = b["supplier"]["s_nationkey"][ps["ps_suppkey"] - 1] == 7
    ps["ps_supplycost"][:] = 0.0
    ps["ps_supplycost"][np.nonzero(german)[0][0]] = 2.5


def q12_window_miss(b):
    rd = b["lineitem"]["l_receiptdate"]
    rd[:] = _sides(len(rd), OQ.Q12_LO - 1, OQ.Q12_HI)


def q12_one_survivor(b):
    rows = np.nonzero(_q12_rows(b))[0]
    b["lineitem"]["l_receiptdate"][rows[1:]] = OQ.Q12_HI


def q12_hot_key(b):
    li = b["lineitem"]
    rows = _q12_rows(b)
    li["l_orderkey"][rows] = li["l_orderkey"][np.nonzero(rows)[0][0]]
    li["l_shipmode"][rows] = 2                # all MAIL: one cell


def q12_zero_sum(b):
    """Counts have no zero sum; the nearest thing: every order is low
    priority, so the high-priority count of both modes is exactly 0."""
    b["orders"]["o_orderpriority"][:] = 4


def q13_join_miss(b):
    """No order carries a key of the customer table (one past its end)."""
    b["orders"]["o_custkey"][:] = len(b["customer"]["c_custkey"]) + 1


def q13_window_miss(b):
    b["orders"]["o_comment_special"][:] = 1


def q13_one_survivor(b):
    q13_window_miss(b)
    b["orders"]["o_comment_special"][321] = 0


def q13_hot_key(b):
    b["orders"]["o_custkey"][:] = 7


def q14_window_miss(b):
    sd = b["lineitem"]["l_shipdate"]
    sd[:] = _sides(len(sd), OQ.Q14_LO - 1, OQ.Q14_HI)


def q14_join_miss(b):
    b["part"]["p_type"][:] %= 25              # no PROMO part


def q14_one_survivor(b):
    q14_window_miss(b)
    li = b["lineitem"]
    li["l_shipdate"][9] = OQ.Q14_LO
    b["part"]["p_type"][li["l_partkey"][9] - 1] = 75     # PROMO ANODIZED BRASS


def q14_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q15_window_miss(b):
    sd = b["lineitem"]["l_shipdate"]
    sd[:] = _sides(len(sd), OQ.Q15_LO - 1, OQ.Q15_HI)


def q15_one_survivor(b):
    q15_window_miss(b)
    b["lineitem"]["l_shipdate"][11] = OQ.Q15_LO


def q15_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q15_hot_key(b):
    li = b["lineitem"]
    m = (li["l_shipdate"] >= OQ.Q15_LO) & (li["l_shipdate"] < OQ.Q15_HI)
    li["l_suppkey"][m] = 7


def q16_window_miss(b):
    b["part"]["p_size"][:] = 1


def q16_join_miss(b):
    b["supplier"]["s_comment_complaints"][:] = 1


def q16_one_survivor(b):
    pa = b["part"]
    pa["p_size"][:] = 1
    pa["p_size"][0], pa["p_brand"][0], pa["p_type"][0] = 49, 0, 0
    b["supplier"]["s_comment_complaints"][:] = 1
    b["supplier"]["s_comment_complaints"][
        b["partsupp"]["ps_suppkey"][0] - 1] = 0


def q17_window_miss(b):
    b["lineitem"]["l_quantity"][:] = 5.0      # 5 < 0.2 * 5 never holds


def _q17_no_part(b):
    c = b["part"]["p_container"]
    c[c == 17] = 18


def q17_join_miss(b):
    """The brand/container parts exist, but no line carries their key."""
    li, pa = b["lineitem"], b["part"]
    sel = (pa["p_brand"] == 12) & (pa["p_container"] == 17)
    other = pa["p_partkey"][~sel][0]
    li["l_partkey"][sel[li["l_partkey"] - 1]] = other


def q17_one_survivor(b):
    li, pa = b["lineitem"], b["part"]
    p = pa["p_partkey"][(pa["p_brand"] == 12) & (pa["p_container"] == 17)][0]
    _q17_no_part(b)
    pa["p_container"][p - 1] = 17
    rows = np.nonzero(li["l_partkey"] == p)[0]
    assert len(rows) >= 2
    li["l_quantity"][rows] = 50.0
    li["l_quantity"][rows[0]] = 1.0


def q17_zero_sum(b):
    b["lineitem"]["l_extendedprice"][:] = 0.0


def q19_window_miss(b):
    q = b["lineitem"]["l_quantity"]
    q[:] = np.where(np.arange(len(q)) % 2 == 0, 0.0, 31.0)


def q19_join_miss(b):
    br = b["part"]["p_brand"]
    br[np.isin(br, [1, 7, 13])] = 0


def q19_one_survivor(b):
    rows = np.nonzero(_q19_rows(b))[0]
    b["lineitem"]["l_shipinstruct"][rows[1:]] = 0


def q19_zero_sum(b):
    b["lineitem"]["l_discount"][:] = 1.0


def q20_window_miss(b):
    sd = b["lineitem"]["l_shipdate"]
    sd[:] = _sides(len(sd), G.Q5_LO - 1, G.Q5_HI)


def q20_join_miss(b):
    n1 = b["part"]["p_name1"]
    n1[n1 == G.P_NAME_FOREST] = 30


def q20_one_survivor(b):
    win = OQ.q20(b["lineitem"], b["part"], b["partsupp"], b["supplier"],
                 b["nation"])
    b["supplier"]["s_nationkey"][win[1:] - 1] = 0


def q22_window_miss(b):
    b["customer"]["c_acctbal"][:] = 100.0     # nobody is ABOVE the average


def q22_join_miss(b):
    n = len(b["customer"]["c_custkey"])
    b["orders"]["o_custkey"][:n] = b["customer"]["c_custkey"]    # anti join


def q22_one_survivor(b):
    q22_join_miss(b)
    cu = b["customer"]
    k = np.nonzero(cu["c_nationkey"] == 3)[0][0]         # country code 13
    cu["c_acctbal"][k] = 9999.75
    oc = b["orders"]["o_custkey"]
    oc[oc == k + 1] = k + 2 if k + 2 <= len(cu["c_custkey"]) else k


# ---- the case table ---------------------------------------------------

_W, _J, _O, _H, _Z, _T, _S = ("window_miss", "join_miss", "one_survivor",
                              "hot_key", "zero_sum", "tie_at_limit",
                              "short_result")
_TABLE = [
    ("q1", (_W, _O, _H, _Z)),
    ("q2", (_W, _J, _O, _T, _S)),
    ("q3", (_W, _J, _O, _H, _Z, _T, _S)),
    ("q4", (_W, _J, _O, _H)),
    ("q5", (_W, _J, _O, _H, _Z)),
    ("q6", (_W, _O, _Z)),
    ("q7", (_W, _J, _O, _Z)),
    ("q8", (_W, _J, _O, _Z)),
    ("q9", (_W, _J, _O, _Z)),
    ("q10", (_W, _J, _O, _H, _Z, _T, _S)),
    ("q11", (_W, _J, _O)),
    ("q12", (_W, _O, _H, _Z)),
    ("q13", (_W, _J, _O, _H)),
    ("q14", (_W, _J, _O, _Z)),
    ("q15", (_W, _O, _H, _Z)),
    ("q16", (_W, _J, _O)),
    ("q17", (_W, _J, _O, _Z)),
    ("q18", (_W, _J, _O, _H, _T, _S)),
    ("q19", (_W, _J, _O, _Z)),
    ("q20", (_W, _J, _O)),
    ("q21", (_W, _J, _O, _T, _S)),
    ("q22", (_W, _J, _O)),
]
CASES = [(q, m) for q, muts in _TABLE for m in muts]
CASE_IDS = ["%s-%s" % c for c in CASES]
_BUILT = {}


def build(q, mut):
    """The frozen mutated tables of one case (built once per process)."""
    if (q, mut) not in _BUILT:
        kind = "raw" if q in RAW_QUERIES else "exact"
        sf = SF_Q21_TIE if (q, mut) == ("q21", "tie_at_limit") else SF
        b = _copy(base(kind, sf))
        globals()["%s_%s" % (q, mut)](b)
        if q not in ("q10", "q18"):
            # one customer table; Q10/Q18 never touch it (their Acero
            # restatements regenerate it from _sf/_seed)
            for c, a in b["customer"].items():
                b["customer_s"][c] = a
        _BUILT[(q, mut)] = _freeze(b)
    return _BUILT[(q, mut)]


def _hot_rows(q, d):
    """Rows that reach the single group of a hot_key case."""
    li = d["lineitem"]
    if q == "q1": return int(run_oracle(q, d)["count_order"][0])
    if q == "q4":
        key = d["orders"]["o_orderkey"][
            (d["orders"]["o_orderdate"] >= OQ.Q4_LO)
            & (d["orders"]["o_orderdate"] < OQ.Q4_HI)][0]
        return int(((li["l_orderkey"] == key)
                    & (li["l_commitdate"] < li["l_receiptdate"])).sum())
    if q == "q12": return int(values(q, run_oracle(q, d)).sum())
    if q == "q13": return max(run_oracle(q, d))
    if q == "q18":
        return int((li["l_orderkey"] ==
                    run_oracle(q, d)["o_orderkey"][0]).sum())
    return int(values(q, run_oracle(q, revalued(d))).sum())   # q3 q5 q10 q15


_ROWS_BY_REVALUE = ("q3", "q5", "q7", "q9", "q10", "q15", "q19")


def survivor_rows(q, d):
    """Rows that reach the final aggregate, where the answer can tell:
    counts directly, revenue sums through revalued() (each row then adds
    exactly 1). None for Q2, Q8, Q11, Q13, Q14, Q18 and Q20, whose answers
    are a min, a ratio, a HAVING, per-order groups or a distinct set."""
    ans = run_oracle(q, d)
    if q == "q1": return int(ans["count_order"].sum())
    if q == "q6": return int(ans["rows_passed"])
    if q in ("q4", "q16", "q21"): return int(sum(ans.values()))
    if q == "q12": return int(values(q, ans).sum())
    if q == "q22": return int(sum(n for n, _ in ans.values()))
    if q == "q17": return int(round(7.0 * run_oracle(q, revalued(d))))
    if q in _ROWS_BY_REVALUE:
        return int(round(values(q, run_oracle(q, revalued(d))).sum()))
    return None


def check_precondition(q, mut, d):
    """No vacuous cases: what the mutator promises, asserted on the oracle's
    own answer before anything is compared."""
    ans = run_oracle(q, d)
    v, n = values(q, ans), n_groups(q, ans)
    if mut in ("window_miss", "join_miss"):
        if q == "q13":                        # left join: all customers at 0
            assert ans == {0: len(d["customer"]["c_custkey"])}
        else:
            assert n == 0 and not v.any(), (n, v)
    elif mut == "one_survivor":
        if q == "q13":
            assert ans == {0: len(d["customer"]["c_custkey"]) - 1, 1: 1}
        else:
            assert n == 1 and np.count_nonzero(v) == 1, (n, v)
        if q == "q3":
            assert len(ans[0]["l_orderkey"]) == 1
        assert survivor_rows(q, d) in (1, None), survivor_rows(q, d)
    elif mut == "hot_key":
        assert np.count_nonzero(v) == 1 and (
            n == 1 or q in FIXED_DOMAIN), (n, v)
        assert _hot_rows(q, d) >= 256
    elif mut == "zero_sum" and q == "q12":
        assert all(h == 0 for h, _ in ans.values()), ans
        assert sum(lo for _, lo in ans.values()) > 0, ans
    elif mut == "zero_sum":
        assert len(v) >= 1 and not v.any(), v
        if q == "q1":
            assert n >= 1
        else:
            assert n_groups(q, run_oracle(q, revalued(d, q))) >= 1
            if q not in SCALAR and q not in FIXED_DOMAIN:
                assert n >= 1
    elif mut == "tie_at_limit":
        lim = LIMITS[q]
        allv = values(q, run_oracle(q, d, limit=1 << 40))
        if q == "q3":
            allv = -np.sort(-run_oracle(q, d)[0]["revenue"])
        assert len(allv) > 4 * lim + 64, len(allv)
        assert allv[lim - 1] == allv[lim], allv[:lim + 1]
    elif mut == "short_result":
        assert 0 < n < LIMITS[q], n
    else:
        raise KeyError(mut)
