"""Float edge values for every aggregate path, and the plain reference.

No device and no numpy reductions: the reference is plain Python over
lists (math.fsum, fractions.Fraction). The rules are those of pyarrow
Acero, the engine every query here is anchored to:

  SUM  finite inputs: math.fsum. Any NaN: NaN. +inf with -inf: NaN. An
       infinity of one sign only: that infinity.
  MIN/MAX  skip NaN; a non-empty, all-NaN group is NaN.
  empty group: the identity (0, +inf, -inf); on the null_values paths NULL
       (None here).
  0.0 and -0.0 compare equal; their sign bit is not asserted.

Intermediate overflow is left out on purpose: 1e308 + 1e308 - 1e308 is
+inf or 1e308 depending on the summation order, and no path here fixes an
order. +-DBL_MAX stand alone in their groups for that reason.

A case is a small table: group ids, value columns, optional validity
masks. Families (float edge values in aggregates):

  exact      integer-valued doubles (and quarter multiples), every partial
             sum in any order below 2**53: bit-exact, sees any dropped or
             doubled row whatever the order.
  cancel     magnitudes in [1, 2**20], mixed signs, true sum near zero:
             |got - fsum| <= gamma(n-1+k) * sum|exact term|.
  subnormal  copies of 5e-324 and mixed-sign subnormals: exact, no flush.
  special    NaN / inf / zeros / DBL_MAX groups, NaNs of both signs with
             payloads.
  hot        one group of 4096 rows beside 63 single-row groups.
"""
import functools
import math
import random
import struct
from collections import namedtuple
from fractions import Fraction

from _key_cases import F64_SPECIAL_BITS

SUM, MIN, MAX = 0, 1, 2
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max"}
U = 2.0 ** -53
INF = float("inf")
DBL_MAX = 1.7976931348623157e308
TINY = 5e-324


def gamma(m):
    """Higham's gamma_m = m*u / (1 - m*u), u = 2**-53."""
    return m * U / (1.0 - m * U)


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


# NaNs of both signs, quiet, signalling and all-ones payloads
# and the pattern MIN/MAX slots hold before their first input (ops.
# MM_NONE_BITS): as an input it is a NaN like any other
NANS = [f64(b) for b in F64_SPECIAL_BITS if math.isnan(f64(b))] + \
    [f64(0x7FF8C0DE0000A66F)]
NAN = NANS[0]


# ---- the reference ---------------------------------------------------------
def ref_sum(xs):
    if any(x != x for x in xs):
        return NAN
    pos, neg = INF in xs, -INF in xs
    if pos and neg:
        return NAN
    if pos or neg:
        return INF if pos else -INF
    return math.fsum(xs)


def ref_min(xs):
    if not xs:
        return INF
    ys = [x for x in xs if x == x]
    return min(ys) if ys else NAN


def ref_max(xs):
    if not xs:
        return -INF
    ys = [x for x in xs if x == x]
    return max(ys) if ys else NAN


REF = {SUM: ref_sum, MIN: ref_min, MAX: ref_max}


def group_rows(gids, col, ngroups, mask=None):
    """-> per group the list of its non-NULL values, in row order."""
    rows = [[] for _ in range(ngroups)]
    for i, (g, x) in enumerate(zip(gids, col)):
        if 0 <= g < ngroups and (mask is None or mask[i]):
            rows[g].append(x)
    return rows


def reference(gids, col, ngroups, op, mask=None, null_values=False):
    """-> list [ngroups] of op over each group; None for a group without a
    value when null_values."""
    out = []
    for xs in group_rows(gids, col, ngroups, mask):
        out.append(None if (null_values and not xs) else REF[op](xs))
    return out


def sum_bound(xs, k=0, exact_terms=None):
    """gamma(n-1+k) * sum|exact term| for one group: the textbook bound of
    a length-n sum in ANY order, k roundings inside a term. exact_terms:
    the terms as Fractions where they are products (else xs themselves)."""
    terms = exact_terms if exact_terms is not None else \
        [Fraction(x) for x in xs]
    n = len(terms)
    if n == 0:
        return 0.0
    mag = sum(abs(t) for t in terms)
    return gamma(n - 1 + k) * float(mag)


def same(got, want, bound=0.0):
    """got equals want under the contract: None is None, NaN by isnan,
    infinities and exact families by ==, sums within bound."""
    if want is None or got is None:
        return want is None and got is None
    got, want = float(got), float(want)
    if want != want:
        return got != got
    if got != got:
        return False
    if math.isinf(want) or math.isinf(got) or bound == 0.0:
        return got == want
    return abs(got - want) <= bound


# ---- cases -------------------------------------------------------------------
# cols: list of value columns (lists of float); masks: None or one list of
# bool per column (True = valid, the NULL tests); k: roundings per term.
Case = namedtuple("Case", "name family gids cols ngroups masks")


def _case(name, family, groups, masks=None, seed=0):
    """groups: list over group id of (col0 values, col1 values, ...) row
    lists; rows of all groups are interleaved by a seeded shuffle."""
    ncols = len(groups[0])
    rows = []
    for g, cols in enumerate(groups):
        for i in range(len(cols[0])):
            rows.append((g,) + tuple(c[i] for c in cols))
    random.Random(seed).shuffle(rows)
    gids = [r[0] for r in rows]
    cols = [[r[1 + c] for r in rows] for c in range(ncols)]
    return Case(name, family, gids, cols, len(groups), masks)


def exact_cases():
    rng = random.Random(20261021)
    sizes = [1, 2, 63, 64, 65, 257, 1000]
    groups = []
    for n in sizes:
        ints = [float(rng.randint(-(1 << 30), 1 << 30)) for _ in range(n)]
        quarters = [rng.randint(-(1 << 20), 1 << 20) * 0.25 for _ in range(n)]
        groups.append((ints, quarters))
    return [_case("exact", "exact", groups, seed=1)]


def cancel_cases():
    rng = random.Random(20261022)
    groups = []
    for n in (4096, 1001, 257, 8):
        half = [rng.uniform(1.0, 2.0 ** 20) for _ in range(n // 2)]
        xs = half + [-x for x in half]
        if n % 2:
            xs.append(rng.uniform(1.0, 2.0))
        ys = [math.ldexp(rng.uniform(1.0, 2.0), rng.randint(0, 19))
              * rng.choice((-1.0, 1.0)) for _ in range(n)]
        groups.append((xs, ys))
    return [_case("cancel", "cancel", groups, seed=2)]


def subnormal_cases():
    rng = random.Random(20261023)
    mixed = [rng.randint(-(1 << 40), 1 << 40) * TINY for _ in range(300)]
    groups = [([TINY] * (1 << k), [-TINY] * (1 << k)) for k in (0, 4, 10)]
    groups.append((mixed, [-x for x in mixed]))
    groups.append(([TINY, -TINY, 2.2250738585072014e-308],
                   [2.225073858507201e-308, TINY, TINY]))
    return [_case("subnormal", "subnormal", groups, seed=3)]


def special_groups():
    """One (name, values) per special group; every NaN pattern appears."""
    return [
        ("only_nan", list(NANS)),
        ("one_nan", [NANS[-1]]),
        ("nan_finite", [NANS[1], 3.0, NANS[2], -7.5, NANS[3]]),
        ("nan_pinf", [NANS[0], INF, NANS[1]]),
        ("nan_ninf", [-INF, NANS[2]]),
        ("only_pinf", [INF, INF]),
        ("only_ninf", [-INF]),
        ("pinf_ninf", [INF, 1.0, -INF]),
        ("only_nzero", [-0.0, -0.0, -0.0]),
        ("zeros", [0.0, -0.0, 0.0, -0.0]),
        ("pmax", [DBL_MAX]),
        ("nmax", [-DBL_MAX]),
        ("finite", [1.0, 2.0, -3.0]),
    ]


def special_cases():
    groups = [(v, list(reversed(v))) for _, v in special_groups()]
    return [_case("special", "special", groups, seed=4)]


HOT_ROWS, HOT_OTHERS = 4096, 63


def hot_cases():
    rng = random.Random(20261024)
    flat = [x for _, v in special_groups() for x in v]
    singles = [flat[i % len(flat)] for i in range(HOT_OTHERS)]
    ints = [float(rng.randint(-(1 << 30), 1 << 30)) for _ in range(HOT_ROWS)]
    # NaN under contention: every 3rd row of the hot group is a NaN
    mixed = [NANS[i % len(NANS)] if i % 3 == 0 else x
             for i, x in enumerate(ints)]
    nans = [NANS[i % len(NANS)] for i in range(HOT_ROWS)]
    out = []
    for name, hot in (("hot_exact", ints), ("hot_nan_mixed", mixed),
                      ("hot_all_nan", nans)):
        groups = [(hot, list(reversed(hot)))]
        groups += [([s], [-s]) for s in singles]
        out.append(_case(name, "hot", groups, seed=5))
    return out


def all_cases():
    return (exact_cases() + cancel_cases() + subnormal_cases()
            + special_cases() + hot_cases())


def case_bound(case, c, g_rows, op):
    """The tolerance of column c's aggregate over one group's rows: 0
    (bit-exact) but for the SUM of the cancel family."""
    if case.family == "cancel" and op == SUM:
        return sum_bound(g_rows)
    return 0.0


# ---- NULL beside NaN (the nullable_vals paths) -------------------------------
def null_nan_case():
    """-> (gids, col, mask, ngroups). Group 0 {NULL, NaN}: MIN/MAX NaN and
    not NULL. Group 1 {NULL}: NULL. Group 2 {NULL, NaN, 2.0}: 2.0. Group 3
    {NaN under a NULL bit}: NULL, the NaN is never read. Group 4 no rows."""
    rows = [(0, 1.0, False), (0, NANS[1], True),
            (1, 5.0, False),
            (2, 9.0, False), (2, NANS[2], True), (2, 2.0, True),
            (3, NANS[0], False)]
    return ([r[0] for r in rows], [r[1] for r in rows],
            [r[2] for r in rows], 5)


# ---- Q1 / Q6 tables -----------------------------------------------------------
Q1_CUTOFF = 10471
Q1_FACTORS = (0.0, 0.25, 0.5)


@functools.lru_cache(maxsize=4)
def q1_case(n, tile, seed=6):
    """Q1 columns over n rows (n > tile): exact data on all six
    accumulators; half the rows, ~2000 at the most, pass the cutoff.
    Group ids are returnflag*2 + linestatus.

      gid 0  plain exact rows, spread over the whole range
      gid 1  one passing row has a NaN price          -> price sums NaN
      gid 2  NaN prices only in rows that FAIL the cutoff -> stays exact
      gid 3  every passing value is -0.0 or cancels to 0 inside one block
      gid 4  +inf at row 0 and -inf at row `tile`: one thread-block at
             n = tile + 1, two at a full grid sweep + 1 (the GPU test
             asserts which) -> NaN either way
      gid 5  no passing row

    -> dict of column lists, cached: read it, do not write to it."""
    rng = random.Random(seed)
    # the background is arithmetic on the row number (n reaches a full
    # grid sweep of the streaming kernel); every row of it fails the cutoff
    ship = [Q1_CUTOFF + 1 + i % 5 for i in range(n)]
    qty = [float(1 + i % 50) for i in range(n)]
    price = [float(900 + i * 7 % 104101) for i in range(n)]
    disc = [Q1_FACTORS[i % 3] for i in range(n)]
    tax = [Q1_FACTORS[i // 3 % 3] for i in range(n)]
    flag = [i % 7 % 3 for i in range(n)]
    stat = [i % 11 % 2 for i in range(n)]
    for i in range(n):          # failing rows of gid 2 carry NaN prices
        g = flag[i] * 2 + stat[i]
        if g == 2 and i % 2:
            price[i] = NANS[i % len(NANS)]
        elif g == 5:
            flag[i], stat[i] = 0, 0
    fixed = {0: 4, tile: 4, 1: 1, tile + 1 if tile + 1 < n else 2: 3}
    passing = set(rng.sample(range(n), min(n // 2, 2000))) | {n - 1, n - 2,
                                                         tile - 1}
    for i in sorted(passing - set(fixed)):
        g = rng.choice((0, 0, 1, 2))
        flag[i], stat[i] = divmod(g, 2)
        ship[i] = Q1_CUTOFF - rng.randint(0, 3)
        price[i] = float(rng.randint(900, 105000))
    for i, g in fixed.items():
        flag[i], stat[i] = divmod(g, 2)
        ship[i] = Q1_CUTOFF
    price[0], price[tile] = INF, -INF
    disc[0] = disc[tile] = 0.0           # inf * (1 - 0) stays inf
    price[1] = NANS[1]
    j = tile + 1 if tile + 1 < n else 2
    qty[j], price[j], disc[j], tax[j] = -0.0, -0.0, 0.0, 0.0
    return {"l_shipdate": ship, "l_quantity": qty, "l_extendedprice": price,
            "l_discount": disc, "l_tax": tax, "l_returnflag": flag,
            "l_linestatus": stat}


def q1_reference(t, lo=0, hi=None):
    """-> 6 rows [sum_qty, sum_price, sum_disc_price, sum_charge, sum_disc,
    count] over rows lo..hi-1 that pass the cutoff. Products are evaluated
    as the kernel's doubles; on exact data every one of them is exact."""
    hi = len(t["l_shipdate"]) if hi is None else hi
    terms = [[[] for _ in range(5)] for _ in range(6)]
    counts = [0] * 6
    for i in range(lo, hi):
        if t["l_shipdate"][i] > Q1_CUTOFF:
            continue
        g = t["l_returnflag"][i] * 2 + t["l_linestatus"][i]
        if not 0 <= g < 6:
            continue
        p, d, x = t["l_extendedprice"][i], t["l_discount"][i], t["l_tax"][i]
        dp = p * (1.0 - d)
        for j, v in enumerate((t["l_quantity"][i], p, dp, dp * (1.0 + x), d)):
            terms[g][j].append(v)
        counts[g] += 1
    return [[ref_sum(terms[g][j]) for j in range(5)] + [float(counts[g])]
            for g in range(6)]


Q6 = dict(date_lo=8766, date_hi=9131, disc_lo=0.25, disc_hi=0.5, qty_hi=24.0)


def q6_case(n, kind, seed=7):
    """Q6 columns over n rows; revenue = sum(price * disc) and the count
    over rows inside the date, discount and quantity windows. kind:
    'exact' | 'nan_pass' (one passing NaN price) | 'nan_fail' (NaN prices
    only outside the windows) | 'inf_pair' (+inf in the first row, -inf in
    the last: another block at n = block+1 pairs... or the tail thread) |
    'nzero' (every passing price is -0.0)."""
    rng = random.Random(seed)
    ship = [rng.randint(Q6["date_lo"] - 40, Q6["date_hi"] + 40)
            for _ in range(n)]
    qty = [float(rng.randint(1, 50)) for _ in range(n)]
    price = [float(rng.randint(900, 105000)) for _ in range(n)]
    disc = [rng.choice((0.0, 0.25, 0.5, 0.75)) for _ in range(n)]

    def passes(i):
        return (Q6["date_lo"] <= ship[i] < Q6["date_hi"]
                and Q6["disc_lo"] <= disc[i] <= Q6["disc_hi"]
                and qty[i] < Q6["qty_hi"])

    def force(i):
        ship[i], disc[i], qty[i] = Q6["date_lo"], 0.5, 1.0

    if kind == "nan_pass":
        force(n // 2)
        price[n // 2] = NANS[2]
    elif kind == "nan_fail":
        for i in range(n):
            if not passes(i) and i % 2:
                price[i] = NANS[i % len(NANS)]
    elif kind == "inf_pair":
        force(0)
        force(n - 1)
        price[0], price[n - 1] = INF, -INF
    elif kind == "nzero":
        for i in range(n):
            if passes(i):
                price[i] = -0.0
    else:
        assert kind == "exact"
    return {"l_shipdate": ship, "l_quantity": qty, "l_extendedprice": price,
            "l_discount": disc}


def q6_reference(t):
    terms = [t["l_extendedprice"][i] * t["l_discount"][i]
             for i in range(len(t["l_shipdate"]))
             if (Q6["date_lo"] <= t["l_shipdate"][i] < Q6["date_hi"]
                 and Q6["disc_lo"] <= t["l_discount"][i] <= Q6["disc_hi"]
                 and t["l_quantity"][i] < Q6["qty_hi"])]
    return ref_sum(terms), float(len(terms))


# ---- HAVING sum > threshold ---------------------------------------------------
GT_VALUES = [NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, DBL_MAX, -DBL_MAX, TINY]
GT_THRESHOLDS = [NAN, INF, -INF, -0.0, 0.0]
