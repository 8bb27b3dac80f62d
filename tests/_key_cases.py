"""Case builders and plain references for the adversarial-key tests of the
join, group-by, partition and sort operators (test_gpu_key_edges.py runs
them on the device, test_key_edges_cpu.py checks the builders themselves).

Everything here is Python integers or numpy, written from the operator's
definition and not from the kernels' bit tricks."""
import math

import numpy as np

M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1

_INC = 0x9E3779B97F4A7C15
_MUL1 = 0xBF58476D1CE4E5B9
_MUL2 = 0x94D049BB133111EB
_INV1 = pow(_MUL1, -1, 1 << 64)
_INV2 = pow(_MUL2, -1, 1 << 64)


def splitmix64_int(x):
    """splitmix64 finalizer over one Python integer (the twin of
    oracle.executors.splitmix64, which test_abi pins to the C code)."""
    x = (x + _INC) & M64
    x ^= x >> 30
    x = (x * _MUL1) & M64
    x ^= x >> 27
    x = (x * _MUL2) & M64
    x ^= x >> 31
    return x


def _unxorshift(y, s):
    """Solve x ^ (x >> s) == y for a 64-bit x."""
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def inv_splitmix64(y):
    """The x in [0, 2^64) with splitmix64(x) == y: undo the three
    xorshifts, multiply by the inverses mod 2^64 of the two constants,
    subtract the increment."""
    y = _unxorshift(y & M64, 31)
    y = (y * _INV2) & M64
    y = _unxorshift(y, 27)
    y = (y * _INV1) & M64
    y = _unxorshift(y, 30)
    return (y - _INC) & M64


def _as_i64(u):
    return u - (1 << 64) if u >> 63 else u


def cluster_keys(cap, home, m, start=0):
    """m distinct i64 keys (Python ints) whose home slot
    splitmix64(key) & (cap-1) is `home`; a different `start` gives a
    disjoint set. INT64_MIN (the tables' empty marker) is never returned."""
    assert cap & (cap - 1) == 0 and 0 <= home < cap <= (1 << 32)
    out = []
    j = start
    while len(out) < m:
        k = _as_i64(inv_splitmix64((j << 32) | home))
        j += 1
        if k != I64_MIN:
            out.append(k)
    return out


def home_slot(key, cap):
    return splitmix64_int(key & M64) & (cap - 1)


def linear_probe_slots(keys, cap):
    """Set of slots a linear-probing table of `cap` slots holds after the
    distinct `keys` were inserted, in any order (the occupied SET does not
    depend on the insertion order)."""
    used = set()
    for k in keys:
        s = home_slot(k, cap)
        while s in used:
            s = (s + 1) & (cap - 1)
        used.add(s)
    return used


def f64_total_order_key(v):
    """Sort key of one double: every NaN greatest, -0.0 before +0.0."""
    v = float(v)
    nan = math.isnan(v)
    zero_rank = 0
    if not nan and v == 0:
        zero_rank = 0 if math.copysign(1.0, v) < 0 else 1
    return (nan, 0.0 if nan else v, zero_rank)


def f64_sort_reference(vals, descending=False):
    """Stable permutation of `vals` in the f64_total_order_key order.
    reverse=True keeps the original order of equal elements too."""
    keys = [f64_total_order_key(v) for v in vals]
    return sorted(range(len(vals)), key=keys.__getitem__, reverse=descending)


F64_SPECIAL_BITS = [
    0x0000000000000000, 0x8000000000000000,      # +-0
    0x0000000000000001, 0x8000000000000001,      # +-5e-324
    0x0010000000000000, 0x8010000000000000,      # +-DBL_MIN
    0x3FF0000000000000, 0xBFF0000000000000,      # +-1
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,      # +-DBL_MAX
    0x7FF0000000000000, 0xFFF0000000000000,      # +-inf
    0x7FF8000000000000, 0xFFF8000000000000,      # quiet NaN, both signs
    0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,      # signalling / all-ones NaN
]


def f64_specials(n, seed):
    """n doubles drawn with repeats from F64_SPECIAL_BITS (bit-exact)."""
    rng = np.random.default_rng(seed)
    pool = np.array(F64_SPECIAL_BITS, dtype=np.uint64)
    vals = pool[rng.integers(0, len(pool), n)]
    vals[: len(pool)] = pool              # every special at least once
    return vals.view(np.float64)


def join_reference(build_keys, probe_keys):
    """dict-of-lists join: (sorted inner (probe, build) pairs, semi probe
    index set, anti probe index set)."""
    rows = {}
    for b, k in enumerate(build_keys):
        rows.setdefault(int(k), []).append(b)
    inner, semi, anti = [], set(), set()
    for p, k in enumerate(probe_keys):
        hit = rows.get(int(k))
        if hit:
            semi.add(p)
            inner.extend((p, b) for b in hit)
        else:
            anti.add(p)
    return sorted(inner), semi, anti


def groupby_reference(keys, vals, agg_ops):
    """{key: [agg per column]} with 0 = SUM, 1 = MIN, 2 = MAX over Python
    floats (the tests use integer-valued doubles, so sums are exact)."""
    out = {}
    for i, k in enumerate(keys):
        k = int(k)
        row = [float(v[i]) for v in vals]
        acc = out.get(k)
        if acc is None:
            out[k] = row
            continue
        for c, op in enumerate(agg_ops):
            if op == 0:
                acc[c] += row[c]
            elif op == 1:
                acc[c] = min(acc[c], row[c])
            else:
                acc[c] = max(acc[c], row[c])
    return out


def range_part_reference(keys, per_range, nparts):
    return [min(max((int(k) - 1) // per_range, 0), nparts - 1) for k in keys]
