"""qk_q1_agg streaming kernel at the sizes where its structure changes:
below one thread-tile, block-tile edges, one grid sweep (one tile per block,
one short and one over), several tiles per block with a ragged tail, misaligned column
pointers (the row-pair fallback kernel) and accumulation across calls.

Reference: numpy bincount over gid = returnflag*2 + linestatus on rows with
shipdate <= cutoff. Gates are the project's: counts
exact, f64 sums within rtol 1e-9.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CUTOFF = 10471          # queries.Q1_CUTOFF; any value works, data is relative
COLS = ["l_shipdate", "l_quantity", "l_extendedprice", "l_discount", "l_tax",
        "l_returnflag", "l_linestatus"]


def _shape():
    """(T, G): rows per block tile and rows of one full grid sweep, read
    from the library (qk_q1_tile_rows / qk_q1_grid_blocks)."""
    from quokka_amd import shim
    t = int(shim._lib.qk_q1_tile_rows())
    nb = ctypes.c_int(0)
    shim._check(shim._lib.qk_q1_grid_blocks(ctypes.byref(nb)),
                "qk_q1_grid_blocks")
    return t, t * nb.value


def _reference(host, lo, hi):
    """(6,6) partials [qty, price, disc_price, charge, disc, count] of rows
    lo..hi-1."""
    s = slice(lo, hi)
    keep = host["l_shipdate"][s] <= CUTOFF
    gid = (host["l_returnflag"][s].astype(np.int64) * 2
           + host["l_linestatus"][s])[keep]
    q = host["l_quantity"][s][keep]
    p = host["l_extendedprice"][s][keep]
    d = host["l_discount"][s][keep]
    t = host["l_tax"][s][keep]
    dp = p * (1.0 - d)
    out = np.zeros((6, 6))
    for j, w in enumerate((q, p, dp, dp * (1.0 + t), d, None)):
        out[:, j] = np.bincount(gid, weights=w, minlength=6)[:6]
    return out


def _check(got, want):
    assert np.array_equal(got[:, 5], want[:, 5]), (got[:, 5], want[:, 5])
    np.testing.assert_allclose(got[:, :5], want[:, :5], rtol=1e-9, atol=0)


@pytest.fixture(scope="module")
def data():
    """3G+5 seeded rows staged once; every case is a row-range view."""
    from quokka_amd import shim
    from quokka_amd.shim import DevColumn
    shim.init(0)
    T, G = _shape()
    n = 3 * G + 5
    rng = np.random.default_rng(20260111)
    flag = rng.integers(0, 3, n).astype(np.uint8)
    stat = rng.integers(0, 2, n).astype(np.uint8)
    # all six group ids present even in the first rows
    flag[:6] = [0, 0, 1, 1, 2, 2]
    stat[:6] = [0, 1, 0, 1, 0, 1]
    host = {
        # +-30 days round the cutoff: both branches inside every wave
        "l_shipdate": (CUTOFF + rng.integers(-30, 31, n)).astype(np.int32),
        "l_quantity": rng.integers(1, 51, n).astype(np.float64),
        "l_extendedprice": rng.uniform(900.0, 105000.0, n),
        "l_discount": rng.integers(0, 11, n) / 100.0,
        "l_tax": rng.integers(0, 9, n) / 100.0,
        "l_returnflag": flag,
        "l_linestatus": stat,
    }
    dev = {k: DevColumn.from_numpy(host[k]) for k in COLS}
    yield {"host": host, "dev": dev, "T": T, "G": G, "n": n}
    for c in dev.values():
        c.free()


def _run(data, lo, hi, acc=None):
    """qk_q1_agg over rows lo..hi-1 of the staged columns -> (6,6)."""
    from quokka_amd import ops, queries
    cols = {k: data["dev"][k].view(lo, hi - lo) for k in COLS}
    own = acc is None
    acc = queries.q1_partials_device(cols, cutoff=CUTOFF, acc=acc)
    got = ops.q1_read_partials(acc)
    if own:
        acc.free()
    return got


def _size(data, case):
    T, G = data["T"], data["G"]
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "G-1": G - 1, "G+1": G + 1,
            "3G+5": 3 * G + 5}.get(case, case)


@pytest.mark.parametrize("case", [0, 1, 2, 3, 4, 5, 7, "T-1", "T", "T+1",
                                  "G-1", "G+1", "3G+5"])
def test_sizes(data, case):
    n = _size(data, case)
    assert n <= data["n"]
    got = _run(data, 0, n)
    want = _reference(data["host"], 0, n)
    print("n=%d counts=%s max rel err=%.3g" % (
        n, got[:, 5].astype(np.int64).tolist(),
        np.max(np.abs(got[:, :5] - want[:, :5])
               / np.maximum(np.abs(want[:, :5]), 1e-300))))
    _check(got, want)


@pytest.mark.parametrize("case", [2, 8, "T+1", "G+1", "3G+5"])
def test_misaligned_views_take_the_fallback(data, case):
    """Rows 1..n-1 through view(1, n-1) on all seven columns: f64 pointers
    8 B-aligned only, shipdate 4 B, flags odd."""
    n = _size(data, case)
    got = _run(data, 1, n)
    _check(got, _reference(data["host"], 1, n))


def test_two_calls_accumulate(data):
    """Two calls into one acc == one call over the concatenation."""
    from quokka_amd import queries
    T, G = data["T"], data["G"]
    cut = G + 2 * T            # aligned split: both calls stream
    n = 2 * G + 3
    acc = queries._zero48()
    _run(data, 0, cut, acc=acc)
    got = _run(data, cut, n, acc=acc)
    acc.free()
    want = _reference(data["host"], 0, n)
    _check(got, want)
    _check(_run(data, 0, n), want)
