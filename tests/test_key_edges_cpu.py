"""CPU tests of the adversarial-key case builders (tests/_key_cases.py) and
of the host-side sentinel-key check: the executors must refuse a build or
group key equal to INT64_MIN (QK_JOIN_EMPTY) before any device call. No GPU
needed."""
import math
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _key_cases as K  # noqa: E402

from oracle.executors import splitmix64  # noqa: E402

I64_MIN, I64_MAX = K.I64_MIN, K.I64_MAX


def test_python_splitmix_matches_the_pinned_twin():
    rng = np.random.default_rng(11)
    xs = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    want = splitmix64(xs)
    for x, w in zip(xs.tolist(), want.tolist()):
        assert K.splitmix64_int(x) == w


def test_inv_splitmix64_round_trips():
    rng = np.random.default_rng(12)
    ys = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    xs = np.array([K.inv_splitmix64(y) for y in ys.tolist()],
                  dtype=np.uint64)
    assert np.array_equal(splitmix64(xs), ys)
    for y in (0, 1, K.M64, 1 << 63):
        assert K.splitmix64_int(K.inv_splitmix64(y)) == y


@pytest.mark.parametrize("cap,home,m", [(64, 63, 20), (64, 62, 30),
                                        (16, 0, 5), (1 << 20, 12345, 8)])
def test_cluster_keys_share_their_home_slot(cap, home, m):
    keys = K.cluster_keys(cap, home, m)
    assert len(set(keys)) == m
    arr = np.array(keys, dtype=np.int64)          # all fit an i64
    assert I64_MIN not in keys
    slots = splitmix64(arr.view(np.uint64)) & np.uint64(cap - 1)
    assert np.all(slots == home)
    more = K.cluster_keys(cap, home, m, start=m)
    assert not set(more) & set(keys)


def test_linear_probe_slots_wraps_the_table_end():
    keys = K.cluster_keys(64, 62, 20)
    assert K.linear_probe_slots(keys, 64) == {62, 63} | set(range(18))


def test_f64_total_order_key():
    key = K.f64_total_order_key
    neg_nan = np.array([0xFFF8000000000000], dtype=np.uint64).view(
        np.float64)[0]
    assert math.isnan(neg_nan) and math.copysign(1.0, neg_nan) < 0
    asc = [-math.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, math.inf]
    for a, b in zip(asc, asc[1:]):
        assert key(a) < key(b), (a, b)
    assert key(math.inf) < key(neg_nan)
    assert key(neg_nan) == key(math.nan)
    vals = [math.nan, 1.0, neg_nan, -0.0, 0.0, 1.0]
    assert K.f64_sort_reference(vals) == [3, 4, 1, 5, 0, 2]
    # descending keeps the input order of equals as well
    assert K.f64_sort_reference(vals, descending=True) == [0, 2, 1, 5, 4, 3]
    sp = K.f64_specials(100, 1)
    assert set(sp.view(np.uint64).tolist()) == set(K.F64_SPECIAL_BITS)


def test_range_part_reference():
    keys = [I64_MIN, I64_MIN + 1, -1, 0, 1, 10, 11, 40, 41, I64_MAX]
    assert K.range_part_reference(keys, 10, 4) == [0, 0, 0, 0, 0, 0, 1, 3,
                                                   3, 3]


# ---- sentinel helper -------------------------------------------------------

def test_sentinel_helper_raises_on_int64_min():
    from quokka_amd import ops
    keys = np.array([5, I64_MIN, 7], dtype=np.int64)
    with pytest.raises(ValueError) as e:
        ops.check_no_sentinel_key(keys, "SomeOperator", "o_key")
    assert "SomeOperator" in str(e.value) and "o_key" in str(e.value)
    assert "INT64_MIN" in str(e.value)


def test_sentinel_helper_passes_neighbours_and_empty():
    from quokka_amd import ops
    ops.check_no_sentinel_key(
        np.array([I64_MIN + 1, -1, 0, I64_MAX], dtype=np.int64), "op", "k")
    ops.check_no_sentinel_key(np.empty(0, dtype=np.int64), "op", "k")


# The executor checks run before the first device call, so they are
# observable on a host without a GPU.

def _tbl(keys, **extra):
    cols = {"k": pa.array(np.asarray(keys, dtype=np.int64))}
    for name, v in extra.items():
        cols[name] = pa.array(np.asarray(v, dtype=np.float64))
    return pa.table(cols)


def test_join_executor_refuses_sentinel_build_key():
    from quokka_amd import GPUBuildProbeJoinExecutor
    ex = GPUBuildProbeJoinExecutor(on="k", how="inner")
    ex.execute([_tbl([1, I64_MIN, 3], b=[1, 2, 3])], 1, 0)
    with pytest.raises(ValueError, match="GPUBuildProbeJoinExecutor.*'k'"):
        ex.execute([_tbl([1, 2], p=[1, 2])], 0, 0)


def test_disk_join_executor_refuses_sentinel_build_key(tmp_path):
    from quokka_amd.executors import GPUDiskBuildProbeJoinExecutor
    ex = GPUDiskBuildProbeJoinExecutor(on="k", spill_dir=str(tmp_path))
    with pytest.raises(ValueError,
                       match="GPUDiskBuildProbeJoinExecutor.*'k'"):
        ex.execute([_tbl([I64_MIN], b=[1])], 1, 0)
    assert ex.count == 0 and not os.listdir(str(tmp_path))


def test_agg_executor_refuses_sentinel_group_key():
    from quokka_amd import GPUAggExecutor
    ex = GPUAggExecutor(["k"], None, "sum(x) as sx")
    with pytest.raises(ValueError, match="GPUAggExecutor.*'k'"):
        ex.execute([_tbl([0, I64_MIN], x=[1, 2])], 0, 0)


def test_distinct_executor_refuses_sentinel_key():
    from quokka_amd.executors import GPUDistinctExecutor
    ex = GPUDistinctExecutor("k")
    with pytest.raises(ValueError, match="GPUDistinctExecutor.*'k'"):
        ex.execute([_tbl([I64_MIN, 4])], 0, 0)
