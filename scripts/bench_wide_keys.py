"""Measure the multi-column group-by through the device key dictionary.

N rows (default 10M), two int64 key columns whose pairs form G groups
(1 k, 1 M, 5 M), one f64 SUM column. Three paths:
  (a) ops.GroupByKeys: qk_keydict_encode (claim / finalise / resolve) +
      qk_groupby_dense_acc, key columns already in HBM
  (b) ops.GroupByI64 over the pre-combined key a * gb + b at the same
      cardinality: the single-key floor that (a) pays two more kernels
      to approach; only possible when the author knows each domain
  (c) GPUAggExecutor.execute() on the Arrow batch with the host-codebook
      _encode_keys path (np.unique per key per batch + packing), against
      the same call with device_keys=True; both include the h2d copies
"first" is one update into a fresh table sized for the batch, "again" a
second update of the same rows into the now populated table. Wall clock
around calls that end in a device sync, best of --reps.
Run on a GPU box: python scripts/bench_wide_keys.py [--rows N] [--reps R]
Prints markdown table rows for profiles/wide_keys.md.
"""
import argparse
import os
import sys
import time

import numpy as np
import pyarrow as pa

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quokka_amd import ops, shim                            # noqa: E402
from quokka_amd.executors import GPUAggExecutor             # noqa: E402

SHAPES = ((32, 32), (1024, 1024), (2500, 2000))


def wall_ms(fn):
    shim.call("qk_stream_sync", None)
    t0 = time.perf_counter()
    fn()
    shim.call("qk_stream_sync", None)
    return (time.perf_counter() - t0) * 1e3


def time_table(make, update, reps):
    first, again = [], []
    groups = 0
    for _ in range(reps):
        gb = make()
        first.append(wall_ms(lambda: update(gb)))
        again.append(wall_ms(lambda: update(gb)))
        groups = gb.n_groups
        gb.free()
    return min(first), min(again), groups


def time_executor(table, reps, **kw):
    ts = []
    for _ in range(reps):
        ex = GPUAggExecutor(["a", "b"], None, "sum(v) as s", **kw)
        ts.append(wall_ms(lambda: ex.execute([table], 0, 0)))
        ex.done(0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n = args.rows
    shim.init(0)
    rng = np.random.default_rng(1)
    print("rows=%d reps=%d" % (n, args.reps), flush=True)
    # warm-up: load every kernel of both table paths once at a small size
    w = [shim.DevColumn.from_numpy(x) for x in
         (np.arange(4096, dtype=np.int64), np.arange(4096, dtype=np.int64),
          np.ones(4096))]
    for make, upd in ((lambda: ops.GroupByKeys(2, 1, expected_groups=1),
                       lambda g: g.update(w[:2], [w[2]], 4096)),
                      (lambda: ops.GroupByI64(4096, 1),
                       lambda g: g.update(w[0], [w[2]], 4096))):
        g = make()
        upd(g)
        g.extract()
        g.free()
    for c in w:
        c.free()
    print("| groups | (a) first ms | (a) again ms | (b) first ms | (b) again "
          "ms | (a)/(b) again | (c) host-codebook execute ms | device_keys "
          "execute ms | device/(c) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for ga, gb_ in SHAPES:
        a = rng.integers(0, ga, n).astype(np.int64)
        b = rng.integers(0, gb_, n).astype(np.int64)
        v = rng.random(n)
        da, db, dv = (shim.DevColumn.from_numpy(x) for x in (a, b, v))
        dk = shim.DevColumn.from_numpy(a * gb_ + b)
        fa, aa, groups = time_table(
            lambda: ops.GroupByKeys(2, 1, expected_groups=n),
            lambda g: g.update([da, db], [dv], n), args.reps)
        fb, ab, groups_b = time_table(
            lambda: ops.GroupByI64(n, 1),
            lambda g: g.update(dk, [dv], n), args.reps)
        assert groups == groups_b, (groups, groups_b)
        for c in (da, db, dv, dk):
            c.free()
        t = pa.table({"a": a, "b": b, "v": v})
        tc = time_executor(t, args.reps)
        td = time_executor(t, args.reps, device_keys=True)
        print("| %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.1f | %.1f | %.3f |"
              % (groups, fa, aa, fb, ab, aa / ab, tc, td, td / tc),
              flush=True)


if __name__ == "__main__":
    main()
