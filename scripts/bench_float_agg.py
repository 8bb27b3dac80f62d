"""What the NaN rule of MIN/MAX costs in the accumulate loop (DESIGN.md
§3a''''''; numbers in profiles/float_agg.md). Workload of
profiles/null_values.md: 10 M rows, two int keys, 1 M groups.

  update  ops.GroupByKeys.update with one SUM, and with one MIN + one MAX:
          first call (every group new) and second call (every group exists)
  kernel  qk_groupby_dense_acc over the same codes, device timer, the same
          two variants, A B A B so that drift shows

Uses nothing newer than ops.GroupByKeys / ops.DenseAcc, so the same script
measures the parent commit (run it with the parent's tree first on
PYTHONPATH). One JSON line per measurement: median, min, max in ms.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

# appended, not inserted: a tree named on PYTHONPATH (the parent's) wins
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quokka_amd import ops, shim                            # noqa: E402
from quokka_amd.shim import DevColumn, c_u32, c_u64         # noqa: E402

N = 10_000_000
GROUPS = 1 << 20
VARIANTS = [("sum", [0]), ("minmax", [1, 2])]


def _ms(fn):
    shim.call("qk_stream_sync", None)
    t0 = time.perf_counter()
    fn()
    shim.call("qk_stream_sync", None)
    return (time.perf_counter() - t0) * 1e3


def _report(name, samples, **extra):
    print(json.dumps(dict(
        name=name, median_ms=round(statistics.median(samples), 4),
        min_ms=round(min(samples), 4), max_ms=round(max(samples), 4),
        reps=len(samples), **extra)), flush=True)


def _inputs():
    rng = np.random.default_rng(GROUPS)
    side = int(round(GROUPS ** 0.5))
    cols = [DevColumn.from_numpy(rng.integers(0, side, N).astype(np.int64)),
            DevColumn.from_numpy(
                rng.integers(0, GROUPS // side, N).astype(np.int64))]
    val = DevColumn.from_numpy(rng.integers(-50, 51, N).astype(np.float64))
    return cols, val


def bench_update(reps, cols, val):
    for tag, agg_ops in VARIANTS:
        first, second = [], []
        for _ in range(reps + 1):               # the first round is warm-up
            gb = ops.GroupByKeys(2, len(agg_ops), agg_ops=agg_ops,
                                 expected_groups=2 * GROUPS)
            vals = [val] * len(agg_ops)
            first.append(_ms(lambda: gb.update(cols, vals, N)))
            second.append(_ms(lambda: gb.update(cols, vals, N)))
            ngroups = gb.n_groups
            gb.free()
        _report("update_%s_new" % tag, first[1:], groups=int(ngroups))
        _report("update_%s_existing" % tag, second[1:], groups=int(ngroups))


def bench_kernel(reps, cols, val):
    kd = ops.DeviceKeyDict(2, expected=2 * GROUPS)
    codes = kd.encode(cols, N)
    g = kd.n_codes
    timer = ctypes.c_void_p(0)
    shim.call("qk_timer_create", ctypes.byref(timer))
    accs = {tag: ops.DenseAcc(len(o), o, capacity=g) for tag, o in VARIANTS}
    ptrs = {tag: DevColumn.from_numpy(np.array(
        [val.ptr.value] * len(o), dtype=np.uint64)) for tag, o in VARIANTS}
    for rnd in range(2):
        for tag, agg_ops in VARIANTS:
            acc = accs[tag]
            samples = []
            for _ in range(reps + 1):
                shim.call("qk_timer_start", timer, None)
                shim.call("qk_groupby_dense_acc", None, c_u64(N), codes.ptr,
                          c_u32(g), ptrs[tag].ptr,
                          acc._ops_dev.ptr if acc._ops_dev else None,
                          acc.nvals, acc.rstride, acc.acc.ptr, acc._err.ptr)
                shim.call("qk_timer_stop", timer, None)
                ms = ctypes.c_float(0)
                shim.call("qk_timer_elapsed_ms", timer, ctypes.byref(ms))
                samples.append(ms.value)
            med = statistics.median(samples[1:])
            _report("kernel_" + tag, samples[1:], round=rnd, groups=int(g),
                    grows_per_s=round(N / med / 1e6, 3))
    shim.call("qk_timer_destroy", timer)
    for c in list(ptrs.values()) + [codes]:
        c.free()
    for a in accs.values():
        a.free()
    kd.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["update", "kernel"])
    args = ap.parse_args()
    shim.init(0)
    print(json.dumps({"package": os.path.dirname(ops.__file__)}), flush=True)
    cols, val = _inputs()
    if args.only in (None, "update"):
        bench_update(args.reps, cols, val)
    if args.only in (None, "kernel"):
        bench_kernel(args.reps, cols, val)
    for c in cols + [val]:
        c.free()


if __name__ == "__main__":
    main()
