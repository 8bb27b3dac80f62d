"""Null values in the aggregate (DESIGN.md §3a''''): that the defaults did
not move, and what the opt-in costs. Workload of profiles/null_keys.md:
10 M rows, two int keys, 1 M groups, one SUM.

  update   ops.GroupByKeys.update, first call (every group new) and second
           call on the same batch (every group exists)
  execute  GPUAggExecutor(device_keys=True).execute on the same rows as an
           Arrow table (host staging included), then done()
  kernel   qk_groupby_dense_acc against qk_groupby_dense_acc_valid over the
           same codes, device timer: no bitmap at all (a 0 pointer), a
           bitmap with 0 % nulls, and one with 10 % nulls

--baseline runs only what exists without the null-value arguments, so the
same script measures the parent commit (run it with the parent's tree
first on PYTHONPATH). Prints one JSON line per measurement: median, min and
max over --reps, in ms.
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
from quokka_amd.executors import GPUAggExecutor             # noqa: E402
from quokka_amd.shim import DevColumn, c_u32, c_u64         # noqa: E402

N = 10_000_000
GROUPS = 1 << 20


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


def _keys(rng):
    side = int(round(GROUPS ** 0.5))
    return (rng.integers(0, side, N).astype(np.int64),
            rng.integers(0, GROUPS // side, N).astype(np.int64))


def bench_update(reps, nullable, frac):
    rng = np.random.default_rng(GROUPS)
    ka, kb = _keys(rng)
    cols = [DevColumn.from_numpy(ka), DevColumn.from_numpy(kb)]
    val = DevColumn.from_numpy(rng.integers(-50, 51, N).astype(np.float64))
    kw, ukw, bitmap = {}, {}, None
    if nullable:
        kw = {"nullable_vals": True}
        if frac is not None:        # device bitmap: the upload is not timed
            bitmap = DevColumn.from_numpy(
                ops.pack_valid(rng.random(N) >= frac))
            ukw = {"val_valid": [bitmap]}
    first, second = [], []
    for _ in range(reps + 1):               # the first round is warm-up
        gb = ops.GroupByKeys(2, 1, expected_groups=2 * GROUPS, **kw)
        first.append(_ms(lambda: gb.update(cols, [val], N, **ukw)))
        second.append(_ms(lambda: gb.update(cols, [val], N, **ukw)))
        ngroups = gb.n_groups
        gb.free()
    tag = "update_" + ("plain" if not nullable else "nullable_" + (
        "nobitmap" if frac is None else "%dpct" % round(100 * frac)))
    _report(tag + "_new", first[1:], groups=int(ngroups))
    _report(tag + "_existing", second[1:], groups=int(ngroups))
    for c in cols + [val] + ([bitmap] if bitmap else []):
        c.free()


def bench_execute(reps, null_values, frac):
    import pyarrow as pa
    rng = np.random.default_rng(GROUPS)
    ka, kb = _keys(rng)
    v = rng.integers(-50, 51, N).astype(np.float64)
    mask = None if not frac else rng.random(N) < frac
    t = pa.table({"ka": ka, "kb": kb, "v": pa.array(v, mask=mask)})
    kw = {"null_values": True} if null_values else {}
    samples, rows = [], 0
    for _ in range(reps + 1):
        ex = GPUAggExecutor(["ka", "kb"], None, "sum(v) as sv",
                            device_keys=True, **kw)
        samples.append(_ms(lambda: ex.execute([t], 0, 0)))
        rows = ex.done(0).num_rows
    tag = "execute_" + ("plain" if not null_values else
                        "null_values_%dpct" % round(100 * (frac or 0)))
    _report(tag, samples[1:], groups=int(rows))


def bench_kernel(reps):
    """The two accumulate kernels over one code column; every group exists
    and its seen bit stands after the first (warm-up) launch."""
    rng = np.random.default_rng(GROUPS)
    ka, kb = _keys(rng)
    cols = [DevColumn.from_numpy(ka), DevColumn.from_numpy(kb)]
    kd = ops.DeviceKeyDict(2, expected=2 * GROUPS)
    codes = kd.encode(cols, N)
    g = kd.n_codes
    val = DevColumn.from_numpy(rng.integers(-50, 51, N).astype(np.float64))
    vptrs = DevColumn.from_numpy(np.array([val.ptr.value], dtype=np.uint64))
    acc = DevColumn.from_numpy(np.zeros(g))
    seen = DevColumn.from_numpy(np.zeros(g, dtype=np.uint64))
    err = DevColumn.from_numpy(np.zeros(1, dtype=np.uint32))
    timer = ctypes.c_void_p(0)
    shim.call("qk_timer_create", ctypes.byref(timer))

    def timed(launch):
        samples = []
        for _ in range(reps + 1):
            shim.call("qk_timer_start", timer, None)
            launch()
            shim.call("qk_timer_stop", timer, None)
            ms = ctypes.c_float(0)
            shim.call("qk_timer_elapsed_ms", timer, ctypes.byref(ms))
            samples.append(ms.value)
        return samples[1:]

    variants = [("plain", None, False)]
    for tag, frac in (("nobitmap", None), ("0pct", 0.0), ("10pct", 0.1)):
        variants.append((tag, frac, True))
    for rnd in range(2):                    # A B C D A B C D: drift shows
        for tag, frac, nullable in variants:
            if not nullable:
                samples = timed(lambda: shim.call(
                    "qk_groupby_dense_acc", None, c_u64(N), codes.ptr,
                    c_u32(g), vptrs.ptr, None, 1, 1, acc.ptr, err.ptr))
                name = "kernel_plain"
            else:
                bitmap = None
                if frac is not None:
                    bitmap = DevColumn.from_numpy(ops.pack_valid(
                        np.random.default_rng(5).random(N) >= frac))
                bptrs = DevColumn.from_numpy(np.array(
                    [bitmap.ptr.value if bitmap else 0], dtype=np.uint64))
                samples = timed(lambda: shim.call(
                    "qk_groupby_dense_acc_valid", None, c_u64(N), codes.ptr,
                    c_u32(g), vptrs.ptr, bptrs.ptr, None, 1, 1, acc.ptr,
                    seen.ptr, err.ptr))
                name = "kernel_valid_" + tag
                bptrs.free()
                if bitmap:
                    bitmap.free()
            med = statistics.median(samples)
            _report(name, samples, round=rnd, groups=int(g),
                    grows_per_s=round(N / med / 1e6, 3))
    assert int(err.to_numpy(1)[0]) == 0
    shim.call("qk_timer_destroy", timer)
    for c in cols + [codes, val, vptrs, acc, seen, err]:
        c.free()
    kd.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true",
                    help="default paths only (runs on the parent commit)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["update", "execute", "kernel"])
    args = ap.parse_args()
    shim.init(0)
    print(json.dumps({"package": os.path.dirname(ops.__file__)}), flush=True)
    want = lambda what: args.only in (None, what)           # noqa: E731
    if want("update"):
        bench_update(args.reps, False, None)
    if want("execute"):
        bench_execute(max(3, args.reps // 2), False, None)
    if args.baseline:
        return
    if want("update"):
        for frac in (None, 0.0, 0.1):
            bench_update(args.reps, True, frac)
    if want("execute"):
        for frac in (0.0, 0.1):
            bench_execute(max(3, args.reps // 2), True, frac)
    if want("kernel"):
        bench_kernel(args.reps)


if __name__ == "__main__":
    main()
