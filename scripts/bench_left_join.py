"""Join payloads that keep their NULLs (DESIGN.md §3a'''''): what the left
join's device emit saves, what the bitmap costs an inner join that did not
need one, the fused optional gather against the two kernels it replaces,
and that probe modes 0-2 did not move.

Workload: 10 M probe rows, 1 M build rows with unique int64 keys, about
half the probe keys present, two numeric payload columns per side (int64
and float64).

  probe    GPUBuildProbeJoinExecutor._probe wall time per probe batch (host
           staging, probe, gathers, Arrow result), build done beforehand:
           left and inner on the default path; with null_payloads=True left
           at 0 % and 10 % payload nulls and inner at 0 %
  take     qk_take_opt_i64 at 10 M indices against qk_gather_i64 +
           qk_valid_gather over the same indices, device timer, with the
           bytes each moves
  modes    qk_join_probe modes 0, 1, 2 (and 3) at 10 M rows, device timer

--baseline runs only what the parent commit has (default-path probe, modes
0-2), so the same script measures it: run it with the parent's tree first
on PYTHONPATH. Prints one JSON line per measurement: median, min and max
over --reps, in ms.
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
from quokka_amd.executors import GPUBuildProbeJoinExecutor  # noqa: E402
from quokka_amd.shim import DevColumn, c_u64                # noqa: E402

N_PROBE = 10_000_000
N_BUILD = 1_000_000


def _report(name, samples, **extra):
    print(json.dumps(dict(
        name=name, median_ms=round(statistics.median(samples), 4),
        min_ms=round(min(samples), 4), max_ms=round(max(samples), 4),
        reps=len(samples), **extra)), flush=True)


def _tables(frac):
    """-> (probe, build) Arrow tables; frac of every payload column NULL."""
    import pyarrow as pa
    rng = np.random.default_rng(N_BUILD)

    def col(values):
        if not frac:
            return pa.array(values)
        return pa.array(values, mask=rng.random(len(values)) < frac)
    build = pa.table({
        "k": rng.permutation(N_BUILD).astype(np.int64),
        "b_i64": col(rng.integers(-2 ** 62, 2 ** 62, N_BUILD)),
        "b_f64": col(rng.standard_normal(N_BUILD))})
    probe = pa.table({
        "k": rng.integers(0, 2 * N_BUILD, N_PROBE).astype(np.int64),
        "p_i64": col(rng.integers(-2 ** 62, 2 ** 62, N_PROBE)),
        "p_f64": col(rng.standard_normal(N_PROBE))})
    return probe, build


def bench_probe(reps, how, null_payloads, frac):
    probe, build = _tables(frac)
    kw = {"null_payloads": True} if null_payloads else {}
    ex = GPUBuildProbeJoinExecutor(on="k", how=how, **kw)
    ex.execute([build], 1, 0)
    samples, rows = [], 0
    for _ in range(reps + 1):               # the first round is warm-up
        shim.call("qk_stream_sync", None)
        t0 = time.perf_counter()
        out = ex.execute([probe], 0, 0)
        samples.append((time.perf_counter() - t0) * 1e3)
        rows = out.num_rows
        del out
    tag = "probe_%s_%s" % (how, "default" if not null_payloads else
                           "null_payloads_%dpct" % round(100 * frac))
    _report(tag, samples[1:], rows=int(rows))


def _timed(timer, reps, launch):
    samples = []
    for _ in range(reps + 1):
        shim.call("qk_timer_start", timer, None)
        launch()
        shim.call("qk_timer_stop", timer, None)
        ms = ctypes.c_float(0)
        shim.call("qk_timer_elapsed_ms", timer, ctypes.byref(ms))
        samples.append(ms.value)
    return samples[1:]


def bench_take(reps):
    """Random gather of 10 M int64 rows out of 1 M, 10 % source nulls and
    10 % NO_ROW. Useful bytes counted per index: 4 (idx) + 8 (src) + 8
    (dst) + 1/8 (bitmap out); the pair reads idx twice. The line traffic
    of the random source reads is not counted."""
    rng = np.random.default_rng(3)
    n = N_PROBE
    idx = rng.integers(0, N_BUILD, n).astype(np.uint32)
    src = DevColumn.from_numpy(rng.integers(-9, 9, N_BUILD).astype(np.int64))
    valid = DevColumn.from_numpy(ops.pack_valid(rng.random(N_BUILD) >= 0.1))
    didx = DevColumn.from_numpy(idx)
    idx[rng.random(n) < 0.1] = ops.NO_ROW
    didx_no = DevColumn.from_numpy(idx)
    dst = DevColumn(np.int64, n)
    out_valid = DevColumn(np.uint8, ops.valid_nbytes(n))
    cnt = DevColumn.from_numpy(np.zeros(1, dtype=np.uint64))
    timer = ctypes.c_void_p(0)
    shim.call("qk_timer_create", ctypes.byref(timer))

    def pair():
        shim.call("qk_gather_i64", None, c_u64(n), didx.ptr, src.ptr,
                  dst.ptr)
        shim.call("qk_valid_gather", None, c_u64(n), didx.ptr, valid.ptr,
                  out_valid.ptr, cnt.ptr)

    def fused(ix, bitmap):
        return lambda: shim.call(
            "qk_take_opt_i64", None, c_u64(n), ix.ptr, src.ptr,
            bitmap.ptr if bitmap else None, dst.ptr, out_valid.ptr, cnt.ptr)
    fused_bytes = n * (4 + 8 + 8) + n // 8
    variants = [("take_pair_gather_plus_valid_gather", pair,
                 fused_bytes + 4 * n),
                ("take_opt_bitmap", fused(didx, valid), fused_bytes),
                ("take_opt_bitmap_10pct_no_row", fused(didx_no, valid),
                 fused_bytes),
                ("take_opt_no_bitmap", fused(didx, None), fused_bytes)]
    for rnd in range(2):                    # A B C D A B C D: drift shows
        for name, launch, nbytes in variants:
            samples = _timed(timer, reps, launch)
            _report(name, samples, round=rnd, gbytes_per_s=round(
                nbytes / statistics.median(samples) / 1e6, 1))
    shim.call("qk_timer_destroy", timer)
    for c in (src, valid, didx, didx_no, dst, out_valid, cnt):
        c.free()


def bench_modes(reps, modes):
    rng = np.random.default_rng(N_BUILD)
    table = ops.JoinTable(N_BUILD)
    bcol = DevColumn.from_numpy(rng.permutation(N_BUILD).astype(np.int64))
    table.build(bcol)
    keys = DevColumn.from_numpy(
        rng.integers(0, 2 * N_BUILD, N_PROBE).astype(np.int64))
    pidx = DevColumn(np.uint32, N_PROBE)
    bidx = DevColumn(np.uint32, N_PROBE)
    cur = DevColumn.from_numpy(np.zeros(1, dtype=np.uint64))
    timer = ctypes.c_void_p(0)
    shim.call("qk_timer_create", ctypes.byref(timer))
    for rnd in range(2):
        for mode in modes:
            samples = _timed(timer, reps, lambda: shim.call(
                "qk_join_probe", None, c_u64(N_PROBE), keys.ptr,
                table.slot_keys.ptr, table.slot_head.ptr,
                table.chain_next.ptr, c_u64(table.cap), mode, pidx.ptr,
                bidx.ptr, c_u64(N_PROBE), cur.ptr))
            _report("probe_kernel_mode%d" % mode, samples, round=rnd)
    shim.call("qk_timer_destroy", timer)
    for c in (bcol, keys, pidx, bidx, cur):
        c.free()
    table.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true",
                    help="default paths only (runs on the parent commit)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["probe", "take", "modes"])
    args = ap.parse_args()
    shim.init(0)
    print(json.dumps({"package": os.path.dirname(ops.__file__)}), flush=True)
    want = lambda what: args.only in (None, what)           # noqa: E731
    if want("probe"):
        bench_probe(args.reps, "left", False, 0.0)
        bench_probe(args.reps, "inner", False, 0.0)
        if not args.baseline:
            bench_probe(args.reps, "left", True, 0.0)
            bench_probe(args.reps, "left", True, 0.1)
            bench_probe(args.reps, "inner", True, 0.0)
    if want("modes"):
        bench_modes(args.reps, (0, 1, 2) if args.baseline else (0, 1, 2, 3))
    if want("take") and not args.baseline:
        bench_take(args.reps)


if __name__ == "__main__":
    main()
