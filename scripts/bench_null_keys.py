"""Null keys (DESIGN.md §3a'''): what the opt-in costs and that the
defaults did not move. Workloads of profiles/wide_keys.md:

  groupby  ops.GroupByKeys.update, 10 M rows, two int keys, one SUM, at
           1 k and 1 M groups: first call (every group new) and second call
           on the same batch (every group exists)
  probe    ops.JoinTable.probe (inner), 10 M rows against 1 M built keys
  prepare  qk_key_null_words alone, device timer, for its bandwidth

--baseline runs only what exists without the null-key arguments, so the
same script measures the parent commit (run it with the parent's tree
first on PYTHONPATH). Prints one JSON line per measurement: median, min and
max over --reps fresh tables, in ms.
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
from quokka_amd.shim import DevColumn, c_u64                # noqa: E402

N = 10_000_000


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


def _masks(rng, frac):
    """Two host masks with `frac` nulls, or None for the plain path."""
    if frac is None:
        return None
    return [rng.random(N) >= frac, rng.random(N) >= frac]


def bench_groupby(groups, reps, nullable, frac):
    rng = np.random.default_rng(groups)
    side = int(round(groups ** 0.5))
    ka = rng.integers(0, side, N).astype(np.int64)
    kb = rng.integers(0, groups // side, N).astype(np.int64)
    cols = [DevColumn.from_numpy(ka), DevColumn.from_numpy(kb)]
    val = DevColumn.from_numpy(rng.random(N))
    masks = _masks(rng, frac)
    bitmaps = None
    if masks is not None:       # device bitmaps: the upload is not timed
        bitmaps = [DevColumn.from_numpy(ops.pack_valid(m)) for m in masks]
    kw = {"nullable_keys": True} if nullable else {}
    first, second = [], []
    for _ in range(reps + 1):               # the first round is warm-up
        gb = ops.GroupByKeys(2, 1, expected_groups=2 * groups, **kw)
        ukw = {"key_valid": bitmaps} if bitmaps is not None else {}
        a = _ms(lambda: gb.update(cols, [val], N, **ukw))
        b = _ms(lambda: gb.update(cols, [val], N, **ukw))
        first.append(a)
        second.append(b)
        ngroups = gb.n_groups
        gb.free()
    tag = "groupby_%s_%s" % (
        "1k" if groups < 10_000 else "1M",
        "nullable_%dpct" % round(100 * frac) if nullable else "plain")
    _report(tag + "_new", first[1:], groups=int(ngroups))
    _report(tag + "_existing", second[1:], groups=int(ngroups))
    for c in cols + [val] + (bitmaps or []):
        c.free()


def bench_probe(reps, frac):
    rng = np.random.default_rng(3)
    nb = 1_000_000
    bk = rng.permutation(nb).astype(np.int64) * 3
    pk = rng.integers(0, 2 * nb, N).astype(np.int64) * 3    # half match
    jt = ops.JoinTable(nb)
    bcol = DevColumn.from_numpy(bk)
    jt.build(bcol)
    pcol = DevColumn.from_numpy(pk)
    kw = {}
    if frac is not None:
        kw["valid"] = DevColumn.from_numpy(
            ops.pack_valid(rng.random(N) >= frac))
    samples, matches = [], 0

    def run():
        nonlocal matches
        pidx, bidx, matches = jt.probe(pcol, mode=0, **kw)
        pidx.free()
        bidx.free()
    for _ in range(reps + 1):
        samples.append(_ms(run))
    _report("probe_%s" % ("plain" if frac is None
                          else "valid_%dpct" % round(100 * frac)),
            samples[1:], matches=int(matches))
    for c in (bcol, pcol) + tuple(kw.values()):
        c.free()
    jt.free()


def bench_prepare(reps, frac):
    """qk_key_null_words on two nullable keys: 2 x (8 B key read + 8 B
    canonical write) + 8 B null word + the bitmaps per row."""
    rng = np.random.default_rng(4)
    cols = [DevColumn.from_numpy(rng.integers(0, 1000, N).astype(np.int64))
            for _ in range(2)]
    bitmaps = [DevColumn.from_numpy(ops.pack_valid(m))
               for m in _masks(rng, frac)]
    canon = [DevColumn(np.int64, N) for _ in range(2)]
    nullw = [DevColumn(np.int64, N)]
    arrays = [DevColumn.from_numpy(np.array([c.ptr.value for c in group],
                                            dtype=np.uint64))
              for group in (cols, bitmaps, canon, nullw)]
    timer = ctypes.c_void_p(0)
    shim.call("qk_timer_create", ctypes.byref(timer))
    samples = []
    for _ in range(reps + 1):
        shim.call("qk_timer_start", timer, None)
        shim.call("qk_key_null_words", None, c_u64(N), 2,
                  *[a.ptr for a in arrays])
        shim.call("qk_timer_stop", timer, None)
        ms = ctypes.c_float(0)
        shim.call("qk_timer_elapsed_ms", timer, ctypes.byref(ms))
        samples.append(ms.value)
    nbytes = N * (2 * 16 + 8) + 2 * (N // 8)
    med = statistics.median(samples[1:])
    _report("prepare_%dpct" % round(100 * frac), samples[1:],
            bytes_per_row=nbytes / N,
            tb_per_s=round(nbytes / med / 1e9, 3),
            of_6p3=round(nbytes / med / 1e9 / 6.3, 3))
    shim.call("qk_timer_destroy", timer)
    for c in cols + bitmaps + canon + nullw + arrays:
        c.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true",
                    help="default paths only (runs on the parent commit)")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    shim.init(0)
    for groups in (1024, 1 << 20):
        bench_groupby(groups, args.reps, False, None)
    bench_probe(args.reps, None)
    if args.baseline:
        return
    for groups in (1024, 1 << 20):
        for frac in (0.0, 0.1):
            bench_groupby(groups, args.reps, True, frac)
    for frac in (0.0, 0.1):
        bench_probe(args.reps, frac)
        bench_prepare(args.reps, frac)


if __name__ == "__main__":
    main()
