"""Device LIKE over an o_comment-shaped string column: kernels-only rates.

Generates random-word comments of 19-78 bytes with the
'special ... requests' phrase planted in ~1.9 % of the rows (the fraction
oracle/tpch_gen.py uses for o_comment_special), then times
'%special%requests%', 'forest%' and '%BRASS' with HIP events after
warm-up (median of --runs), once through the LDS-staged path and once
through the direct-global path (the A/B), and pyarrow.compute.match_like on the same
bytes on the host CPU.

  python scripts/bench_like.py --rows 20000000 --runs 15

Rates are over algorithmic bytes: offsets + string bytes + 1 B/row out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12   # B/s, the achievable-HBM figure README uses
PATTERNS = ["%special%requests%", "forest%", "%BRASS"]


def gen_comments(n, seed):
    """-> pyarrow string array built from numpy buffers (no per-row
    Python): each row is a random run of a word-salad text, 19-78 bytes."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    words = ("furiously quickly carefully slyly blithely final regular "
             "express pending ironic bold even silent deposits accounts "
             "packages theodolites instructions foxes pinto beans platelets "
             "ideas asymptotes dependencies excuses").split()
    salad = " ".join(words[i] for i in rng.integers(0, len(words), 200000))
    salad = np.frombuffer(salad.encode(), dtype=np.uint8)
    # one block of up to 2^20 distinct rows, repeated to n rows (keeps
    # the host generation cheap; every repeat is its own device memory)
    n0 = min(n, 1 << 20)
    lens0 = rng.integers(19, 79, n0)
    off0 = np.zeros(n0 + 1, dtype=np.int64)
    np.cumsum(lens0, out=off0[1:])
    start = rng.integers(0, len(salad) - 80, n0)
    idx = np.arange(off0[-1]) - np.repeat(off0[:-1] - start, lens0)
    data0 = salad[idx]
    # plant 'special <word> requests' at the row start in ~1.9 % of rows
    phrase = np.frombuffer(b"special pack requests", dtype=np.uint8)
    hit = np.nonzero((rng.random(n0) < 0.019) & (lens0 >= len(phrase)))[0]
    pos = off0[hit][:, None] + np.arange(len(phrase))[None, :]
    data0[pos.reshape(-1)] = np.tile(phrase, len(hit))
    reps = -(-n // n0)
    lens = np.tile(lens0, reps)[:n]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    data = np.tile(data0, reps)[:off[-1]]
    arr = pa.Array.from_buffers(
        pa.large_string(), n,
        [None, pa.py_buffer(off), pa.py_buffer(data)])
    return arr.cast(pa.string()) if off[-1] < 2 ** 31 else arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    assert args.runs >= 10

    import pyarrow.compute as pc
    from quokka_amd import ops, shim
    from quokka_amd.shim import DevColumn, c_u64

    shim.init(0)
    arr = gen_comments(args.rows, args.seed)
    n = len(arr)
    sc = ops.StringColumn.from_arrow(arr)
    width = sc.offsets.dtype.itemsize
    nbytes = sc.data.nbytes
    algo = (n + 1) * width + nbytes + n
    sfx = "i64" if width == 8 else "i32"
    out = DevColumn(np.uint8, n)
    timer = shim.Timer()
    print(json.dumps({"rows": n, "string_bytes": nbytes,
                      "offset_width": width, "algorithmic_bytes": algo,
                      "lds_tile": shim.LIKE_TILE}))

    for p in PATTERNS:
        pat = shim.like_compile(p)
        res = {"pattern": p}
        flags = {}
        fn = "qk_str_like_path_" + sfx
        for label, stage in (("lds", 1), ("direct", 0)):
            ms = []
            for it in range(args.warmup + args.runs):
                timer.start(None)
                shim.call(fn, None, c_u64(n), sc.offsets.ptr, sc.data.ptr,
                          ctypes.byref(pat), 0, stage, out.ptr)
                timer.stop(None)
                shim.call("qk_stream_sync", None)
                if it >= args.warmup:
                    ms.append(timer.elapsed_ms())
            med = statistics.median(ms)
            flags[label] = out.to_numpy(n)
            res[label] = {"median_ms": round(med, 4),
                          "min_ms": round(min(ms), 4),
                          "max_ms": round(max(ms), 4),
                          "rows_per_s": round(n / (med * 1e-3)),
                          "GB_per_s": round(algo / (med * 1e-3) / 1e9, 1),
                          "frac_hbm": round(algo / (med * 1e-3)
                                            / HBM_ACHIEVABLE, 3)}
        t0 = time.perf_counter()
        cpu = pc.match_like(arr, p)
        cpu_s = time.perf_counter() - t0
        cpu = np.asarray(cpu).astype(np.uint8)
        res["selected"] = int(cpu.sum())
        res["equal_lds_cpu"] = bool(np.array_equal(flags["lds"], cpu))
        res["equal_direct_cpu"] = bool(np.array_equal(flags["direct"], cpu))
        res["pyarrow_match_like"] = {
            "ms": round(cpu_s * 1e3, 2),
            "rows_per_s": round(n / cpu_s),
            "GB_per_s": round(algo / cpu_s / 1e9, 2)}
        res["lds_speedup_over_direct"] = round(
            res["direct"]["median_ms"] / res["lds"]["median_ms"], 3)
        # what qk_str_like_* itself picks for this pattern
        anchored = pat.anchor_start + pat.anchor_end
        res["default_path"] = "lds" if pat.nseg > anchored else "direct"
        print(json.dumps(res))
    timer.destroy()
    out.free()
    sc.free()


if __name__ == "__main__":
    main()
