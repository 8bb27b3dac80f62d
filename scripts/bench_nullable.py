"""Measure what nullable columns cost on the device path.

For an i64 column of N rows (default 24M) written PLAIN and dictionary,
data page v1, uncompressed, at null fractions 0, 0.01 and 0.5:
  - the mask-mode decode (qk_pq_def_pages + dense value decode +
    qk_valid_expand), file bytes already in HBM, page plan built once
  - the existing non-null decode of the same values written non-nullable
Both are timed with HIP events around the whole column decode (as
bench_parquet.py's kernels-only figure; the mask-mode span includes the
copy-back of the small per-page table and the host prefix sum that sit
between its kernels). Then the JIT filter rate with one nullable input
against the same predicate on a non-null copy.
Run on a GPU box: python scripts/bench_nullable.py [rows]
Prints markdown table rows for profiles/nullable.md.
"""
import io
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quokka_amd import jit, ops, parquet_gpu as P, shim    # noqa: E402
from quokka_amd.shim import Timer                           # noqa: E402


def write(arr, dictionary):
    buf = io.BytesIO()
    pq.write_table(pa.table({"x": arr}), buf, compression="NONE",
                   use_dictionary=dictionary, data_page_version="1.0")
    return buf.getvalue()


def plan(raw, mask):
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    max_def = md.schema.column(0).max_definition_level
    chunks, row = [], 0
    for rg in range(md.num_row_groups):
        ch = P._Chunk(raw, md.row_group(rg).column(0), max_def, row,
                      mask=mask)
        row += ch.n
        chunks.append(ch)
    return chunks, row


def best_ms(fn, reps=5):
    timer = Timer()
    fn()
    ts = []
    for _ in range(reps):
        timer.start(None)
        fn()
        timer.stop(None)
        shim.call("qk_stream_sync", None)
        ts.append(timer.elapsed_ms())
    timer.destroy()
    return min(ts)


def time_decode(raw, mask):
    dev = P._upload(shim, raw)
    chunks, total = plan(raw, mask)
    decode = P._decode_masked if mask else P._decode_column

    def once():
        c = decode(shim, dev, chunks, total)
        shim.call("qk_stream_sync", None)
        c.free()

    ms = best_ms(once)
    dev.free()
    return ms


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
    shim.init(0)
    rng = np.random.default_rng(1)
    print("rows=%d" % n, flush=True)
    print("| encoding | null fraction | non-null decode ms | mask decode ms "
          "| ratio |")
    print("|---|---|---|---|---|")
    for enc, dictionary in (("PLAIN", False), ("dictionary", True)):
        vals = rng.integers(0, 1000, n) if dictionary else \
            rng.integers(-1 << 40, 1 << 40, n)
        schema = pa.schema([pa.field("x", pa.int64(), nullable=False)])
        raw0 = io.BytesIO()
        pq.write_table(pa.table({"x": vals}, schema=schema), raw0,
                       compression="NONE", use_dictionary=dictionary,
                       data_page_version="1.0")
        base = time_decode(raw0.getvalue(), False)
        for frac in (0.0, 0.01, 0.5):
            nulls = rng.random(n) < frac
            raw = write(pa.array(vals, mask=nulls, type=pa.int64()),
                        dictionary)
            ms = time_decode(raw, True)
            print("| %s | %.2f | %.3f | %.3f | %.2f |"
                  % (enc, frac, base, ms, ms / base), flush=True)

    # JIT filter: one nullable input vs the same predicate on a non-null
    # copy (the u8 validity flag adds 1 byte per row of traffic, plus the
    # qk_valid_to_u8 pass that fills it)
    vals = rng.integers(-1000, 1000, n)
    mask = rng.random(n) >= 0.01
    plain = shim.DevColumn.from_numpy(np.where(mask, vals, 0))
    nullable = ops.NullableColumn.from_numpy(vals, mask)
    schema = {"x": np.dtype(np.int64)}
    f0 = jit.JitFilter("x > 0", schema)
    f1 = jit.JitFilter("x > 0", schema, nullable=("x",))

    def run(f, col):
        idx, _ = f.run({"x": col})
        idx.free()

    t0 = best_ms(lambda: run(f0, plain))
    t1 = best_ms(lambda: run(f1, nullable))
    print()
    print("| JIT filter `x > 0` | ms | Grows/s |")
    print("|---|---|---|")
    print("| non-null input | %.3f | %.2f |" % (t0, n / t0 / 1e6))
    print("| nullable input | %.3f | %.2f |" % (t1, n / t1 / 1e6))
    print("ratio %.2f" % (t1 / t0))


if __name__ == "__main__":
    main()
