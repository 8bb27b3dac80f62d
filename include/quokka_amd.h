/* quokka_amd — C ABI of the MI355X-native columnar execution path.
 *
 * This is the drop-in boundary beneath the reference's (marsupialtail/quokka)
 * Executor / partition-function plugin API. The reference is pure Python
 * (pyquokka/executors/base_executor.py:26-32 `Executor.execute/done`,
 * pyquokka/core.py:152-195 `partition_fn`) delegating all arithmetic to
 * polars/duckdb; this library replaces exactly that arithmetic with HIP
 * kernels for gfx950. The Python classes in quokka_amd/executors.py bind
 * these entry points via ctypes and present the reference's own interface
 * (same names / argument meaning / error behaviour); see INTEGRATION.md for
 * the binding a pyquokka maintainer would add.
 *
 * Conventions:
 *  - every function returns 0 on success, nonzero HIP/ABI error code;
 *    qk_last_error() returns a static string for the calling thread's last
 *    failure. No function falls back to CPU: with no usable GPU, calls fail.
 *  - `stream` is an opaque HIP stream handle from qk_stream_create (NULL =
 *    default stream). All kernel entry points are asynchronous on `stream`.
 *  - device pointers are void* from qk_dmalloc; columns are dense device
 *    arrays (no nulls — the reference's TPC-H hot path has none).
 *  - dates are int32 days since 1970-01-01 (Arrow date32), strings are
 *    host-side dictionary codes (u8), matching the staging layer.
 */
#ifndef QUOKKA_AMD_H
#define QUOKKA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- context ------------------------------------------------------- */
int qk_init(int device);                 /* set + warm the HIP device      */
int qk_device_count(int *out);
const char *qk_last_error(void);
const char *qk_build_arch(void);         /* "gfx950"                       */

/* ---- device memory -------------------------------------------------- */
int qk_dmalloc(uint64_t nbytes, void **dptr);
int qk_hmalloc_impl(uint64_t nbytes, void **hptr); /* pinned host memory */
int qk_hfree(void *hptr);                          /* free pinned memory */
int qk_dfree(void *dptr);
int qk_h2d(void *dst_dev, const void *src_host, uint64_t nbytes);
int qk_d2h(void *dst_host, const void *src_dev, uint64_t nbytes);
/* Async variants on a stream; src/dst host memory must be PINNED
 * (qk_hmalloc_impl) or the copy silently degrades to staged+sync. Used
 * by the double-buffered staging bounce (shim._PinnedBounce): host
 * memmove of chunk k+1 overlaps the DMA of chunk k on alternating
 * streams. */
int qk_h2d_async(void *stream, void *dst_dev, const void *src_host,
                 uint64_t nbytes);
int qk_d2h_async(void *stream, void *dst_host, const void *src_dev,
                 uint64_t nbytes);
int qk_dmemset(void *dst_dev, int value, uint64_t nbytes);
int qk_fill_i64(void *stream, int64_t *dst_dev, int64_t value, uint64_t n);

/* ---- streams & timing ----------------------------------------------- */
int qk_stream_create(void **stream);
int qk_stream_destroy(void *stream);
int qk_stream_sync(void *stream);
/* Bare (non-timing) HIP events for cross-stream ordering: the overlapped
 * shuffle records an event on the comm stream after each received chunk and
 * the compute stream waits on it before probing that chunk (north_star:
 * RCCL repartition overlapped with probe on a side HIP stream; replaces the
 * reference's 8-thread Flight do_put pool overlap, core.py:324-371). */
int qk_event_create(void **ev);
int qk_event_destroy(void *ev);
int qk_event_record(void *ev, void *stream);
int qk_stream_wait_event(void *stream, void *ev);
/* HIP-event timer pair on the launching stream (roofline measurement). */
int qk_timer_create(void **timer);
int qk_timer_destroy(void *timer);
int qk_timer_start(void *timer, void *stream);
int qk_timer_stop(void *timer, void *stream);
int qk_timer_elapsed_ms(void *timer, float *out_ms);   /* syncs the stop event */

/* ---- synthetic data (bench only; distributions = oracle/tpch_gen.py) */
/* Fill lineitem columns for rows [row_offset, row_offset+n) with the TPC-H
 * distributions of oracle/tpch_gen.py (counter-based RNG: value depends only
 * on (seed, global row)). Any output pointer may be NULL to skip a column.
 * n_parts/n_suppliers/n_orders scale key ranges (pass tpch_gen values). */
int qk_gen_lineitem(void *stream, uint64_t n, uint64_t row_offset, uint64_t seed,
                    int64_t n_parts, int64_t n_suppliers, int64_t n_orders,
                    int64_t *l_orderkey, int64_t *l_suppkey,
                    double *l_quantity, double *l_extendedprice,
                    double *l_discount, double *l_tax,
                    uint8_t *l_returnflag, uint8_t *l_linestatus,
                    int32_t *l_shipdate, int32_t *l_commitdate,
                    int32_t *l_receiptdate);

/* Orders columns for rows [row_offset, row_offset+n): o_orderkey SPARSE
 * per TPC-H spec 4.2.3 (8 keys per 32-key bucket, = oracle/tpch_gen
 * sparse_orderkeys), o_custkey uniform 1..n_customers with the spec's
 * custkey%3 != 0 mortality hole, o_orderdate uniform spec range,
 * o_shippriority 0. Consistent with qk_gen_lineitem's l_orderkey (order
 * row = lineitem row/4: every order has exactly 4 lines). */
/* o_orderpriority: uniform u8 code 0..4; o_totalprice: derived from the
 * order's 4 lines by re-deriving their qty/partkey/disc/tax with
 * qk_gen_lineitem's counter-based formulas (pass the same li_n_parts). */
int qk_gen_orders(void *stream, uint64_t n, uint64_t row_offset, uint64_t seed,
                  int64_t n_customers, int64_t *o_orderkey, int64_t *o_custkey,
                  int32_t *o_orderdate, int32_t *o_shippriority,
                  uint8_t *o_orderpriority, double *o_totalprice,
                  int64_t li_n_parts);
/* Customer columns: c_custkey dense row+1, c_mktsegment uniform u8 0..4,
 * c_nationkey uniform i32 0..24. Any output may be NULL. */
int qk_gen_customer(void *stream, uint64_t n, uint64_t row_offset,
                    uint64_t seed, int64_t *c_custkey, uint8_t *c_mktsegment,
                    int32_t *c_nationkey);
/* Supplier columns: s_suppkey dense row+1, s_nationkey uniform 0..24. */
int qk_gen_supplier(void *stream, uint64_t n, uint64_t row_offset,
                    uint64_t seed, int64_t *s_suppkey, int32_t *s_nationkey);
/* Aux independent-draw column generator (device mirror of
 * oracle/tpch_gen.py's independent columns). mode 0: out_u8 = uniform
 * code in [0,a) (l_shipmode, tpch_gen:231). mode 1: out_u8 = bernoulli
 * flag, P = a/1e6 (o_comment_special, tpch_gen:165). mode 2: out_f64 =
 * uniform cents in [a,b] / 100 (c_acctbal, tpch_gen:250). */
int qk_gen_aux(void *stream, uint64_t n, uint64_t row_offset, uint64_t seed,
               uint64_t salt, int mode, int64_t a, int64_t b,
               uint8_t *out_u8, double *out_f64);

/* ---- TPC-H Q1: fused filter + group-by partial aggregate ------------- *
 * Replaces the map-side partial agg the reference folds into partition_fn
 * (pyquokka/core.py:173-176 + df.py:1354-1394: per-batch DuckDB
 * "SUM/COUNT group by l_returnflag,l_linestatus") and the probe-side concat
 * of SQLAggExecutor.execute (sql_executors.py:587-590), in one pass.
 * out_dev = device f64[6 groups][8]:
 *   [sum_qty, sum_base_price, sum_disc_price, sum_charge, sum_disc, count,
 *    pad, pad]; group id = l_returnflag*2 + l_linestatus.
 * ACCUMULATES into out_dev (caller zeroes once; repeated calls = executor
 * state accumulation across batches, sql_executors.py:587-590). */
int qk_q1_agg(void *stream, uint64_t n,
              const int32_t *l_shipdate, const double *l_quantity,
              const double *l_extendedprice, const double *l_discount,
              const double *l_tax, const uint8_t *l_returnflag,
              const uint8_t *l_linestatus, int32_t cutoff_date,
              double *out_dev /* f64[48] */);
/* Shape of the qk_q1_agg streaming kernel, for tests that need its edges:
 * rows per block tile (returns the size, not an error code), and the
 * number of blocks of one launch over a large input on the current device
 * (blocks x tile rows = rows of one full grid sweep). */
int qk_q1_tile_rows(void);
int qk_q1_grid_blocks(int *out);
/* Launch shape of the generic operators (sort, partition, join, group-by),
 * for tests that need its edges: threads per block and the block cap of one
 * launch (both return the size, not an error code). Up to
 * qk_block_threads() * qk_max_blocks() rows qk_sort_pairs_u64 and
 * qk_partition_scatter give each block one tile of qk_block_threads() rows;
 * above it a block loops over several tiles. */
int qk_block_threads(void);
int qk_max_blocks(void);

/* ---- TPC-H Q6: fused filter + sum ------------------------------------ *
 * tpch_ref.py:171-183 semantics. out_dev = f64[2] {sum_revenue, count};
 * accumulates like qk_q1_agg. Bounds are the exact f64 constants of the
 * reference SQL expressions. */
int qk_q6_agg(void *stream, uint64_t n,
              const int32_t *l_shipdate, const double *l_quantity,
              const double *l_extendedprice, const double *l_discount,
              int32_t date_lo, int32_t date_hi,
              double disc_lo, double disc_hi, double qty_hi,
              double *out_dev /* f64[2] */);

/* ---- generic filter: compare + compaction ----------------------------- *
 * Replaces the predicate filter of partition_fn (core.py:170, polars
 * DataFrame.filter) for single-column compares; emits the ORDERED indices
 * of passing rows (row order preserved, as polars filter does).
 * op: 0 '<', 1 '<=', 2 '>', 3 '>=', 4 '==', 5 '!='.
 * out_count_dev: device u64, set to number of passing rows (must be zeroed).
 * out_idx capacity must be >= n. */
int qk_filter_i32(void *stream, uint64_t n, const int32_t *col, int op,
                  int32_t value, uint32_t *out_idx, uint64_t *out_count_dev);
int qk_filter_u8(void *stream, uint64_t n, const uint8_t *col, int op,
                 uint8_t value, uint32_t *out_idx, uint64_t *out_count_dev);
/* f64 variant; threshold is a kernel argument (no JIT literal). */
int qk_filter_f64(void *stream, uint64_t n, const double *col, int op,
                  double value, uint32_t *out_idx, uint64_t *out_count_dev);

/* elementwise revenue: out[i] = a[i] * (1 - b[i]) (the per-row product the
 * reference computes before summing, apps/tpc-h/tpch.py:151) */
int qk_flag_gt_i32(void *stream, uint64_t n, const int32_t *a,
                   const int32_t *b, double *out); /* out=a>b?1:0 (Q21) */
int qk_mul_1md(void *stream, uint64_t n, const double *a, const double *b,
               double *out);

/* gather: dst[i] = src[idx[i]] (column compaction / join payload gather) */
int qk_gather_i64(void *stream, uint64_t n_idx, const uint32_t *idx,
                  const int64_t *src, int64_t *dst);
int qk_gather_f64(void *stream, uint64_t n_idx, const uint32_t *idx,
                  const double *src, double *dst);
int qk_gather_i32(void *stream, uint64_t n_idx, const uint32_t *idx,
                  const int32_t *src, int32_t *dst);
int qk_gather_u8(void *stream, uint64_t n_idx, const uint32_t *idx,
                 const uint8_t *src, uint8_t *dst);

/* ---- hash join build / probe (i64 keys) ------------------------------- *
 * Replaces BuildProbeJoinExecutor (sql_executors.py:325-377): build side =
 * stream 1 (vstacked state), probe = stream 0, how in {inner,semi,anti}
 * (left via inner + host fill, or on the device in probe mode 3).
 * Open-addressing table, linear probing,
 * capacity a power of two >= 2x build rows. Duplicate build keys chain
 * through chain_next. slot_keys must be pre-filled with QK_JOIN_EMPTY
 * (qk_fill_i64), slot_head with -1 bytes (qk_dmemset 0xff).
 * Build may be called repeatedly (batch accumulation): build_row_offset is
 * added to local row indices so chains index the concatenated build side.
 * PRECONDITION: QK_JOIN_EMPTY marks a free slot, so no BUILD key (and no
 * group key of qk_groupby_i64_sum) may equal it: such a row would match the
 * first free slot without claiming it, and a later key that claims the slot
 * inherits its chain (or its sums). The kernels do not check; callers with
 * host keys reject it before staging (quokka_amd.ops.check_no_sentinel_key).
 * PROBE keys may take any value: a probe for QK_JOIN_EMPTY stops at the
 * first free slot, whose head is -1, and reports no match. */
#define QK_JOIN_EMPTY INT64_MIN
int qk_join_build(void *stream, uint64_t n_build, const int64_t *keys,
                  uint32_t build_row_offset, int64_t *slot_keys,
                  int32_t *slot_head, int32_t *chain_next, uint64_t capacity);
/* mode: 0 = inner (emit probe_idx,build_idx pairs), 1 = semi (probe_idx
 * only), 2 = anti (probe_idx only), 3 = left: inner, plus one pair
 * (probe_idx, QK_NO_ROW) for every probe row without a match, so a row
 * with d matches appears max(1, d) times. out_cursor_dev (u64, zeroed)
 * returns the TOTAL pair count even when it exceeds out_capacity (no silent
 * truncation: caller re-runs with larger buffers when cursor > capacity).
 * QK_NO_ROW is the build index of "no build row". Build rows are int32
 * chain indices, so no real row reaches it. Modes 0 and 3 need
 * out_build_idx. */
#define QK_NO_ROW 0xFFFFFFFFu
int qk_join_probe(void *stream, uint64_t n_probe, const int64_t *keys,
                  const int64_t *slot_keys, const int32_t *slot_head,
                  const int32_t *chain_next, uint64_t capacity, int mode,
                  uint32_t *out_probe_idx, uint32_t *out_build_idx,
                  uint64_t out_capacity, uint64_t *out_cursor_dev);
/* The same join over a NULLABLE key column: valid_dev is the column's
 * validity bitmap (layout under "nullable columns" below), and a NULL key
 * matches nothing on either side, as in the reference's polars join
 * (sql_executors.py:371). The key word under a null is never read, so it
 * may hold anything, QK_JOIN_EMPTY included; the precondition above binds
 * valid build keys only.
 * Build: a null row takes no slot and no chain link but keeps its row
 * number build_row_offset + i, so the caller still advances its build
 * count by n_build and build indices keep addressing the payload columns.
 * Probe: a null row is a miss decided without a walk: nothing in mode 0
 * and 1, emitted in mode 2, emitted once with QK_NO_ROW in mode 3.
 * Everything else as qk_join_build /
 * qk_join_probe, which remain the entry points for columns without a
 * bitmap. */
int qk_join_build_valid(void *stream, uint64_t n_build, const int64_t *keys,
                        const uint64_t *valid_dev, uint32_t build_row_offset,
                        int64_t *slot_keys, int32_t *slot_head,
                        int32_t *chain_next, uint64_t capacity);
int qk_join_probe_valid(void *stream, uint64_t n_probe, const int64_t *keys,
                        const uint64_t *valid_dev, const int64_t *slot_keys,
                        const int32_t *slot_head, const int32_t *chain_next,
                        uint64_t capacity, int mode, uint32_t *out_probe_idx,
                        uint32_t *out_build_idx, uint64_t out_capacity,
                        uint64_t *out_cursor_dev);

/* ---- fused Q3 path ---------------------------------------------------- *
 * Filter + semi-join + build and filter + probe + group-by aggregate fused
 * into single passes (the reference folds filters and per-batch partial
 * aggs into partition_fn the same way, core.py:152-195 + df.py:1354-1394).
 * Build keys must be UNIQUE (orders/customer primary keys); slot_head
 * stores the build ROW index; the orders table's slots double as group-by
 * slots for the probe aggregate. Tables pre-filled like qk_join_build's. */
int qk_build_u8eq(void *stream, uint64_t n, const int64_t *keys,
                  const uint8_t *flag, uint8_t flag_val, int64_t *slot_keys,
                  int32_t *slot_head, uint64_t capacity, uint32_t *bloom,
                  uint64_t bloom_mask);
/* bloom/bloom_mask (nullable/0): optional Bloom prefilter the probe-side
 * kernels test before the table walk (bits = pow2, mask = bits-1). */
int qk_q3_build_orders(void *stream, uint64_t n, const int64_t *o_orderkey,
                       const int64_t *o_custkey, const int32_t *o_orderdate,
                       int32_t date_lt, const int64_t *cust_keys,
                       const int32_t *cust_head, uint64_t cust_cap,
                       int64_t *slot_keys, int32_t *slot_head,
                       uint64_t capacity, uint32_t *bloom,
                       uint64_t bloom_mask, const uint32_t *cust_bloom,
                       uint64_t cust_bloom_mask);
/* Count the rows qk_q3_build_orders would insert (for tight table sizing;
 * count_dev u64, zeroed). */
int qk_q3_count_orders(void *stream, uint64_t n, const int64_t *o_custkey,
                       const int32_t *o_orderdate, int32_t date_lt,
                       const int64_t *cust_keys, const int32_t *cust_head,
                       uint64_t cust_cap, uint64_t *count_dev,
                       const uint32_t *cust_bloom, uint64_t cust_bloom_mask);
int qk_q3_probe_agg(void *stream, uint64_t n, const int64_t *l_orderkey,
                    const int32_t *l_shipdate, const double *l_price,
                    const double *l_disc, int32_t date_gt,
                    const int64_t *slot_keys, const int32_t *slot_head,
                    uint64_t capacity, double *slot_sums /* f64[capacity],
                    zeroed; groups keyed by slot */,
                    uint64_t *match_count_dev /* nullable, zeroed u64 */);
/* Non-temporal-load variant of qk_q3_probe_agg: streams the lineitem
 * columns without polluting the caches so the build table stays resident
 * (same results; perf variant, A/B-measured in profiles/). */
int qk_q3_probe_agg_nt(void *stream, uint64_t n, const int64_t *l_orderkey,
                       const int32_t *l_shipdate, const double *l_price,
                       const double *l_disc, int32_t date_gt,
                       const int64_t *slot_keys, const int32_t *slot_head,
                       uint64_t capacity, double *slot_sums,
                       uint64_t *match_count_dev, const uint32_t *bloom,
                       uint64_t bloom_mask);
/* 4-rows-per-lane ILP variant: doubles the independent bloom/table load
 * chains per lane (the probe is random-load latency-bound at full
 * occupancy — r01 stall anatomy); same results, A/B in profiles/r02. */
int qk_q3_probe_agg_nt4(void *stream, uint64_t n, const int64_t *l_orderkey,
                        const int32_t *l_shipdate, const double *l_price,
                        const double *l_disc, int32_t date_gt,
                        const int64_t *slot_keys, const int32_t *slot_head,
                        uint64_t capacity, double *slot_sums,
                        uint64_t *match_count_dev, const uint32_t *bloom,
                        uint64_t bloom_mask);
/* Emit (orderkey, orders_build_row, revenue) for slots with sum != 0.
 * cursor (u64, zeroed) = group count (counted even past out_cap). */
int qk_q3_extract(void *stream, const int64_t *slot_keys,
                  const int32_t *slot_head, const double *slot_sums,
                  uint64_t capacity, int64_t *out_keys, int32_t *out_row,
                  double *out_sums, uint64_t out_cap, uint64_t *cursor_dev);

/* ---- fused Q5 path ----------------------------------------------------- *
 * Key -> i32-value hash tables and a fused lineitem probe for the 6-table
 * chain (tpch_ref.py:142-169). Unique build keys (primary keys). */
/* Insert keys[i] -> vals[i] where bit vals[i] of accept_mask is set
 * (accept_mask = 0xFFFFFFFF accepts all; else vals must be in [0,32)). */
int qk_build_keyval_i32(void *stream, uint64_t n, const int64_t *keys,
                        const int32_t *vals, uint32_t accept_mask,
                        int64_t *slot_keys, int32_t *slot_val,
                        uint64_t capacity, uint32_t *bloom,
                        uint64_t bloom_mask);
/* Orders in [date_lo, date_hi) whose o_custkey hits the customer table:
 * insert o_orderkey -> customer nationkey. slot_keys == NULL -> count-only
 * (count_dev gets the survivor count either way when non-NULL). */
int qk_q5_build_orders(void *stream, uint64_t n, const int64_t *o_orderkey,
                       const int64_t *o_custkey, const int32_t *o_orderdate,
                       int32_t date_lo, int32_t date_hi,
                       const int64_t *cust_keys, const int32_t *cust_val,
                       uint64_t cust_cap, int64_t *slot_keys,
                       int32_t *slot_val, uint64_t capacity,
                       uint64_t *count_dev, uint32_t *bloom,
                       uint64_t bloom_mask, const uint32_t *cust_bloom,
                       uint64_t cust_bloom_mask);
/* Fused probe: join lineitem to orders (-> customer nation) and supplier
 * (-> supplier nation); where equal accumulate revenue into out25[nation].
 * out25: f64[32], zeroed (slots 25..31 unused). */
int qk_q5_probe_agg(void *stream, uint64_t n, const int64_t *l_orderkey,
                    const int64_t *l_suppkey, const double *l_price,
                    const double *l_disc, const int64_t *ord_keys,
                    const int32_t *ord_val, uint64_t ord_cap,
                    const int64_t *supp_keys, const int32_t *supp_val,
                    uint64_t supp_cap, double *out25,
                    uint64_t *match_count_dev /* nullable */);

/* Non-temporal-load variant of qk_q5_probe_agg (see qk_q3_probe_agg_nt). */
int qk_q5_probe_agg_nt(void *stream, uint64_t n, const int64_t *l_orderkey,
                       const int64_t *l_suppkey, const double *l_price,
                       const double *l_disc, const int64_t *ord_keys,
                       const int32_t *ord_val, uint64_t ord_cap,
                       const int64_t *supp_keys, const int32_t *supp_val,
                       uint64_t supp_cap, double *out25,
                       uint64_t *match_count_dev, const uint32_t *bloom,
                       uint64_t bloom_mask);

/* ---- group-by (i64 key) sum ------------------------------------------- *
 * Replaces SQLAggExecutor's DuckDB group-by (sql_executors.py:592-599) for
 * distributive SUM over an i64 key (the post-rewrite partial form,
 * sql_utils.py:299-413). Open-addressing accumulate table; slot_keys
 * pre-filled with QK_JOIN_EMPTY (so no key may equal it, see
 * QK_JOIN_EMPTY above), slot_sums zeroed. Repeated calls
 * accumulate. nvals value columns share one key lookup (vals/slot_sums are
 * arrays-of-columns, each `capacity` doubles: slot_sums[c*capacity+slot]). */
/* agg_ops_dev (device i32[nvals], nullable -> all SUM): per value column
 * 0 = SUM (slot init 0), 1 = MIN (init +inf), 2 = MAX (init -inf) — the
 * distributive ops the two-phase rewrite emits (sql_utils.py:299-413). */
/* n_inserted_dev (u64, nullable): incremented once per NEW group claimed —
 * the host reads it after each batch and rebuilds into a larger table
 * before cumulative distinct keys approach capacity (the find-or-insert
 * probe loop would otherwise spin forever on a full table). */
int qk_groupby_i64_sum(void *stream, uint64_t n, const int64_t *keys,
                       const void *vals_dev /* dev double*[nvals] */,
                       const int32_t *agg_ops_dev /* NULL = all SUM */,
                       int nvals, int rstride /* pow2 words/slot >= 1+nvals */,
                       int64_t *table, uint64_t cap, uint64_t *n_inserted);
/* Initialize an INTERLEAVED group-by table: every slot record =
 * [key=EMPTY | v0..v(nvals-1) = inits[c] | pad] of rstride 8-byte words
 * (pow2 so a record never straddles a 128 B HBM line: find-or-insert
 * touches ONE random line per row, not one per array). */
int qk_groupby_init(void *stream, int64_t *table, uint64_t cap, int rstride,
                    int nvals, const double *inits_dev);
int qk_fill_f64(void *stream, double *dst_dev, double value, uint64_t n);
/* Compact occupied slots to out_keys/out_sums (unordered); out_cursor_dev
 * (u64, zeroed) = number of groups. out capacity must be >= group count. */
int qk_groupby_extract(void *stream, const int64_t *table, int rstride,
                       int nvals, uint64_t cap, int64_t *out_keys,
                       double *out_sums /* column-major, stride out_cap */,
                       uint64_t out_cap, uint64_t *cursor);
/* Thresholded extract: only groups whose sums[col] > threshold are
 * compacted (HAVING clauses, e.g. Q18's sum(l_quantity) > 300 over
 * ~n_orders groups — d2h of only the qualifying handful). */
int qk_groupby_extract_gt(void *stream, const int64_t *table, int rstride,
                          int nvals, uint64_t cap, int col, double threshold,
                          int64_t *out_keys, double *out_sums,
                          uint64_t out_cap, uint64_t *cursor);

/* ---- hash partition (shuffle map side) -------------------------------- *
 * Replaces partition_key_str (quokka_runtime.py:217-231). Int key semantics
 * bit-exact with the reference (:222): part = key % nparts (non-negative
 * keys; a negative key takes the mathematical, non-negative mod).
 * hist_dev: u64[nparts], zeroed. nparts == 0 is refused with
 * hipErrorInvalidValue before any launch, by both entry points;
 * qk_partition_scatter also refuses nparts > 512. */
int qk_partition_hist(void *stream, uint64_t n, const int64_t *keys,
                      uint32_t nparts, uint64_t *hist_dev);
/* Scatter row indices grouped by partition: out_idx[offsets[p] ... ] = rows
 * of partition p (order within a partition unspecified). cursors_dev must be
 * initialized to the exclusive prefix sum of hist (u64[nparts]). */
int qk_partition_scatter(void *stream, uint64_t n, const int64_t *keys,
                         uint32_t nparts, uint64_t *cursors_dev,
                         uint32_t *out_idx);

/* ---- stable radix sort ------------------------------------------------ *
 * Replaces the sorts the reference delegates to polars
 * (SuperFastSortExecutor sql_executors.py:88-187; build-side sort :369;
 * order-by tails). Stable ascending LSD sort of (u64 key, u32 payload);
 * keys_tmp/pay_tmp: caller scratch of same sizes; npasses -1 derives the
 * pass count from the max key. Order-preserving key maps for f64/i64 and
 * an iota payload helper included. */
int qk_sort_pairs_u64(void *stream, uint64_t n, uint64_t *keys,
                      uint32_t *payload, uint64_t *keys_tmp,
                      uint32_t *pay_tmp, int npasses);
/* f64 image order: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN. Every NaN,
 * of either sign and any payload, maps to UINT64_MAX: NaNs sort last
 * ascending, first descending (after qk_bnot_u64), and keep their input
 * order among themselves. */
int qk_map_f64_u64(void *stream, uint64_t n, const double *in, uint64_t *out);
int qk_map_i64_u64(void *stream, uint64_t n, const int64_t *in,
                   uint64_t *out);
int qk_iota_u32(void *stream, uint64_t n, uint32_t *out);
int qk_bnot_u64(void *stream, uint64_t n, uint64_t *x); /* stable desc sort */

/* ---- hiprtc JIT (arbitrary predicates / transforms / partial aggs) --- *
 * Runtime-compiled gfx950 kernels for the reference's ARBITRARY
 * filter_sql predicates (core.py:157-170), transform_sql expressions
 * (datastream.py:652-815) and folded map-side batch aggregates
 * (df.py:1354-1394) — quokka_amd/jit.py translates the SQL grammar to
 * the C expressions these take. Compilation needs no GPU; module load
 * is lazy at first run. coltypes: 0=i32, 1=f64, 2=u8, 3=i64.
 * qk_jit_last_error() returns the hiprtc log on compile failure. */
const char *qk_jit_last_error(void);
int qk_jit_filter_build(const char *c_expr, int ncols, const int *coltypes,
                        void **prog_out);
int qk_jit_filter_run(void *prog, void *stream, uint64_t n,
                      const void *const *col_ptrs, uint32_t *out_idx,
                      uint64_t *count_dev);
int qk_jit_map_build(const char *c_expr, int ncols, const int *coltypes,
                     void **prog_out);
int qk_jit_map_run(void *prog, void *stream, uint64_t n,
                   const void *const *col_ptrs, double *out_dev);
/* group_expr: C int expression over v<i>; ngroups*naggs <= 64 (register
 * accumulators; use qk_groupby_* for high cardinality). out accumulates
 * ngroups*naggs f64 (row-major [group][agg]). agg_ops (or NULL = all
 * SUM): 0=SUM, 1=MIN, 2=MAX per aggregate — the caller must initialize
 * `out` to the matching identity (0 / +inf / -inf) before the first
 * run; untouched MIN/MAX groups keep the identity. */
int qk_jit_agg_build(const char *pred_or_empty, const char *group_expr,
                     int ngroups, int naggs, const char *const *agg_exprs,
                     const int *agg_ops, int ncols, const int *coltypes,
                     void **prog_out);
int qk_jit_agg_run(void *prog, void *stream, uint64_t n,
                   const void *const *col_ptrs, double *out_dev);
int qk_jit_filter_free(void *prog);   /* frees any qk_jit_* program */
uint64_t qk_jit_code_size(void *prog);

/* ---- RCCL exchange (multi-GPU hash repartition) ----------------------- *
 * Replaces the reference's shuffle data plane (core.py:276-376 push ->
 * Arrow Flight do_put/do_get, flight.py) for the join/group-by
 * repartition: per-rank column buffers, partition-ordered by
 * `key % world` (quokka_runtime.py:222), exchanged with grouped
 * ncclSend/ncclRecv over xGMI — direct per-peer sends (7 p2p links/GPU),
 * not a ring (SURVEY.md §5 backend note). One rank per GPU; the 128-byte
 * unique id is broadcast host-side (gloo) by the caller. */
#define QK_UID_BYTES 128
int qk_comm_unique_id(uint8_t out[QK_UID_BYTES]);
int qk_comm_init(int rank, int world, const uint8_t uid[QK_UID_BYTES],
                 void **comm_out);
int qk_comm_destroy(void *comm);
/* All-to-all of one column: for each peer p, send send_counts[p] elements
 * of `elem_size` bytes from send_buf + send_offsets[p]*elem_size and
 * receive recv_counts[p] into recv_buf + recv_offsets[p]*elem_size.
 * Counts/offsets are HOST arrays (exchanged by the caller beforehand).
 * Grouped send/recv, completes on `stream`. */
int qk_alltoallv(void *stream, void *comm, int world, uint32_t elem_size,
                 const void *send_buf, const uint64_t *send_offsets,
                 const uint64_t *send_counts, void *recv_buf,
                 const uint64_t *recv_offsets, const uint64_t *recv_counts);
/* All-reduce SUM of an f64 device buffer (tiny partial-agg combine). */
int qk_allreduce_f64(void *stream, void *comm, double *buf, uint64_t n);

/* ---- GPU Parquet page decode ------------------------------------------ *
 * The reference scans Parquet with pyarrow's CPU reader
 * (pyquokka/dataset.py InputParquetDataset.get_next_batch ->
 * pyarrow.parquet). Here the host parses only METADATA (footer via
 * pyarrow; per-page Thrift headers and RLE run boundaries in
 * quokka_amd/parquet_thrift.py + parquet_gpu.py) and the raw column
 * chunk bytes are uploaded once; these kernels do all VALUE decoding in
 * HBM. Host-built tile tables (uploaded as u64 arrays) give each
 * workgroup one bounded slice of work.
 *
 * PLAIN pages (fixed-width): tiles = ntiles x 3 u64
 * [src_byte_off, dst_elem_off, count]; elem-wise copy of `count` values
 * of `elem_size` bytes from src_bytes+src_byte_off (byte-aligned, may be
 * unaligned) to dst + dst_elem_off. */
int qk_pq_plain_copy(void *stream, uint64_t ntiles, const uint64_t *tiles,
                     const void *src_bytes, void *dst, uint32_t elem_size);
/* RLE/bit-packed hybrid dictionary indices (parquet encoding.md),
 * parsed AND expanded on-device, one wave per page (low-cardinality
 * columns emit millions of tiny runs — host-side run parsing cost
 * seconds, so the host ships one descriptor per page): ents = npages x
 * 8 u64 [src_off (first run header, after the bit-width byte), src_end,
 * dst_off, count, bit_width, idx_off, dict_n, 0]. Emits u32
 * (index + idx_off) — idx_off rebases each chunk's dictionary into a
 * column-global concatenated dictionary so a whole multi-row-group
 * column expands in ONE launch. bit_width 0 => all idx_off, the stream
 * is not read. src_bytes needs >= 8 bytes of slack after the end.
 * err_dev = npages i64, written for every page: 0 ok; 1 stream truncated
 * (a header varint that reaches src_end or is longer than 10 bytes, RLE
 * value bytes or the used values of a bit-packed run past src_end, or
 * the stream ends with values still owed); 2 an index >= dict_n among
 * the `count` values used (padding bits of a clipped last group are not
 * values); 3 bit_width > 32 or src_off > src_end, refused before any
 * read. The first error in stream order ends the page. No byte at or
 * past src_end influences out or err_dev; a bit-packed run is accepted
 * when the bytes of the values used, ceil(n * bit_width / 8), lie before
 * src_end even if the padding of its last group does not. A page writes
 * only inside out[dst_off, dst_off + count), and every u32 it writes lies
 * in [idx_off, idx_off + max(dict_n, 1)): an index >= dict_n is written
 * as idx_off, so a gather stays in range before the host has seen
 * err_dev. */
int qk_pq_rle_pages(void *stream, uint64_t npages, const uint64_t *ents,
                    const uint8_t *src_bytes, uint32_t *out,
                    int64_t *err_dev);

/* ---- nullable columns: validity bitmaps ------------------------------ *
 * A nullable column is a dense value column of n rows (null slots hold 0)
 * plus a validity bitmap in Arrow layout: bit i lives in byte i >> 3, LSB
 * first, 1 = valid. The bitmap buffer is 8-byte aligned, sized up to a
 * multiple of 8 bytes plus 8 bytes of slack, and every bit at an index
 * >= n is 0 (kernels popcount whole 64-bit words without a tail mask).
 * Null keys are opt-in: qk_join_build_valid / qk_join_probe_valid take a
 * key column's bitmap, and qk_key_null_words / qk_nullword_to_valid carry
 * null group and distinct keys through the key dictionary. Those entry
 * points never read the value under a null. Null strings outside key
 * columns are not supported.
 *
 * qk_pq_def_pages: definition levels of a flat column (max_def == 1, bit
 * width 1, RLE/bit-packed hybrid) -> validity bits, one wave per page.
 * descs = npages x 6 u64 [levels_off, page_end, v2_levels_len,
 * first_row, num_values, 0], offsets into src_dev. v2_levels_len ==
 * UINT64_MAX marks a v1 page, whose block starts with its own [u32 len]
 * prefix; a v2 page's levels have no prefix and the length comes from
 * the page header. The page's bits go to valid_dev at first_row; pages
 * start at any row, so the first and last word of a page may be shared
 * with the neighbouring page: those are OR-ed in atomically and
 * valid_dev must be ZEROED before the call. Interior words are plain
 * stores. out_dev = npages x 4 i64 [non_null_count, values_off (absolute,
 * first byte after the levels), err, first_value_byte (the bit width of an
 * RLE_DICTIONARY page; -1 when the page has no value bytes, as an
 * all-null page may)]; err: 0 ok, 1 levels run past the
 * page, 2 stream truncated, 3 a level above 1. A corrupt stream ends
 * with an error code, never a spin or a read past page_end. */
int qk_pq_def_pages(void *stream, uint64_t npages, const uint64_t *descs_dev,
                    const uint8_t *src_dev, uint64_t *valid_dev,
                    int64_t *out_dev);
/* Inverse of compaction: out[row] = valid[row] ? dense[rank(row)] : 0,
 * rank = number of valid rows before `row`. Parquet stores only the
 * non-null values; dense_dev holds popcount(valid) of them. elem_size 4
 * or 8. */
int qk_valid_expand(void *stream, uint64_t n, const uint64_t *valid_dev,
                    const void *dense_dev, void *out_dev, uint32_t elem_size);
/* bitmap -> u8 0/1 flags, out[i] = bit i (the predicate JIT reads
 * validity as one more u8 input column) */
int qk_valid_to_u8(void *stream, uint64_t n, const uint64_t *valid_dev,
                   uint8_t *out);
/* Bitmap of the rows idx[0..n_idx) selects, plus their null count ADDED
 * to *out_null_count_dev (caller zeroes it). Writes ceil(n_idx / 64)
 * whole words of out_valid_dev; the caller zeroes the slack behind them. */
int qk_valid_gather(void *stream, uint64_t n_idx, const uint32_t *idx,
                    const uint64_t *valid_dev, uint64_t *out_valid_dev,
                    uint64_t *out_null_count_dev);
/* Optional gather, value and validity in one pass over idx (the emit of a
 * join whose payload columns hold NULLs, and of the left join, whose
 * unmatched rows have no build row). Row i is valid iff idx[i] != QK_NO_ROW
 * and (src_valid_dev == NULL, meaning every source row is valid, or bit
 * idx[i] of src_valid_dev is set). A valid row writes dst[i] = src[idx[i]];
 * an invalid row writes dst[i] = 0 and does not read src, so null slots
 * hold 0 and the value under a source null is never used. out_valid_dev
 * gets ceil(n_idx / 64) whole words, bits at an index >= n_idx 0; the
 * caller zeroes the slack word behind them. The null count is ADDED to
 * *out_null_count_dev (caller zeroes it). n_idx == 0 launches nothing.
 * PRECONDITION: every index other than QK_NO_ROW is below the source
 * length (rows of src, bits of src_valid_dev); the kernel does not check. */
int qk_take_opt_i64(void *stream, uint64_t n_idx, const uint32_t *idx,
                    const int64_t *src, const uint64_t *src_valid_dev,
                    int64_t *dst, uint64_t *out_valid_dev,
                    uint64_t *out_null_count_dev);
int qk_take_opt_f64(void *stream, uint64_t n_idx, const uint32_t *idx,
                    const double *src, const uint64_t *src_valid_dev,
                    double *dst, uint64_t *out_valid_dev,
                    uint64_t *out_null_count_dev);
int qk_take_opt_i32(void *stream, uint64_t n_idx, const uint32_t *idx,
                    const int32_t *src, const uint64_t *src_valid_dev,
                    int32_t *dst, uint64_t *out_valid_dev,
                    uint64_t *out_null_count_dev);
int qk_take_opt_u8(void *stream, uint64_t n_idx, const uint32_t *idx,
                   const uint8_t *src, const uint64_t *src_valid_dev,
                   uint8_t *dst, uint64_t *out_valid_dev,
                   uint64_t *out_null_count_dev);
/* ---- device string dictionary ---------------------------------------- *
 * General variable-width string keys for join/group-by (the reference
 * joins/groups on arbitrary key types via polars, sql_executors.py:
 * 325-377/:556-599). Open-addressing table keyed by a 64-bit byte hash
 * with EXACT byte verification against an on-device arena; assigns dense
 * u32 codes, consistent across calls because table+arena persist. Equal
 * strings => equal codes (bytes verified), so string joins/group-bys run
 * on the existing integer kernels over the codes.
 * slot_hash u64[cap] zeroed (0 = empty), slot_code i32[cap] filled -1,
 * code_off u64 / code_len u32 per code, arena + arena_cursor_dev (u64),
 * counter_dev (u32) = number of codes. HOST must guarantee, before each
 * call: table load < 1/2 after worst-case n new codes, code arrays hold
 * counter + n, arena holds cursor + sum(len). */
int qk_str_dict_encode(void *stream, uint64_t n, const int64_t *offsets,
                       const uint8_t *bytes, uint64_t *slot_hash,
                       int32_t *slot_code, uint64_t capacity,
                       uint64_t *code_off, uint32_t *code_len,
                       uint8_t *arena, uint64_t *arena_cursor_dev,
                       uint32_t *counter_dev, uint32_t *out_codes);
/* Growth: re-seat (hash, code) pairs into a larger zeroed/-1 table;
 * codes and arena unchanged (previously returned codes stay valid). */
int qk_str_dict_rehash(void *stream, uint32_t ncodes,
                       const uint64_t *code_off, const uint32_t *code_len,
                       const uint8_t *arena, uint64_t *slot_hash,
                       int32_t *slot_code, uint64_t capacity);
/* Per-row string hash for hash partitioning: out[i] = the dictionary's
 * 64-bit byte hash of row i (length-seeded splitmix64 fold over 8-byte
 * little-endian words, zero-padded tail, 0 remapped to 1) shifted right by
 * one, so it is a non-negative i64 for qk_partition_hist/_scatter. A pure
 * function of the row's bytes: equal strings get equal values in every
 * call, process and rank. offsets: i64[n + 1] into bytes. */
int qk_str_hash_i64(void *stream, uint64_t n, const int64_t *offsets,
                    const uint8_t *bytes, int64_t *out);
/* ---- device key dictionary (K full-width key columns) ----------------- *
 * SQLAggExecutor groups by an arbitrary groupby_keys list inside DuckDB
 * (sql_executors.py:556-599) and DistinctExecutor calls
 * unique(subset=keys) (sql_executors.py:517-554). Here every key column is
 * one 64-bit word per row, and a row's tuple of nkeys words maps to a
 * dense u32 code that is the same in every later call (slots, key store
 * and counter persist). No key value is reserved: INT64_MIN, 0, -1 and
 * INT64_MAX are ordinary keys in every column.
 *
 * key_cols_dev: device array of nkeys pointers to i64 columns of n rows.
 * slots: u64[capacity] (pow2), zeroed before first use. A word is 0 when
 *   free; otherwise bits 62..32 hold a non-zero 31-bit hash tag and bits
 *   31..0 the code. Bit 63 marks a slot claimed during the running call,
 *   whose low half is then the claiming batch row; no such word survives a
 *   call that reports no error. All nkeys words are compared before a slot
 *   counts as a match; the tag only spares most of those compares.
 * store: i64[nkeys * code_cap], column-major: word k of code c is
 *   store[k * code_cap + c].
 * counter_dev (u32): number of codes handed out so far.
 * row_slot: scratch, u64[n]. out_codes: u32[n].
 * err_dev (u32, zeroed by the caller): OR of 1 = a probe walk visited all
 *   `capacity` slots without finding the key or a free slot, 2 = a new
 *   code did not fit code_cap. After an error the table must be dropped.
 * Three launches (claim, finalise, resolve); no lane waits for another
 * lane's store, and every probe walk ends after `capacity` steps. HOST
 * must guarantee before each call: 2 * (counter + n) <= capacity,
 * counter + n <= code_cap, n < 2^32, counter + n < 2^32 - 1. */
int qk_keydict_encode(void *stream, uint64_t n, int nkeys,
                      const void *key_cols_dev /* dev int64_t*[nkeys] */,
                      uint64_t *slots, uint64_t capacity, int64_t *store,
                      uint64_t code_cap, uint32_t *counter_dev,
                      uint64_t *row_slot, uint32_t *out_codes,
                      uint32_t *err_dev);
/* Growth: seat (hash of store[code], code) for every code < ncodes into a
 * larger zeroed slot array. Codes and key store are not touched (the host
 * grows the store by per-column device copies). err_dev as above (bit 1). */
int qk_keydict_rehash(void *stream, uint32_t ncodes, int nkeys,
                      const int64_t *store, uint64_t code_cap,
                      uint64_t *slots, uint64_t capacity, uint32_t *err_dev);
/* ---- null keys in the key dictionary ---------------------------------- *
 * DuckDB's GROUP BY makes one group of NULL keys per null pattern and
 * polars' unique(subset=) lets nulls equal each other. A nullable
 * dictionary keys each row on nkeys + W words, W = ceil(nkeys / 64): the
 * nkeys CANONICAL key words (the key word where the key is valid, 0 where
 * it is NULL) followed by W NULL WORDS (bit k % 64 of null word k / 64 is 1
 * when key k of the row is NULL). Two rows then share a code exactly when
 * they have the same null pattern and equal words in every non-null
 * position; (NULL, 0), (0, NULL), (0, 0) and (NULL, NULL) are four keys.
 * qk_keydict_encode / qk_keydict_rehash run over the nkeys + W columns
 * unchanged; the null words are ordinary store columns.
 *
 * qk_key_null_words, the prepare pass, one streaming launch:
 * key_cols_dev: device array of nkeys pointers to i64 columns of n rows.
 * valid_ptrs_dev: device array of nkeys bitmap pointers (layout under
 *   "nullable columns" above; at least ceil(n / 64) whole words); 0 = key
 *   k has no nulls, and then nothing of key k is read or written.
 * canon_cols_dev: device array of nkeys pointers; entry k is an i64 column
 *   of n rows wherever valid_ptrs_dev[k] != 0 and receives the canonical
 *   copy of key k (entries of keys without a bitmap are ignored). The word
 *   a key column holds under a null does not reach any output.
 * null_cols_dev: device array of W pointers to i64 columns of n rows, all
 *   written. */
int qk_key_null_words(void *stream, uint64_t n, int nkeys,
                      const void *key_cols_dev /* dev int64_t*[nkeys] */,
                      const void *valid_ptrs_dev /* dev uint64_t*[nkeys] */,
                      const void *canon_cols_dev /* dev int64_t*[nkeys] */,
                      const void *null_cols_dev /* dev int64_t*[W] */);
/* The inverse, at extraction: Arrow validity bitmap of one key over the
 * first g codes, bit c = !(null_col[c] >> bit & 1), where null_col is the
 * key's null-word store column (store + (nkeys + k / 64) * code_cap) and
 * bit = k % 64. Writes every word of a valid_nbytes(g) = (ceil(g / 64) + 1)
 * * 8 byte buffer (bits at an index >= g are 0, g == 0 included) and ADDS
 * the null count to *out_null_count_dev (caller zeroes it). */
int qk_nullword_to_valid(void *stream, uint64_t g, const int64_t *null_col,
                         int bit, uint64_t *out_valid_dev,
                         uint64_t *out_null_count_dev);
/* ---- dense accumulate over key-dictionary codes ----------------------- *
 * The aggregate half of SQLAggExecutor's group-by (sql_executors.py:
 * 556-599) once qk_keydict_encode has turned the key columns into dense
 * codes: acc holds one record of rstride (pow2 >= nvals) doubles per code,
 * record c at acc[c * rstride], so a row touches one line and extraction
 * is a plain copy of the first `counter` records.
 * qk_groupby_dense_init sets records [first, first + count) to the op
 * identities inits_dev[nvals] (0 SUM, +inf MIN, -inf MAX; pad words 0). */
int qk_groupby_dense_init(void *stream, double *acc, uint64_t first,
                          uint64_t count, int rstride, int nvals,
                          const double *inits_dev);
/* For each row i: acc[codes[i]][c] op= vals[c][i], op per agg_ops_dev as in
 * qk_groupby_i64_sum (NULL = all SUM). A code >= ncodes is skipped and
 * reported as bit 4 of err_dev (u32, zeroed by the caller). */
int qk_groupby_dense_acc(void *stream, uint64_t n, const uint32_t *codes,
                         uint32_t ncodes,
                         const void *vals_dev /* dev double*[nvals] */,
                         const int32_t *agg_ops_dev, int nvals, int rstride,
                         double *acc, uint32_t *err_dev);
/* qk_groupby_dense_acc over value columns with SQL NULLs: SUM / MIN / MAX
 * skip them, and an aggregate that met no value is NULL (DuckDB's GROUP BY,
 * pyarrow Acero with min_count = 1).
 * valid_ptrs_dev: device array of nvals bitmap pointers (layout under
 *   "nullable columns" above; at least ceil(n / 64) whole words; the bits of
 *   the last word at row indices >= n may hold anything); 0 = column c has
 *   no nulls, and then nothing of a bitmap is read for it. Where a row's bit
 *   is 0 the value word under it is not read and nothing of that row
 *   reaches column c's accumulator.
 * seen: one u64 per code, beside the records and zeroed by the caller for
 *   new codes; bit c of seen[code] is set once column c of that group has
 *   received a value, so nvals <= 64. Records keep the layout and the
 *   identities of qk_groupby_dense_init: an aggregate whose seen bit is 0
 *   still holds its identity. A code >= ncodes writes neither. */
int qk_groupby_dense_acc_valid(void *stream, uint64_t n,
                               const uint32_t *codes, uint32_t ncodes,
                               const void *vals_dev /* dev double*[nvals] */,
                               const void *valid_ptrs_dev
                               /* dev uint64_t*[nvals] */,
                               const int32_t *agg_ops_dev, int nvals,
                               int rstride, double *acc, uint64_t *seen,
                               uint32_t *err_dev);
/* ---- LIKE over free-text string columns ------------------------------- *
 * The reference hands `col LIKE 'pat'` / NOT LIKE / = / <> on varchar
 * columns to DuckDB or polars inside filter_sql (core.py:157-163; the
 * TPC-H call sites are apps/tpc-h/tpch.py:137,316,380,389,413,416,481).
 * Semantics: DuckDB's default LIKE — case-sensitive, % = any run of bytes
 * (empty included), _ = exactly one UTF-8 code point, no ESCAPE clause
 * (backslash is an ordinary byte).
 *
 * qk_like_pat is the compiled pattern: the pattern bytes with every '%'
 * removed, cut into at most QK_LIKE_MAX_SEGS non-empty segments (runs of
 * literal bytes and _ wildcards between % signs), plus whether the first
 * segment is anchored at the start and the last at the end. `wild` marks
 * which bytes of `pat` are _ wildcards; exact patterns (= / <>) have none
 * and a single doubly-anchored segment. Plain data, passed to the kernel
 * by value. */
#define QK_LIKE_MAX_PAT 256
#define QK_LIKE_MAX_SEGS 16
typedef struct {
  uint32_t nseg;
  uint8_t anchor_start;
  uint8_t anchor_end;
  uint8_t exact;
  uint8_t pad_;
  uint16_t seg_off[QK_LIKE_MAX_SEGS]; /* into pat */
  uint16_t seg_len[QK_LIKE_MAX_SEGS];
  uint32_t wild[QK_LIKE_MAX_PAT / 32]; /* bit k: pat[k] is a _ wildcard */
  uint8_t pat[QK_LIKE_MAX_PAT];
} qk_like_pat;
/* Host only: compile SQL pattern bytes (exact != 0: every byte literal,
 * the = / <> form; replaces the pattern handling DuckDB does for
 * tpch.py:380 `o_comment not like '%special%requests%'` and :416
 * `p_brand != 'Brand#45'`). Returns non-zero, with qk_last_error set, for
 * len > QK_LIKE_MAX_PAT or more than QK_LIKE_MAX_SEGS segments — never
 * truncates. */
int qk_like_compile(const uint8_t *pat, uint32_t len, int exact,
                    qk_like_pat *out);
/* Per-row match over an Arrow string column (offsets[n+1] + bytes, both
 * device pointers): out_flags[r] = match(row r) ^ (negate != 0), 0 or 1
 * (tpch.py:380 filter_sql("o_comment not like ..."), :413, :316, :481).
 * One block handles 256 consecutive rows, whose bytes are one contiguous
 * span. For a pattern with a searched segment (a % before or between
 * literals), spans that fit the LDS tile (qk_like_tile_bytes) are staged
 * into LDS with 16-byte loads and matched from there; longer spans, and
 * every span of a pattern made of anchored segments only (prefix, suffix,
 * equality: a few bytes per row), are matched straight from global memory
 * by the same matcher. i32 = Arrow `string`
 * offsets, i64 = `large_string`. `pat` is a HOST pointer. n == 0 returns
 * 0 without a launch. */
int qk_str_like_i32(void *stream, uint64_t n, const int32_t *offsets,
                    const uint8_t *bytes, const qk_like_pat *pat, int negate,
                    uint8_t *out_flags);
int qk_str_like_i64(void *stream, uint64_t n, const int64_t *offsets,
                    const uint8_t *bytes, const qk_like_pat *pat, int negate,
                    uint8_t *out_flags);
/* The two above with the path chosen by the caller (stage != 0: LDS
 * staging for spans that fit; 0: every block direct from global memory)
 * instead of by the pattern's shape: the A/B of scripts/bench_like.py and
 * the tests of either path. Same results. */
int qk_str_like_path_i32(void *stream, uint64_t n, const int32_t *offsets,
                         const uint8_t *bytes, const qk_like_pat *pat,
                         int negate, int stage, uint8_t *out_flags);
int qk_str_like_path_i64(void *stream, uint64_t n, const int64_t *offsets,
                         const uint8_t *bytes, const qk_like_pat *pat,
                         int negate, int stage, uint8_t *out_flags);
/* The same matcher in a plain CPU loop over HOST pointers (what DuckDB's
 * LIKE computes for tpch.py:380 on the host): the CPU tests reach the
 * shared __host__ __device__ matcher through this. */
int qk_str_like_host_i64(uint64_t n, const int64_t *offsets,
                         const uint8_t *bytes, const qk_like_pat *pat,
                         int negate, uint8_t *out_flags);
/* Bytes of the LDS tile of qk_str_like_* (a block's span, plus up to 15
 * bytes of alignment shift, must fit it to take the staged path). Returns
 * the size, not an error code. */
int qk_like_tile_bytes(void);
/* Composite i64 key column: out = x * scale + y (per-(a,b) group keys,
 * e.g. Q20's (partkey, suppkey) quantity sums). */
int qk_i64_combine(void *stream, uint64_t n, const int64_t *x,
                   const int64_t *y, int64_t scale, int64_t *out);
/* Arithmetic shift right: out = x >> shift (decompose pow2-scaled
 * composite keys on device, e.g. pair key -> orderkey). */
int qk_i64_shr(void *stream, uint64_t n, const int64_t *x, int shift,
               int64_t *out);
/* Synchronous device-to-device copy (dict growth, arena relocation). */
int qk_d2d(void *dst_dev, const void *src_dev, uint64_t nbytes);

/* GPU snappy decompression of Parquet pages (the reference reads
 * compressed files transparently through pyarrow,
 * unordered_readers.py:51). One wave per page, pages independent.
 * descs_dev: npages x 8 u64 [src_off, src_len, dst_off,
 * uncompressed_len, mode (0 raw / 1 verify v1 def-levels max_def==1 /
 * 2 v1 def-levels present and left in place for qk_pq_def_pages: the
 * page is only decompressed, data_off_rel is 0),
 * num_values, 0, 0]; out_dev: npages x 4 i64 [data_off_rel (start of
 * values after the in-page levels block), err (0 ok / 1 corrupt /
 * 2 length mismatch / 3 nulls present), first_byte_after_levels (the
 * RLE bit-width byte, -1 if none), 0]. */
int qk_snappy_pages(void *stream, uint64_t npages, const uint64_t *descs_dev,
                    const uint8_t *src_dev, uint8_t *dst_dev,
                    int64_t *out_dev);
/* GPU gzip (DEFLATE) decompression of Parquet pages: entropy decode is
 * sequential, so lane 0 decodes a page's bit stream (canonical Huffman
 * tables built in LDS) and pages decode independently in parallel.
 * descs_dev: npages x 8 u64 [src_off, src_len, dst_off,
 * uncompressed_len, mode (1 = gzip wrapper / 0 = raw deflate), 0,0,0];
 * out_dev: npages x 4 i64 [written, err (0 ok/1 corrupt/2 length
 * mismatch/3 unsupported), first_byte, 0]. */
int qk_gzip_pages(void *stream, uint64_t npages, const uint64_t *descs_dev,
                  const uint8_t *src_dev, uint8_t *dst_dev,
                  int64_t *out_dev);
/* Host-side Thrift compact-protocol walk of one column chunk's page
 * headers (parquet-format PageHeader; the metadata side of the decode —
 * pyarrow exposes only the footer, and walking thousands of headers in
 * Python measured ~0.2 s/GB of file, dominating warm end-to-end scans).
 * out: max_pages x 10 i64 [kind(0 data v1/2 dict/3 data v2), num_values,
 * encoding, def_level_encoding(-1 none/3 RLE), data_off(abs),
 * data_len(compressed), v2_levels_len, num_nulls, uncompressed_len, 0];
 * *n_out = pages written. Walks until num_values data values covered. */
#define QK_PQ_PAGE_FIELDS 10
int qk_pq_walk_pages(const uint8_t *buf, uint64_t start,
                     uint64_t total_len, int64_t num_values, int64_t *out,
                     int64_t max_pages, int64_t *n_out);

/* Range-partition ids (quokka_runtime.py:234-243 partition_key_range):
 * id = (key - 1) / (total_range / nparts), floor division, clamped into
 * [0, nparts-1] (the reference misroutes keys outside [1, total_range];
 * we clamp — documented divergence, same key->same channel). Every key
 * <= 0, INT64_MIN included, gives id 0, so ids never decrease as the key
 * grows. Feed the
 * ids to qk_partition_hist/scatter (id % nparts == id). */
int qk_range_part_ids(void *stream, uint64_t n, const int64_t *keys,
                      int64_t per_range, uint32_t nparts, int64_t *out);

/* ---- GPU CSV parse ---------------------------------------------------- *
 * The reference's CSV scan splits files into byte ranges and decodes on
 * the CPU with polars.read_csv (unordered_readers.py:273-442, :438).
 * Here the raw bytes live in HBM: qk_csv_newlines builds the ORDERED
 * newline index (u64 positions; count written to out_count_dev), then
 * qk_csv_parse decodes one row per thread. Anything unparseable is a row
 * error, never a silently different value. coltypes:
 *  0=i64: [+-]digits, at most 18 digits.
 *  1=f64: [+-]digits[.digits] with at least one digit, <=15 significant
 *    digits and <=18 decimals — parsed as exact-int / exact power-of-ten
 *    division, BIT-EXACT vs strtod ("-0" is -0.0).
 *  2=date32: exactly "YYYY-MM-DD", a real day of the proleptic Gregorian
 *    calendar (day checked against month and leap rule) -> days since
 *    1970-01-01.
 *  3=u8 dictionary code: the field must equal a candidate byte for byte
 *    over its whole length; unknown value = row error. <=32 candidates
 *    per column. dict_cands/dict_lens (first 8 bytes LE, length clamped
 *    to 255) are the prefilter; dict_bytes holds all candidates' bytes
 *    back to back and dict_offs[ncols * QK_CSV_MAX_DICT + 1] their u32
 *    start offsets (slot c * QK_CSV_MAX_DICT + j runs to the next slot's
 *    offset; unused slots are empty), against which a hit is confirmed.
 *  4=skip: any bytes.
 * Rows: a trailing '\r' is stripped (a '\r' elsewhere is field data);
 * exactly one trailing separator after the last schema field (dbgen
 * .tbl) is tolerated; fewer fields than the schema, or any further field
 * after it — an empty one included — is a row error. A field that starts
 * with quote_char runs to its closing quote ("" escapes stay in the
 * slice, so they fail typed parses); a missing closing quote, or a byte
 * other than the separator or the row end after it, is a row error.
 * Where this is stricter or more lenient than strtod / pyarrow.csv:
 * STRICTER — no exponent, inf, nan, hex or surrounding blanks; f64 text
 * with >15 significant digits or >18 decimals and i64 text with >18
 * digits are errors although strtod / strtoll can read them (the parse
 * would no longer be exact); empty fields are errors, not nulls, except
 * for an empty dictionary candidate. MORE LENIENT — year 0000 is read
 * as the proleptic year 0.
 * err_row: device u64 initialized to UINT64_MAX; the LOWEST failing row
 * index lands there. */
#define QK_CSV_MAX_DICT 32
int qk_csv_newlines(void *stream, uint64_t data_start, uint64_t n,
                    const uint8_t *bytes, uint64_t *out_pos,
                    uint64_t *out_count_dev);
/* Quote-aware variant (RFC-4180): a newline ends a row only when the
 * count of `quote` chars before it is even ("" escapes toggle twice and
 * cancel). Slower 5-pass path; callers use it only when the buffer
 * contains the quote char at all. An odd total number of quote chars
 * (a quote never closed, which would swallow every later row) writes
 * UINT64_MAX to out_count_dev; out_pos is then unspecified. */
int qk_csv_newlines_quoted(void *stream, uint64_t data_start, uint64_t n,
                           const uint8_t *bytes_dev, uint8_t quote_char,
                           uint64_t *out_pos_dev, uint64_t *out_count_dev);
int qk_csv_parse(void *stream, uint64_t nrows, const uint8_t *bytes,
                 uint64_t data_start, const uint64_t *nl_pos, uint8_t sep,
                 uint8_t quote_char /* 0 = no quoting */, int ncols,
                 const int *coltypes, void *const *out_ptrs,
                 const uint64_t *dict_cands, const uint8_t *dict_lens,
                 const int *ncands, const uint8_t *dict_bytes,
                 const uint32_t *dict_offs, uint64_t *err_row);

#ifdef __cplusplus
}
#endif
#endif /* QUOKKA_AMD_H */
