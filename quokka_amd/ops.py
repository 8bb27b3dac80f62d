"""Mid-level device operators over DevColumns.

Each operator maps 1:1 onto a reference delegate (SURVEY.md §2 native-
accounting table): filter -> polars DataFrame.filter (core.py:170);
join build/probe -> polars join (sql_executors.py:371); groupby -> DuckDB
group-by (sql_executors.py:595); partition -> partition_key_str
(quokka_runtime.py:217-231).
"""
import ctypes

import numpy as np

from . import shim
from .shim import DevBuffer, DevColumn, c_u64, c_u32, c_i64, c_i32, c_vp

# comparison ops for filter kernels
LT, LE, GT, GE, EQ, NE = range(6)


def _count_buf():
    b = DevBuffer(8)
    shim.call("qk_dmemset", b.ptr, 0, c_u64(8))
    return b


def _read_u64(buf):
    out = np.zeros(1, dtype=np.uint64)
    shim.call("qk_d2h", out.ctypes.data_as(c_vp), buf.ptr, c_u64(8))
    return int(out[0])


def filter_col(col, op, value, stream=None):
    """Ordered compaction: returns (idx DevColumn u32, count). Row order of
    passing rows is preserved (polars filter semantics)."""
    sh = stream.handle if stream else None
    idx = DevColumn(np.uint32, col.n)
    cnt = _count_buf()
    if col.dtype == np.dtype(np.int32):
        shim.call("qk_filter_i32", sh, c_u64(col.n), col.ptr, op,
                  c_i32(int(value)), idx.ptr, cnt.ptr)
    elif col.dtype == np.dtype(np.uint8):
        shim.call("qk_filter_u8", sh, c_u64(col.n), col.ptr, op,
                  ctypes.c_uint8(int(value)), idx.ptr, cnt.ptr)
    elif col.dtype == np.dtype(np.float64):
        shim.call("qk_filter_f64", sh, c_u64(col.n), col.ptr, op,
                  ctypes.c_double(float(value)), idx.ptr, cnt.ptr)
    else:
        raise TypeError("filter_col: unsupported dtype %s" % col.dtype)
    if stream:
        stream.sync()
    n = _read_u64(cnt)
    cnt.free()
    idx.n = n  # logical length; allocation stays col.n
    return idx, n


def q1_agg(n, shipdate, qty, price, disc, tax, rflag, lstat, cutoff,
           out_buf, stream=None):
    """Accumulate Q1 partials into out_buf (DevBuffer of 48 f64, zeroed by
    caller). See include/quokka_amd.h qk_q1_agg."""
    sh = stream.handle if stream else None
    shim.call("qk_q1_agg", sh, c_u64(n), shipdate.ptr, qty.ptr, price.ptr,
              disc.ptr, tax.ptr, rflag.ptr, lstat.ptr, c_i32(cutoff),
              out_buf.ptr)


def q1_read_partials(out_buf):
    """d2h the 6x8 accumulator block -> (6,6) float array
    [sum_qty,sum_base,sum_disc_price,sum_charge,sum_disc,count]."""
    host = np.zeros(48, dtype=np.float64)
    shim.call("qk_d2h", host.ctypes.data_as(c_vp), out_buf.ptr, c_u64(48 * 8))
    return host.reshape(6, 8)[:, :6].copy()


def q6_agg(n, shipdate, qty, price, disc, date_lo, date_hi, disc_lo, disc_hi,
           qty_hi, out_buf, stream=None):
    sh = stream.handle if stream else None
    shim.call("qk_q6_agg", sh, c_u64(n), shipdate.ptr, qty.ptr, price.ptr,
              disc.ptr, c_i32(date_lo), c_i32(date_hi),
              ctypes.c_double(disc_lo), ctypes.c_double(disc_hi),
              ctypes.c_double(qty_hi), out_buf.ptr)


def check_no_sentinel_key(keys, operator, column):
    """Raise ValueError when the host i64 key array `keys` contains
    INT64_MIN. That value is QK_JOIN_EMPTY, the free-slot marker of the
    join and group-by tables: a build or group key equal to it matches the
    first free slot without claiming it, and a later key inherits its chain
    or its sums. Host-only, so executors call it before any device call.
    Join PROBE keys need no check (a probe for it reports no match)."""
    keys = np.asarray(keys)
    if keys.size and keys.dtype == np.int64 and \
            bool((keys == shim.JOIN_EMPTY).any()):
        raise ValueError(
            "%s: key column %r contains INT64_MIN (%d), the reserved "
            "empty-slot marker of the device hash table; such keys are "
            "not supported" % (operator, column, int(shim.JOIN_EMPTY)))


# A MIN/MAX slot that no input has reached holds this quiet-NaN pattern
# (QK_MM_NONE in csrc): a NaN input turns it into the canonical NaN, a
# number replaces either, and the read-out maps what is left of it to the
# op's identity. So MIN/MAX skip NaN beside numbers, an all-NaN group is
# NaN, and an untouched slot still reads +inf / -inf.
MM_NONE_BITS = 0x7FF8C0DE0000A66F


def _pow2_at_least(n):
    c = 1
    while c < n:
        c <<= 1
    return c


def _key_bitmap(col, valid, n, what="key"):
    """Validity bitmap of a key (or value) column for n rows -> (device bitmap or
    None, owned). `valid` is None, a device bitmap (anything with .ptr, in
    the NullableColumn.valid layout) or a host bool mask (True = valid),
    which is packed and uploaded; with None a NullableColumn supplies its
    own. The caller frees an owned bitmap."""
    if valid is None:
        return (col.valid, False) if isinstance(col, NullableColumn) \
            else (None, False)
    if hasattr(valid, "ptr"):
        return valid, False
    mask = np.asarray(valid)
    if mask.dtype != np.bool_ or mask.ndim != 1 or len(mask) < n:
        raise TypeError("%s validity: a device bitmap or a host bool "
                        "mask of at least n rows expected" % what)
    bits = pack_valid(mask[:n])
    buf = DevBuffer(len(bits))
    shim.call("qk_h2d", buf.ptr, bits.ctypes.data_as(c_vp),
              c_u64(len(bits)))
    return buf, True


class JoinTable:
    """Device hash-join state = BuildProbeJoinExecutor's vstacked build side
    (sql_executors.py:346-374). build() may be called per build batch;
    probe() per probe batch.

    Precondition: no BUILD key equals INT64_MIN (QK_JOIN_EMPTY, the
    free-slot marker). build() takes device keys and does not look at
    them; callers with host keys use check_no_sentinel_key first. Probe
    keys may take any value.

    Null keys: build() and probe() take `valid`, the key column's validity
    (a device bitmap or a host bool mask; a NullableColumn supplies its
    own). A null key matches nothing on either side and the word under it
    is never read, so the precondition binds valid build keys only. A null
    build row still takes its row number, so build indices address the
    payload columns as before."""

    def __init__(self, expected_build_rows, stream=None):
        self.cap = _pow2_at_least(max(16, 2 * int(expected_build_rows)))
        self.stream = stream
        self.slot_keys = DevColumn(np.int64, self.cap)
        self.slot_head = DevColumn(np.int32, self.cap)
        self.chain_cap = max(16, int(expected_build_rows))
        self.chain_next = DevColumn(np.int32, self.chain_cap)
        self.n_build = 0
        sh = stream.handle if stream else None
        shim.call("qk_fill_i64", sh, self.slot_keys.ptr,
                  c_i64(int(shim.JOIN_EMPTY)), c_u64(self.cap))
        shim.call("qk_dmemset", self.slot_head.ptr, 0xFF,
                  c_u64(self.cap * 4))

    def build(self, keys_col, n=None, valid=None):
        n = keys_col.n if n is None else n
        if self.n_build + n > self.chain_cap or self.n_build + n > self.cap // 2:
            raise RuntimeError(
                "JoinTable overflow: built %d + %d > capacity %d; size the "
                "table from the build side's total rows"
                % (self.n_build, n, min(self.chain_cap, self.cap // 2)))
        sh = self.stream.handle if self.stream else None
        bitmap, owned = _key_bitmap(keys_col, valid, n)
        table = (c_u32(self.n_build), self.slot_keys.ptr, self.slot_head.ptr,
                 self.chain_next.ptr, c_u64(self.cap))
        if bitmap is None:
            shim.call("qk_join_build", sh, c_u64(n), keys_col.ptr, *table)
        else:
            shim.call("qk_join_build_valid", sh, c_u64(n), keys_col.ptr,
                      bitmap.ptr, *table)
            if owned:
                shim.call("qk_stream_sync", sh)
                bitmap.free()
        self.n_build += n

    def probe(self, keys_col, mode=0, out_factor=1.5, n=None, valid=None):
        """mode 0 inner / 1 semi / 2 anti / 3 left. Returns (probe_idx,
        build_idx, count) DevColumns (build_idx None for semi/anti). Left
        is inner plus every probe row without a match once, with NO_ROW as
        its build index. Grows the output
        and re-probes when the first guess undershoots (counted, never
        truncated). With `valid` a null probe row is a miss."""
        n = keys_col.n if n is None else n
        sh = self.stream.handle if self.stream else None
        bitmap, owned = _key_bitmap(keys_col, valid, n)
        out_cap = max(16, int(n * out_factor))
        while True:
            probe_idx = DevColumn(np.uint32, out_cap)
            build_idx = DevColumn(np.uint32, out_cap) if mode in (0, 3) \
                else None
            cur = _count_buf()
            name, keys = ("qk_join_probe", (keys_col.ptr,)) if bitmap is None \
                else ("qk_join_probe_valid", (keys_col.ptr, bitmap.ptr))
            shim.call(name, sh, c_u64(n), *keys, self.slot_keys.ptr,
                      self.slot_head.ptr, self.chain_next.ptr,
                      c_u64(self.cap), mode, probe_idx.ptr,
                      build_idx.ptr if build_idx else None, c_u64(out_cap),
                      cur.ptr)
            if self.stream:
                self.stream.sync()
            total = _read_u64(cur)
            cur.free()
            if total <= out_cap:
                if owned:
                    bitmap.free()
                probe_idx.n = total
                if build_idx is not None:
                    build_idx.n = total
                return probe_idx, build_idx, total
            probe_idx.free()
            if build_idx is not None:
                build_idx.free()
            out_cap = int(total)

    def free(self):
        self.slot_keys.free()
        self.slot_head.free()
        self.chain_next.free()


class GroupByI64:
    """Device group-by accumulate table over an i64 key with nvals f64 SUM
    columns (SQLAggExecutor's post-rewrite distributive form,
    sql_utils.py:299-413). update() per batch, extract() at done().

    Precondition: no key equals INT64_MIN (QK_JOIN_EMPTY, the free-slot
    marker). update() takes device keys and does not look at them;
    callers with host keys use check_no_sentinel_key first."""

    # what an aggregate without input READS as (SUM/MIN/MAX); a MIN/MAX
    # slot itself starts at MM_NONE_BITS, see _slot_inits
    AGG_INIT = {0: 0.0, 1: float("inf"), 2: float("-inf")}

    @classmethod
    def _slot_inits(cls, agg_ops):
        """What a fresh record holds: 0 for SUM, MM_NONE_BITS for MIN/MAX
        (read back as AGG_INIT; see atomic_mm_f64 for why not +-inf)."""
        bits = [MM_NONE_BITS if op else 0 for op in agg_ops] or [0]
        return np.asarray(bits, dtype=np.uint64).view(np.float64)

    def __init__(self, expected_groups, nvals, stream=None, agg_ops=None):
        """agg_ops: per value column 0=SUM, 1=MIN, 2=MAX (default all SUM),
        the distributive ops of the two-phase rewrite (sql_utils.py)."""
        self.cap = _pow2_at_least(max(16, 2 * int(expected_groups)))
        self.nvals = nvals
        self.agg_ops = list(agg_ops) if agg_ops else [0] * nvals
        assert len(self.agg_ops) == nvals
        self.stream = stream
        # INTERLEAVED slot records [key | v0..v(nvals-1) | pad], rstride
        # pow2 8-byte words: find-or-insert touches ONE random HBM line
        # per row (key and values share the line) instead of one line in
        # the key array plus one per value array — the bound the
        # high-cardinality dedups (Q13/Q16/Q18/Q21) sit on
        self.rstride = 1
        while self.rstride < 1 + nvals:
            self.rstride <<= 1
        self.table = DevColumn(np.int64, self.cap * self.rstride)
        self._inits_dev = DevColumn.from_numpy(
            self._slot_inits(self.agg_ops))
        sh = stream.handle if stream else None
        shim.call("qk_groupby_init", sh, self.table.ptr, c_u64(self.cap),
                  self.rstride, self.nvals, self._inits_dev.ptr)
        self._ops_dev = None
        if any(self.agg_ops):
            self._ops_dev = DevColumn.from_numpy(
                np.asarray(self.agg_ops, dtype=np.int32))
        self.n_groups = 0           # exact, from the device insert counter
        self._nins = _count_buf()

    def update(self, keys_col, val_cols, n=None, max_new_groups=None):
        """max_new_groups: optional caller-known bound on DISTINCT keys
        this batch can introduce (e.g. the key domain size) — without it
        the growth check conservatively assumes every row is new."""
        n = keys_col.n if n is None else n
        if not n:
            return
        assert len(val_cols) == self.nvals
        # cumulative distinct keys can exceed the first batch's sizing: a
        # full table makes the kernel's find-or-insert loop spin forever,
        # so grow FIRST whenever this batch could push the exact group
        # count (device insert counter) past half capacity
        bound = n if max_new_groups is None else min(n, int(max_new_groups))
        if 2 * (self.n_groups + bound) > self.cap:
            self._grow(self.n_groups + bound)
        sh = self.stream.handle if self.stream else None
        ptrs = np.array([c.ptr.value if hasattr(c.ptr, "value") else c.ptr
                         for c in val_cols], dtype=np.uint64)
        dptrs = DevBuffer(ptrs.nbytes)
        shim.call("qk_h2d", dptrs.ptr, ptrs.ctypes.data_as(c_vp),
                  c_u64(ptrs.nbytes))
        shim.call("qk_groupby_i64_sum", sh, c_u64(n), keys_col.ptr,
                  dptrs.ptr, self._ops_dev.ptr if self._ops_dev else None,
                  self.nvals, self.rstride, self.table.ptr,
                  c_u64(self.cap), self._nins.ptr)
        if self.stream:
            self.stream.sync()
        self.n_groups = _read_u64(self._nins)
        dptrs.free()

    def _grow(self, need_groups):
        """Rebuild into a larger table (>= 4x the needed group count):
        extract the accumulated (keys, sums) and re-insert them — correct
        for SUM (adds into the zero start) and MIN/MAX alike: the fresh
        slot holds MM_NONE_BITS, which a number replaces and over which
        the NaN of an all-NaN group is written back as the canonical NaN.
        Mirrors GPUDistinctExecutor._grow."""
        keys, sums = self.extract()
        old_groups = len(keys)
        self.table.free()
        self.cap = _pow2_at_least(max(16, 4 * int(need_groups)))
        self.table = DevColumn(np.int64, self.cap * self.rstride)
        sh = self.stream.handle if self.stream else None
        shim.call("qk_groupby_init", sh, self.table.ptr, c_u64(self.cap),
                  self.rstride, self.nvals, self._inits_dev.ptr)
        shim.call("qk_dmemset", self._nins.ptr, 0, c_u64(8))
        self.n_groups = 0
        if old_groups:
            kcol = DevColumn.from_numpy(keys)
            vcols = [DevColumn.from_numpy(np.ascontiguousarray(sums[i]))
                     for i in range(self.nvals)]
            self.update(kcol, vcols, old_groups)
            kcol.free()
            for v in vcols:
                v.free()

    def extract(self):
        """-> (keys np.int64[K], sums np.float64[nvals, K]); unordered."""
        out_keys, out_sums, k, out_cap = self.extract_device()
        keys = out_keys.to_numpy(k)
        # d2h only the K occupied entries of each value column (the
        # compaction writes column c at [c*out_cap, c*out_cap + K) —
        # a full-capacity copy measured 100s of ms on 2^27-slot tables)
        sums = np.empty((self.nvals, k), dtype=np.float64)
        for c in range(self.nvals):
            if k:
                shim.call("qk_d2h", sums[c].ctypes.data_as(c_vp),
                          shim.c_vp(out_sums.ptr.value + c * out_cap * 8),
                          c_u64(k * 8))
        out_keys.free()
        out_sums.free()
        return keys, sums

    def extract_device(self):
        """Like extract() but the compacted (keys, sums) STAY ON DEVICE:
        returns (keys DevColumn i64 [n], sums DevColumn f64
        [nvals x out_cap, column-major with stride out_cap], n, out_cap).
        Caller frees both columns. Feeds device-side second-level
        aggregation (e.g. Q21's per-order distinct-supplier counts)."""
        sh = self.stream.handle if self.stream else None
        out_cap = self.cap
        out_keys = DevColumn(np.int64, out_cap)
        out_sums = DevColumn(np.float64, out_cap * self.nvals)
        cur = _count_buf()
        shim.call("qk_groupby_extract", sh, self.table.ptr,
                  self.rstride, self.nvals, c_u64(self.cap),
                  out_keys.ptr, out_sums.ptr, c_u64(out_cap), cur.ptr)
        if self.stream:
            self.stream.sync()
        k = _read_u64(cur)
        cur.free()
        out_keys.n = k
        return out_keys, out_sums, k, out_cap

    def extract_where_gt(self, col, threshold, out_guess=1 << 20):
        """Extract only groups whose sums[col] > threshold (HAVING — e.g.
        Q18's sum(l_quantity) > 300): the d2h stays proportional to the
        QUALIFYING groups, not the table. Returns (keys, sums) like
        extract(); reruns with a larger buffer if the guess undershoots
        (counted, never truncated)."""
        import ctypes as _ct
        sh = self.stream.handle if self.stream else None
        out_cap = min(self.cap, max(16, int(out_guess)))
        while True:
            out_keys = DevColumn(np.int64, out_cap)
            out_sums = DevColumn(np.float64, out_cap * self.nvals)
            cur = _count_buf()
            shim.call("qk_groupby_extract_gt", sh, self.table.ptr,
                      self.rstride, self.nvals, c_u64(self.cap),
                      int(col), _ct.c_double(float(threshold)),
                      out_keys.ptr, out_sums.ptr, c_u64(out_cap), cur.ptr)
            if self.stream:
                self.stream.sync()
            k = _read_u64(cur)
            cur.free()
            if k <= out_cap:
                keys = out_keys.to_numpy(k)
                sums = out_sums.to_numpy(out_cap * self.nvals).reshape(
                    self.nvals, out_cap)[:, :k].copy()
                out_keys.free()
                out_sums.free()
                return keys, sums
            out_keys.free()
            out_sums.free()
            out_cap = int(k)

    def free(self):
        self.table.free()
        self._inits_dev.free()
        self._nins.free()
        if self._ops_dev is not None:
            self._ops_dev.free()


def _arrow_string_buffers(col, who):
    """pyarrow string / large_string Array -> (offsets np.int64[n + 1]
    into data, data np.uint8), read with the offset width of the column's
    own type. Any other type is refused by name: binary and large_binary
    share the layout but are not strings, and anything else would be read
    with the wrong width. Arrow may leave out the data buffer (and, for an
    empty array, the offsets) when no row has bytes."""
    import pyarrow as pa
    large = pa.types.is_large_string(col.type)
    if not (large or pa.types.is_string(col.type)):
        raise TypeError("%s: not a string column (%s)" % (who, col.type))
    n = len(col)
    bufs = col.buffers()
    if n == 0 or bufs[1] is None:
        off = np.zeros(n + 1, dtype=np.int64)
    else:
        off = np.frombuffer(bufs[1], dtype=np.int64 if large else np.int32,
                            count=col.offset + n + 1)[col.offset:]
        off = off.astype(np.int64)
    if bufs[2] is None or bufs[2].size == 0:
        data = np.empty(0, dtype=np.uint8)
    else:
        data = np.frombuffer(bufs[2], dtype=np.uint8)
    return off, data


def str_hash_i64(col, stream=None):
    """pyarrow string / large_string / dictionary-of-string Array or
    ChunkedArray without nulls -> DevColumn i64 of n rows: the string
    dictionary's byte hash of each row, shifted right by one
    (qk_str_hash_i64). A pure function of the row's bytes, so
    partition_i64 over it places a string on the same channel in every
    call, process and rank."""
    import pyarrow as pa
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    if pa.types.is_dictionary(col.type):
        col = col.dictionary_decode() if hasattr(col, "dictionary_decode") \
            else col.cast(col.type.value_type)
    off, data = _arrow_string_buffers(col, "str_hash_i64")
    if col.null_count:
        raise TypeError("null string keys unsupported")
    n = len(col)
    out = DevColumn(np.int64, n)
    if n == 0:
        return out
    lo, hi = int(off[0]), int(off[-1])
    doff = DevColumn.from_numpy(off - lo if lo else off)
    dbytes = DevBuffer(max(1, hi - lo))
    if hi > lo:
        shim._bounce.h2d(dbytes.ptr, data[lo:hi])
    sh = stream.handle if stream else None
    shim.call("qk_str_hash_i64", sh, c_u64(n), doff.ptr, dbytes.ptr, out.ptr)
    if stream:
        stream.sync()
    else:
        shim.call("qk_stream_sync", None)
    doff.free()
    dbytes.free()
    return out


class DeviceStringDict:
    """Device-resident accumulating string dictionary: arbitrary-width,
    unbounded-cardinality string keys -> dense u32 codes, consistent
    across batches (the table and byte arena persist; growth re-seats
    hashes without changing codes). Replaces the round-1 host
    `staging.StringDict` (<=256 values) for join/group-by keys — the
    reference handles such keys inside polars (sql_executors.py:325-377,
    :556-599).

    encode(offsets, bytes) takes Arrow-layout string data (int64 offsets
    of n+1 entries + the byte buffer) and returns np.uint32 codes[n].
    `values` materializes decoded strings lazily (host list, index ==
    code)."""

    def __init__(self, expected=1024, stream=None):
        self.stream = stream
        self.cap = _pow2_at_least(max(64, 4 * int(expected)))
        self._alloc_table(self.cap)
        self.code_cap = max(1024, self.cap // 2)
        self.code_off = DevColumn(np.uint64, self.code_cap)
        self.code_len = DevColumn(np.uint32, self.code_cap)
        self.arena_cap = 1 << 20
        self.arena = DevBuffer(self.arena_cap)
        self._ctr = DevBuffer(16)           # [arena_cursor u64, counter u32]
        shim.call("qk_dmemset", self._ctr.ptr, 0, c_u64(16))
        self.n_codes = 0
        self.arena_used = 0
        self._values = []                   # host cache of bytes, by code
        self._strs = []                     # their decoded view, by code

    def _alloc_table(self, cap):
        self.slot_hash = DevColumn(np.uint64, cap)
        self.slot_code = DevColumn(np.int32, cap)
        shim.call("qk_dmemset", self.slot_hash.ptr, 0, c_u64(cap * 8))
        shim.call("qk_dmemset", self.slot_code.ptr, 0xFF, c_u64(cap * 4))

    @property
    def _cursor_ptrs(self):
        import ctypes as _ct
        return (self._ctr.ptr,
                shim.c_vp(self._ctr.ptr.value + 8))

    def encode(self, offsets, data, stream=None):
        """offsets: np.int64[n+1] (or any int np array), data: np.uint8
        bytes buffer. Returns np.uint32[n] codes."""
        st = stream or self.stream
        sh = st.handle if st else None
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if n <= 0:
            return np.empty(0, dtype=np.uint32)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        # worst case: every row is a new distinct string
        self._ensure(n, int(offsets[-1] - offsets[0]), sh)
        doff = DevColumn.from_numpy(offsets - offsets[0])
        dbytes = DevColumn.from_numpy(
            data[int(offsets[0]):int(offsets[-1])] if offsets[0] else
            data[: int(offsets[-1])])
        out = DevColumn(np.uint32, n)
        acur, cnt = self._cursor_ptrs
        shim.call("qk_str_dict_encode", sh, c_u64(n), doff.ptr, dbytes.ptr,
                  self.slot_hash.ptr, self.slot_code.ptr, c_u64(self.cap),
                  self.code_off.ptr, self.code_len.ptr, self.arena.ptr,
                  acur, cnt, out.ptr)
        if st:
            st.sync()
        else:
            shim.call("qk_stream_sync", None)
        host = np.zeros(2, dtype=np.uint64)
        shim.call("qk_d2h", host.ctypes.data_as(c_vp), self._ctr.ptr,
                  c_u64(16))
        self.arena_used = int(host[0])
        self.n_codes = int(np.uint64(host[1]) & np.uint64(0xFFFFFFFF))
        codes = out.to_numpy(n)
        doff.free(); dbytes.free(); out.free()
        return codes

    def encode_column(self, col, stream=None, nulls="raise"):
        """pyarrow string/large_string column -> np.uint32 codes.

        nulls="mask" accepts null strings and returns (codes, mask): mask
        is a host bool array, True = valid, or None when the column has no
        nulls. A null row is encoded as whatever bytes its offsets cover
        (usually none), so its code means nothing and the caller masks
        it. The default refuses nulls as before."""
        import pyarrow as pa
        if nulls not in ("raise", "mask"):
            raise ValueError("nulls must be 'raise' or 'mask', got %r"
                             % (nulls,))
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks()
        if pa.types.is_dictionary(col.type):
            col = col.dictionary_decode() if hasattr(col, "dictionary_decode") \
                else col.cast(col.type.value_type)
        off, data = _arrow_string_buffers(col, "DeviceStringDict."
                                          "encode_column")
        mask = None
        if col.null_count:
            if nulls == "raise":
                raise TypeError("null string keys unsupported")
            import pyarrow.compute as pc
            mask = np.ascontiguousarray(
                pc.is_valid(col).to_numpy(zero_copy_only=False), dtype=bool)
        codes = self.encode(off, data, stream)
        return (codes, mask) if nulls == "mask" else codes

    def _ensure(self, n_new, nbytes_new, sh):
        need_codes = self.n_codes + n_new
        if 2 * need_codes > self.cap:
            new_cap = _pow2_at_least(4 * need_codes)
            self.slot_hash.free(); self.slot_code.free()
            self._alloc_table(new_cap)
            self.cap = new_cap
            shim.call("qk_str_dict_rehash", sh, c_u32(self.n_codes),
                      self.code_off.ptr, self.code_len.ptr, self.arena.ptr,
                      self.slot_hash.ptr, self.slot_code.ptr,
                      c_u64(self.cap))
        if need_codes > self.code_cap:
            new_cc = _pow2_at_least(2 * need_codes)
            for name in ("code_off", "code_len"):
                old = getattr(self, name)
                new = DevColumn(old.dtype, new_cc)
                if self.n_codes:
                    shim.call("qk_d2d", new.ptr, old.ptr,
                              c_u64(self.n_codes * old.dtype.itemsize))
                old.free()
                setattr(self, name, new)
            self.code_cap = new_cc
        if self.arena_used + nbytes_new > self.arena_cap:
            new_ac = max(2 * self.arena_cap,
                         self.arena_used + nbytes_new)
            new_ar = DevBuffer(new_ac)
            if self.arena_used:
                shim.call("qk_d2d", new_ar.ptr, self.arena.ptr,
                          c_u64(self.arena_used))
            self.arena.free()
            self.arena = new_ar
            self.arena_cap = new_ac

    @property
    def values_bytes(self):
        """The stored strings as `bytes`, index == code (lazily
        materialized). Whatever encode() was given comes back as it is,
        UTF-8 or not."""
        if len(self._values) < self.n_codes:
            k0 = len(self._values)
            k = self.n_codes - k0
            offs = self.code_off.to_numpy(self.n_codes)[k0:]
            lens = self.code_len.to_numpy(self.n_codes)[k0:]
            lo = int(offs.min()) if k else 0
            hi = int((offs + lens).max()) if k else 0
            blob = np.empty(max(1, hi - lo), dtype=np.uint8)
            if hi > lo:
                shim.call("qk_d2h", blob.ctypes.data_as(c_vp),
                          shim.c_vp(self.arena.ptr.value + lo),
                          c_u64(hi - lo))
            raw = blob.tobytes()
            for o, ln in zip(offs, lens):
                s = int(o) - lo
                self._values.append(raw[s:s + int(ln)])
        return self._values

    @property
    def values(self):
        """Decoded strings, index == code: the UTF-8 view of
        values_bytes."""
        raw = self.values_bytes
        for b in raw[len(self._strs):]:
            self._strs.append(b.decode())
        return self._strs

    def decode(self, codes):
        vals = np.asarray(self.values, dtype=object)
        return vals[np.asarray(codes, dtype=np.int64)]

    def free(self):
        for c in (self.slot_hash, self.slot_code, self.code_off,
                  self.code_len):
            c.free()
        self.arena.free()
        self._ctr.free()


def _dev_ptr_array(cols):
    """Device array of the columns' pointers (the `T *const *` argument of
    the multi-column kernels). Caller frees."""
    ptrs = np.array([c.ptr.value if hasattr(c.ptr, "value") else c.ptr
                     for c in cols], dtype=np.uint64)
    buf = DevBuffer(ptrs.nbytes)
    shim.call("qk_h2d", buf.ptr, ptrs.ctypes.data_as(c_vp),
              c_u64(ptrs.nbytes))
    return buf


class DeviceKeyDict:
    """Device dictionary over K full-width key columns: each row's tuple
    of K 64-bit words -> a dense u32 code, the same in every later batch
    (slot array, key store and counter persist; growth re-seats the slots
    and copies the store, codes never change). What DeviceStringDict is
    for one string column, for the arbitrary groupby_keys / subset lists
    of SQLAggExecutor and DistinctExecutor (sql_executors.py:556-599,
    :517-554). No key value is reserved; growth is internal.

    nullable=True admits NULL keys (DESIGN.md §3a'''): rows are keyed on
    the K canonical words (0 under a null) plus W = ceil(K / 64) null
    words, so NULLs of one column equal each other, every null pattern is
    its own key, and what the caller's column holds under a null does not
    matter. W is always there, so batches with and without nulls share
    codes. encode() then takes one validity per key; keys_valid_host()
    gives the nulls back."""

    MAX_CODES = 2 ** 31 - 1

    def __init__(self, nkeys, expected=1024, stream=None, nullable=False):
        if int(nkeys) < 1:
            raise ValueError("DeviceKeyDict: nkeys must be >= 1")
        self.nkeys = int(nkeys)
        self.nullable = bool(nullable)
        # words per row in slots and store: the keys, then the null words
        self.nwords = self.nkeys + ((self.nkeys + 63) // 64
                                    if self.nullable else 0)
        self.stream = stream
        self.cap = _pow2_at_least(max(2, 2 * int(expected)))
        self.slots = self._new_slots(self.cap)
        self.code_cap = max(1, int(expected))
        self.store = DevColumn(np.int64, self.nwords * self.code_cap)
        self._ctr = DevBuffer(8)            # [counter u32, error u32]
        shim.call("qk_dmemset", self._ctr.ptr, 0, c_u64(8))
        self.n_codes = 0
        self._broken = False

    @staticmethod
    def _new_slots(cap):
        s = DevColumn(np.uint64, cap)
        shim.call("qk_dmemset", s.ptr, 0, c_u64(cap * 8))
        return s

    @property
    def _err_ptr(self):
        return shim.c_vp(self._ctr.ptr.value + 4)

    def _sync_state(self, sh, what):
        shim.call("qk_stream_sync", sh)
        host = np.zeros(2, dtype=np.uint32)
        shim.call("qk_d2h", host.ctypes.data_as(c_vp), self._ctr.ptr,
                  c_u64(8))
        if host[1]:
            self._broken = True
            raise RuntimeError(
                "DeviceKeyDict.%s: device error word %d (1 = probe walk "
                "exhausted the slot array, 2 = key store full); the "
                "dictionary is unusable" % (what, int(host[1])))
        self.n_codes = int(host[0])

    def _ensure(self, n, sh):
        need = self.n_codes + n
        if need > self.MAX_CODES:
            raise ValueError(
                "DeviceKeyDict: %d codes + %d rows exceeds the limit of "
                "2**31 - 1 groups" % (self.n_codes, n))
        if need > self.code_cap:
            new_cc = _pow2_at_least(2 * need)
            new = DevColumn(np.int64, self.nwords * new_cc)
            shim.call("qk_stream_sync", sh)
            if self.n_codes:
                for k in range(self.nwords):
                    shim.call(
                        "qk_d2d", shim.c_vp(new.ptr.value + k * new_cc * 8),
                        shim.c_vp(self.store.ptr.value
                                  + k * self.code_cap * 8),
                        c_u64(self.n_codes * 8))
            # the old store may be recycled by the pool: copies first
            shim.call("qk_stream_sync", None)
            self.store.free()
            self.store = new
            self.code_cap = new_cc
        if 2 * need > self.cap:
            self.slots.free()
            self.cap = _pow2_at_least(2 * need)
            self.slots = self._new_slots(self.cap)
            shim.call("qk_keydict_rehash", sh, c_u32(self.n_codes),
                      self.nwords, self.store.ptr, c_u64(self.code_cap),
                      self.slots.ptr, c_u64(self.cap), self._err_ptr)
            self._sync_state(sh, "rehash")

    def _null_words(self, key_cols, valid, n, sh):
        """The prepare pass of a nullable dictionary (qk_key_null_words):
        -> (the K + W word columns to encode, temporaries to free once the
        encode has run)."""
        if valid is None:
            valid = [None] * self.nkeys
        if len(valid) != self.nkeys:
            raise ValueError("DeviceKeyDict.encode: %d validity entries, "
                             "expected %d" % (len(valid), self.nkeys))
        tmp, bitmaps, canon = [], [], []

        def ptr_array(items):
            ptrs = np.array([0 if x is None else
                             getattr(x.ptr, "value", x.ptr) or 0
                             for x in items], dtype=np.uint64)
            buf = DevBuffer(ptrs.nbytes)
            tmp.append(buf)
            shim.call("qk_h2d", buf.ptr, ptrs.ctypes.data_as(c_vp),
                      c_u64(ptrs.nbytes))
            return buf.ptr
        try:
            for c, v in zip(key_cols, valid):
                bm, owned = _key_bitmap(c, v, n)
                if owned:
                    tmp.append(bm)
                bitmaps.append(bm)
                canon.append(None if bm is None else DevColumn(np.int64, n))
                if bm is not None:
                    tmp.append(canon[-1])
            nullw = [DevColumn(np.int64, n)
                     for _ in range(self.nwords - self.nkeys)]
            tmp.extend(nullw)
            shim.call("qk_key_null_words", sh, c_u64(n), self.nkeys,
                      ptr_array(key_cols), ptr_array(bitmaps),
                      ptr_array(canon), ptr_array(nullw))
        except Exception:
            for t in tmp:
                t.free()
            raise
        words = [c if k is None else k for c, k in zip(key_cols, canon)]
        return words + nullw, tmp

    def encode(self, key_cols, n=None, valid=None):
        """key_cols: K int64 DevColumns (one 64-bit word per row and key).
        Returns a DevColumn of u32 codes, n rows; caller frees.

        valid (nullable dictionaries only): one entry per key, a device
        bitmap in the NullableColumn.valid layout, a host bool mask (True
        = valid) or None for a key without nulls; a NullableColumn among
        key_cols supplies its own bitmap."""
        if self._broken:
            raise RuntimeError("DeviceKeyDict: unusable after a device "
                               "error")
        if valid is not None and not self.nullable:
            raise TypeError("DeviceKeyDict.encode: valid= needs a "
                            "dictionary made with nullable=True")
        if len(key_cols) != self.nkeys:
            raise ValueError("DeviceKeyDict.encode: %d key columns, "
                             "expected %d" % (len(key_cols), self.nkeys))
        for c in key_cols:
            if c.dtype != np.dtype(np.int64):
                raise TypeError("DeviceKeyDict.encode: key columns are "
                                "int64 words, got %s" % c.dtype)
        n = min(c.n for c in key_cols) if n is None else int(n)
        if any(c.n < n for c in key_cols):
            raise ValueError("DeviceKeyDict.encode: a key column is "
                             "shorter than n")
        if n >= 2 ** 32:
            raise ValueError("DeviceKeyDict.encode: at most 2**32 - 1 rows "
                             "per call")
        out = DevColumn(np.uint32, n)
        if not n:
            return out
        sh = self.stream.handle if self.stream else None
        self._ensure(n, sh)
        tmp = []
        if self.nullable:
            key_cols, tmp = self._null_words(key_cols, valid, n, sh)
        dptrs = _dev_ptr_array(key_cols)
        row_slot = DevColumn(np.uint64, n)
        shim.call("qk_keydict_encode", sh, c_u64(n), self.nwords, dptrs.ptr,
                  self.slots.ptr, c_u64(self.cap), self.store.ptr,
                  c_u64(self.code_cap), self._ctr.ptr, row_slot.ptr,
                  out.ptr, self._err_ptr)
        try:
            self._sync_state(sh, "encode")
        finally:
            dptrs.free()
            row_slot.free()
            for t in tmp:
                t.free()
        return out

    def keys_host(self):
        """-> list of K np.int64 arrays of n_codes words, index == code (in
        a nullable dictionary 0 wherever keys_valid_host() says NULL)."""
        outs = []
        for k in range(self.nkeys):
            a = np.empty(self.n_codes, dtype=np.int64)
            if self.n_codes:
                shim._bounce.d2h(a, shim.c_vp(
                    self.store.ptr.value + k * self.code_cap * 8))
            outs.append(a)
        return outs

    def keys_valid_host(self):
        """-> list of K bool arrays of n_codes entries, index == code,
        False where that key of the code is NULL (qk_nullword_to_valid
        over the null-word store columns)."""
        if not self.nullable:
            raise TypeError("DeviceKeyDict.keys_valid_host: the dictionary "
                            "was not made with nullable=True")
        g = self.n_codes
        sh = self.stream.handle if self.stream else None
        nb = valid_nbytes(g)
        bitmap = DevBuffer(nb)
        raw = np.empty(nb, dtype=np.uint8)
        outs = []
        for k in range(self.nkeys):
            cnt = _count_buf()
            shim.call("qk_nullword_to_valid", sh, c_u64(g), shim.c_vp(
                self.store.ptr.value
                + (self.nkeys + k // 64) * self.code_cap * 8), k % 64,
                bitmap.ptr, cnt.ptr)
            shim.call("qk_stream_sync", sh)
            shim.call("qk_d2h", raw.ctypes.data_as(c_vp), bitmap.ptr,
                      c_u64(nb))
            nulls = _read_u64(cnt)
            cnt.free()
            m = np.unpackbits(raw, bitorder="little")[:g].astype(bool)
            if g - int(m.sum()) != nulls:
                raise RuntimeError("DeviceKeyDict.keys_valid_host: bitmap "
                                   "and null count of key %d disagree" % k)
            outs.append(m)
        bitmap.free()
        return outs

    def free(self):
        self.slots.free()
        self.store.free()
        self._ctr.free()


class DenseAcc:
    """The accumulator half of GroupByKeys: one record of rstride (pow2 >=
    nvals) f64 words per dense code, SUM/MIN/MAX per agg_ops, growth by
    device copy, accumulate by a column of codes. The codes come from a
    DeviceKeyDict (GroupByKeys) or from the caller: the grand aggregate of
    GPUAggExecutor(null_values=True) runs it over an all-zero code column
    with one code.

    nullable_vals=True admits SQL NULLs among the values (DESIGN.md
    §3a''''): accumulate() then takes one validity per value column and
    launches qk_groupby_dense_acc_valid, a `seen` column beside the
    records (one u64 per code, bit c set once value column c of that code
    has received a value) grows with them, and extract_valid() says which
    aggregates are NULL. The bits of one word cap this at 64 value
    columns. With the default the launches are those of
    qk_groupby_dense_acc alone."""

    AGG_INIT = GroupByI64.AGG_INIT
    MAX_NULLABLE_VALS = 64

    def __init__(self, nvals, agg_ops=None, capacity=1024, stream=None,
                 nullable_vals=False, who="DenseAcc"):
        self.nvals = int(nvals)
        self.agg_ops = list(agg_ops) if agg_ops else [0] * self.nvals
        assert len(self.agg_ops) == self.nvals
        self.nullable_vals = bool(nullable_vals)
        self.who = who
        if self.nullable_vals and self.nvals > self.MAX_NULLABLE_VALS:
            raise ValueError(
                "%s: nullable_vals=True takes at most %d value columns "
                "(one bit each of a group's seen word), got %d"
                % (who, self.MAX_NULLABLE_VALS, self.nvals))
        self.stream = stream
        self.rstride = _pow2_at_least(max(1, self.nvals))
        self._inits_dev = DevColumn.from_numpy(
            GroupByI64._slot_inits(self.agg_ops))
        self._ops_dev = None
        if any(self.agg_ops):
            self._ops_dev = DevColumn.from_numpy(
                np.asarray(self.agg_ops, dtype=np.int32))
        self._err = DevBuffer(4)
        shim.call("qk_dmemset", self._err.ptr, 0, c_u64(4))
        self.cap = max(1, int(capacity))
        self.acc = DevColumn(np.float64, self.cap * self.rstride)
        self._init_records(self.acc, 0, self.cap)
        self.seen = None
        if self.nullable_vals:
            self.seen = DevColumn(np.uint64, self.cap)
            shim.call("qk_dmemset", self.seen.ptr, 0, c_u64(self.cap * 8))

    def _init_records(self, acc, first, count):
        sh = self.stream.handle if self.stream else None
        shim.call("qk_groupby_dense_init", sh, acc.ptr, c_u64(first),
                  c_u64(count), self.rstride, self.nvals,
                  self._inits_dev.ptr)

    def _grow_acc(self, need):
        """Records of existing codes move by device copy, bit for bit (a
        MIN/MAX slot's no-input and all-NaN patterns included); the new
        capacity starts at the slot starts of _slot_inits (0 for SUM,
        MM_NONE_BITS for MIN/MAX), and its seen words at 0."""
        new_cap = _pow2_at_least(2 * need)
        new = DevColumn(np.float64, new_cap * self.rstride)
        sh = self.stream.handle if self.stream else None
        shim.call("qk_stream_sync", sh)
        shim.call("qk_d2d", new.ptr, self.acc.ptr,
                  c_u64(self.cap * self.rstride * 8))
        self._init_records(new, self.cap, new_cap - self.cap)
        new_seen = None
        if self.seen is not None:
            new_seen = DevColumn(np.uint64, new_cap)
            shim.call("qk_d2d", new_seen.ptr, self.seen.ptr,
                      c_u64(self.cap * 8))
            shim.call("qk_dmemset",
                      shim.c_vp(new_seen.ptr.value + self.cap * 8), 0,
                      c_u64((new_cap - self.cap) * 8))
        shim.call("qk_stream_sync", sh)
        self.acc.free()
        self.acc = new
        if new_seen is not None:
            self.seen.free()
            self.seen = new_seen
        self.cap = new_cap

    def check_vals(self, val_cols, n, val_valid):
        """Host-only argument checks of accumulate(), for callers that
        must refuse before any device work of their own."""
        assert len(val_cols) == self.nvals
        for v in val_cols:
            if v.dtype != np.dtype(np.float64) or v.n < n:
                raise TypeError("%s.update: value columns are float64 with "
                                "at least n rows" % self.who)
        if self.nullable_vals:
            if val_valid is not None and len(val_valid) != self.nvals:
                raise ValueError("%s.update: %d value validity entries, "
                                 "expected %d" % (self.who, len(val_valid),
                                                  self.nvals))
        elif val_valid is not None or any(isinstance(v, NullableColumn)
                                          for v in val_cols):
            raise TypeError("%s.update: val_valid= or a NullableColumn "
                            "value needs a table made with "
                            "nullable_vals=True" % self.who)

    def accumulate(self, codes, ncodes, val_cols, n, val_valid=None):
        """Row i of the value columns goes into the record of codes[i]
        (u32 DevColumn, every code < ncodes). val_valid (nullable_vals=True
        only): one entry per value column, a device bitmap in the
        NullableColumn.valid layout, a host bool mask (True = valid) or
        None for a column without nulls; a NullableColumn among val_cols
        supplies its own bitmap."""
        self.check_vals(val_cols, n, val_valid)
        if not n or not self.nvals:
            return
        if ncodes > self.cap:
            self._grow_acc(ncodes)
        sh = self.stream.handle if self.stream else None
        ops_ptr = self._ops_dev.ptr if self._ops_dev else None
        tmp = []
        try:
            dptrs = _dev_ptr_array(val_cols)
            tmp.append(dptrs)
            if not self.nullable_vals:
                shim.call("qk_groupby_dense_acc", sh, c_u64(n), codes.ptr,
                          c_u32(ncodes), dptrs.ptr, ops_ptr, self.nvals,
                          self.rstride, self.acc.ptr, self._err.ptr)
            else:
                bitmaps = []
                for c, v in zip(val_cols, val_valid or [None] * self.nvals):
                    bm, owned = _key_bitmap(c, v, n, "value")
                    if owned:
                        tmp.append(bm)
                    bitmaps.append(0 if bm is None else
                                   getattr(bm.ptr, "value", bm.ptr) or 0)
                vptrs = DevColumn.from_numpy(
                    np.array(bitmaps, dtype=np.uint64))
                tmp.append(vptrs)
                shim.call("qk_groupby_dense_acc_valid", sh, c_u64(n),
                          codes.ptr, c_u32(ncodes), dptrs.ptr, vptrs.ptr,
                          ops_ptr, self.nvals, self.rstride, self.acc.ptr,
                          self.seen.ptr, self._err.ptr)
            shim.call("qk_stream_sync", sh)
        finally:
            for t in tmp:
                t.free()
        err = np.zeros(1, dtype=np.uint32)
        shim.call("qk_d2h", err.ctypes.data_as(c_vp), self._err.ptr,
                  c_u64(4))
        if err[0]:
            raise RuntimeError("%s.update: a code lay beyond the "
                               "accumulator records (device error word %d)"
                               % (self.who, int(err[0])))

    def extract(self, g):
        """-> np.float64 [nvals, g], column i the record of code i. An
        aggregate that met no value reads as its op identity (AGG_INIT;
        the MM_NONE_BITS of such a MIN/MAX slot is mapped here)."""
        recs = np.empty(g * self.rstride, dtype=np.float64)
        if g and self.nvals:
            shim.call("qk_stream_sync",
                      self.stream.handle if self.stream else None)
            shim._bounce.d2h(recs, self.acc.ptr)
        out = np.ascontiguousarray(
            recs.reshape(g, self.rstride)[:, :self.nvals].T)
        for c, op in enumerate(self.agg_ops):
            if op:  # a MIN/MAX slot no value reached
                out[c][out[c].view(np.uint64) == MM_NONE_BITS] = \
                    self.AGG_INIT[op]
        return out

    def extract_valid(self, g):
        """-> bool [nvals, g], False where that aggregate of code i is
        NULL (none of its inputs was a value)."""
        if not self.nullable_vals:
            raise TypeError("%s.extract_vals_valid: the table was not made "
                            "with nullable_vals=True" % self.who)
        words = np.empty(g, dtype=np.uint64)
        if g:
            shim.call("qk_stream_sync",
                      self.stream.handle if self.stream else None)
            shim._bounce.d2h(words, self.seen.ptr)
        bits = np.arange(self.nvals, dtype=np.uint64)[:, None]
        return ((words[None, :] >> bits) & np.uint64(1)).astype(bool)

    def free(self):
        self.acc.free()
        if self.seen is not None:
            self.seen.free()
        self._inits_dev.free()
        self._err.free()
        if self._ops_dev is not None:
            self._ops_dev.free()


class GroupByKeys:
    """Group-by over K full-width key columns with nvals f64 SUM/MIN/MAX
    columns: DeviceKeyDict codes, then one dense accumulate into the
    record of each row's code (SQLAggExecutor's DuckDB group-by over an
    arbitrary groupby_keys list, sql_executors.py:556-599). Because codes
    are dense the accumulate needs no second hash walk and extract() no
    compaction. Growth is internal; the group limit is 2**31 - 1.
    nullable_keys=True makes NULL a group, one per null pattern across the
    keys (DeviceKeyDict(nullable=True)); extract_valid() says where.
    nullable_vals=True lets the value columns hold NULLs, which SUM / MIN /
    MAX skip (DenseAcc); extract_vals_valid() says which aggregates met no
    value and are NULL."""

    AGG_INIT = GroupByI64.AGG_INIT

    def __init__(self, nkeys, nvals, agg_ops=None, expected_groups=1024,
                 stream=None, nullable_keys=False, nullable_vals=False):
        self.nvals = int(nvals)
        self.agg_ops = list(agg_ops) if agg_ops else [0] * self.nvals
        assert len(self.agg_ops) == self.nvals
        if nullable_vals and self.nvals > DenseAcc.MAX_NULLABLE_VALS:
            raise ValueError(
                "GroupByKeys: nullable_vals=True takes at most %d value "
                "columns (one bit each of a group's seen word), got %d"
                % (DenseAcc.MAX_NULLABLE_VALS, self.nvals))
        self.stream = stream
        self.nullable_vals = bool(nullable_vals)
        self.dict = DeviceKeyDict(nkeys, expected_groups, stream,
                                  nullable=nullable_keys)
        self._acc = DenseAcc(self.nvals, self.agg_ops, expected_groups,
                             stream, nullable_vals, who="GroupByKeys")

    @property
    def n_groups(self):
        return self.dict.n_codes

    @property
    def rstride(self):
        return self._acc.rstride

    @property
    def acc_cap(self):
        return self._acc.cap

    def update(self, key_cols, val_cols, n=None, key_valid=None,
               val_valid=None):
        """key_valid: one validity entry per key, as DeviceKeyDict.encode's
        `valid` (nullable_keys=True only). val_valid: one per value column
        in the same forms (nullable_vals=True only); a NullableColumn among
        val_cols supplies its own."""
        assert len(val_cols) == self.nvals
        n = min(c.n for c in key_cols) if n is None else int(n)
        if not n:
            return
        self._acc.check_vals(val_cols, n, val_valid)
        if key_valid is None:
            codes = self.dict.encode(key_cols, n)
        else:
            codes = self.dict.encode(key_cols, n, valid=key_valid)
        try:
            self._acc.accumulate(codes, self.dict.n_codes, val_cols, n,
                                 val_valid)
        finally:
            codes.free()

    def extract(self):
        """-> (list of K np.int64 key-word arrays [G], sums np.float64
        [nvals, G]); row g of every array belongs to code g. An aggregate
        that extract_vals_valid() calls NULL holds its op identity (0,
        +inf, -inf)."""
        g = self.dict.n_codes
        keys = self.dict.keys_host()
        return keys, self._acc.extract(g)

    def extract_valid(self):
        """-> list of K bool arrays [G], False where that key of group g is
        NULL; row g belongs to code g, as in extract()."""
        return self.dict.keys_valid_host()

    def extract_vals_valid(self):
        """-> bool array [nvals, G], False where that aggregate of group g
        is NULL: every input it was given was NULL (nullable_vals=True
        only). Row g belongs to code g, as in extract()."""
        return self._acc.extract_valid(self.dict.n_codes)

    def free(self):
        self.dict.free()
        self._acc.free()


class StringColumn:
    """Device-resident Arrow string column: `offsets` (DevColumn i32 or
    i64, n+1 entries starting at 0) + `data` (DevBuffer of the string
    bytes). The free-text columns the reference filters with LIKE inside
    DuckDB/polars (apps/tpc-h/tpch.py:380 o_comment, :413 s_comment, :316
    p_name) live on the device in this form."""

    def __init__(self, offsets, data, n):
        self.offsets = offsets
        self.data = data
        self.n = int(n)

    @classmethod
    def from_arrow(cls, col):
        """pyarrow string / large_string / dictionary-of-string Array or
        ChunkedArray -> StringColumn. The Arrow offsets and data buffers
        are uploaded as they are (no per-row host work); a sliced array
        uploads only the bytes its rows cover."""
        import pyarrow as pa
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks()
        if pa.types.is_dictionary(col.type):
            col = col.dictionary_decode() if hasattr(col, "dictionary_decode") \
                else col.cast(col.type.value_type)
        large = pa.types.is_large_string(col.type)
        if not (large or pa.types.is_string(col.type)):
            raise TypeError("StringColumn.from_arrow: not a string column "
                            "(%s)" % col.type)
        if col.null_count:
            raise TypeError("null strings unsupported")
        n = len(col)
        odt = np.int64 if large else np.int32
        bufs = col.buffers()
        if n == 0 or bufs[1] is None:
            off = np.zeros(n + 1, dtype=odt)
        else:
            off = np.frombuffer(bufs[1], dtype=odt,
                                count=col.offset + n + 1)[col.offset:]
        lo, hi = int(off[0]), int(off[-1])
        if lo:
            off = off - odt(lo)
        data = DevBuffer(hi - lo)
        if hi > lo:
            raw = np.frombuffer(bufs[2], dtype=np.uint8, count=hi)[lo:]
            shim._bounce.h2d(data.ptr, raw)
        return cls(DevColumn.from_numpy(off), data, n)

    def free(self):
        self.offsets.free()
        self.data.free()


def like(strcol, pattern, negate=False, exact=False, stream=None):
    """Per-row SQL LIKE over a StringColumn -> DevColumn u8 of 0/1 flags
    (DuckDB's default semantics: case-sensitive, % any run, _ one UTF-8
    code point, no ESCAPE). exact=True is string equality: every pattern
    byte literal. negate=True gives NOT LIKE / <>."""
    pat = shim.like_compile(pattern, exact)
    out = DevColumn(np.uint8, strcol.n)
    fn = "qk_str_like_i64" if strcol.offsets.dtype == np.dtype(np.int64) \
        else "qk_str_like_i32"
    sh = stream.handle if stream else None
    shim.call(fn, sh, c_u64(strcol.n), strcol.offsets.ptr, strcol.data.ptr,
              ctypes.byref(pat), int(bool(negate)), out.ptr)
    return out


def valid_nbytes(n):
    """Bytes of a validity bitmap for n rows: whole 64-bit words plus 8
    bytes of slack (include/quokka_amd.h)."""
    return ((int(n) + 63) // 64) * 8 + 8


def pack_valid(mask):
    """Host bool array -> validity bitmap bytes (np.uint8, valid_nbytes
    long, bits past the end 0)."""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(valid_nbytes(len(mask)), dtype=np.uint8)
    bits = np.packbits(mask, bitorder="little")
    out[:len(bits)] = bits
    return out


class NullableColumn:
    """A device column with SQL NULLs: `values` (DevColumn of n rows; null
    slots hold 0, so a kernel that ignores validity still reads defined
    data) + `valid` (DevBuffer, Arrow validity layout: bit i in byte
    i >> 3, LSB first, 1 = valid; valid_nbytes(n) long, every bit at an
    index >= n is 0). ptr/n/dtype delegate to `values`, so code that only
    wants the values keeps working. As a key column it supplies its bitmap
    to JoinTable.build / probe and to a DeviceKeyDict / GroupByKeys made
    nullable (DESIGN.md §3a'''); those paths never read the value under a
    null. Null strings outside key columns are not supported."""

    def __init__(self, values, valid, n, null_count):
        self.values = values
        self.valid = valid
        self.n = int(n)
        self.null_count = int(null_count)

    @property
    def ptr(self):
        return self.values.ptr

    @property
    def dtype(self):
        return self.values.dtype

    @classmethod
    def from_numpy(cls, values, mask):
        """Host values + bool mask (True = valid); null slots are zeroed."""
        mask = np.asarray(mask, dtype=bool)
        values = np.asarray(values)
        values = np.where(mask, values, np.zeros(1, dtype=values.dtype))
        bits = pack_valid(mask)
        vb = DevBuffer(len(bits))
        shim.call("qk_h2d", vb.ptr, bits.ctypes.data_as(c_vp),
                  c_u64(len(bits)))
        return cls(DevColumn.from_numpy(values), vb, len(mask),
                   int(len(mask) - mask.sum()))

    def valid_to_numpy(self):
        """-> host bool array of n rows (True = valid)."""
        raw = np.empty(valid_nbytes(self.n), dtype=np.uint8)
        shim.call("qk_d2h", raw.ctypes.data_as(c_vp), self.valid.ptr,
                  c_u64(raw.nbytes))
        return np.unpackbits(raw, bitorder="little")[:self.n].astype(bool)

    def to_numpy(self, n=None):
        return self.values.to_numpy(n)

    def valid_flags(self, stream=None):
        """-> DevColumn u8 of 0/1 validity flags (qk_valid_to_u8)."""
        out = DevColumn(np.uint8, max(1, self.n))
        out.n = self.n
        sh = stream.handle if stream else None
        shim.call("qk_valid_to_u8", sh, c_u64(self.n), self.valid.ptr,
                  out.ptr)
        return out

    def free(self):
        self.values.free()
        self.valid.free()


def take_nullable(col, idx, n_idx=None, stream=None):
    """col[idx] for a device u32 index column (a JitFilter result), nulls
    kept: the existing value gather plus qk_valid_gather. `col` may be a
    NullableColumn or a plain DevColumn (then every row is valid).
    Returns a NullableColumn."""
    n_idx = idx.n if n_idx is None else int(n_idx)
    sh = stream.handle if stream else None
    src = col.values if isinstance(col, NullableColumn) else col
    values = src.gather(idx, n_idx, stream)
    nb = valid_nbytes(n_idx)
    valid = DevBuffer(nb)
    if not isinstance(col, NullableColumn):
        bits = pack_valid(np.ones(n_idx, dtype=bool))
        shim.call("qk_h2d", valid.ptr, bits.ctypes.data_as(c_vp), c_u64(nb))
        return NullableColumn(values, valid, n_idx, 0)
    shim.call("qk_dmemset", valid.ptr, 0, c_u64(nb))
    cnt = _count_buf()
    shim.call("qk_valid_gather", sh, c_u64(n_idx), idx.ptr, col.valid.ptr,
              valid.ptr, cnt.ptr)
    shim.call("qk_stream_sync", sh)
    nulls = _read_u64(cnt)
    cnt.free()
    return NullableColumn(values, valid, n_idx, nulls)


NO_ROW = shim.NO_ROW    # QK_NO_ROW: JoinTable.probe(mode=3)'s "no build row"


def take_optional(col, idx, n_idx=None, stream=None):
    """col[idx] where idx (a device u32 index column) may hold NO_ROW:
    such a row, and a row whose source is NULL, comes back NULL with 0 in
    its slot. `col` is a NullableColumn or a plain DevColumn (every row
    valid). One qk_take_opt_* launch writes values, bitmap and null count;
    every index other than NO_ROW must be below col.n. Returns a
    NullableColumn."""
    n_idx = idx.n if n_idx is None else int(n_idx)
    sh = stream.handle if stream else None
    src = col.values if isinstance(col, NullableColumn) else col
    fn = shim._DTYPE_TAKE_OPT.get(src.dtype)
    if fn is None:
        raise TypeError("take_optional: unsupported dtype %s" % src.dtype)
    values = DevColumn(src.dtype, n_idx)
    nb = valid_nbytes(n_idx)
    valid = DevBuffer(nb)
    # the kernel writes whole words up to ceil(n_idx / 64); the slack word
    # behind them is zeroed here
    shim.call("qk_dmemset", c_vp(valid.ptr.value + nb - 8), 0, c_u64(8))
    cnt = _count_buf()
    shim.call(fn, sh, c_u64(n_idx), idx.ptr, src.ptr,
              col.valid.ptr if isinstance(col, NullableColumn) else None,
              values.ptr, valid.ptr, cnt.ptr)
    shim.call("qk_stream_sync", sh)
    nulls = _read_u64(cnt)
    cnt.free()
    return NullableColumn(values, valid, n_idx, nulls)


def sort_permutation(col, stream=None, descending=False):
    """Stable sort permutation of a DevColumn (i64/f64/i32/u32 keys):
    returns a u32 DevColumn `perm` with rows in ascending (or descending)
    key order; equal keys keep their original relative order (stable,
    like polars sort — sql_executors.py:369 build-side sort semantics).
    Device LSD radix sort (qk_sort_pairs_u64)."""
    n = col.n
    sh = stream.handle if stream else None
    keys = DevColumn(np.uint64, max(1, n))
    if col.dtype == np.dtype(np.float64):
        shim.call("qk_map_f64_u64", sh, c_u64(n), col.ptr, keys.ptr)
    elif col.dtype == np.dtype(np.int64):
        shim.call("qk_map_i64_u64", sh, c_u64(n), col.ptr, keys.ptr)
    elif col.dtype in (np.dtype(np.int32), np.dtype(np.uint32)):
        tmp = DevColumn(np.int64, max(1, n))
        host = col.to_numpy(n).astype(np.int64)   # widen via host (i32 cols are small in this path)
        tmp2 = DevColumn.from_numpy(host)
        shim.call("qk_map_i64_u64", sh, c_u64(n), tmp2.ptr, keys.ptr)
        tmp.free(); tmp2.free()
    else:
        raise TypeError("sort_permutation: unsupported dtype %s" % col.dtype)
    if descending:
        # stable descending == stable ascending on complemented key image
        shim.call("qk_bnot_u64", sh, c_u64(n), keys.ptr)
    perm = DevColumn(np.uint32, max(1, n))
    shim.call("qk_iota_u32", sh, c_u64(n), perm.ptr)
    ktmp = DevColumn(np.uint64, max(1, n))
    ptmp = DevColumn(np.uint32, max(1, n))
    shim.call("qk_sort_pairs_u64", sh, c_u64(n), keys.ptr, perm.ptr,
              ktmp.ptr, ptmp.ptr, -1)
    if stream:
        stream.sync()
    keys.free(); ktmp.free(); ptmp.free()
    perm.n = n
    return perm


def partition_i64(keys_col, nparts, stream=None, n=None):
    """Hash partition, int-key semantics key % nparts
    (quokka_runtime.py:222). Returns (offsets np.uint64[nparts+1],
    idx DevColumn u32 with rows grouped by partition)."""
    n = keys_col.n if n is None else n
    sh = stream.handle if stream else None
    hist = DevBuffer(nparts * 8)
    shim.call("qk_dmemset", hist.ptr, 0, c_u64(nparts * 8))
    shim.call("qk_partition_hist", sh, c_u64(n), keys_col.ptr,
              c_u32(nparts), hist.ptr)
    if stream:
        stream.sync()
    h = np.zeros(nparts, dtype=np.uint64)
    shim.call("qk_d2h", h.ctypes.data_as(c_vp), hist.ptr, c_u64(nparts * 8))
    offsets = np.zeros(nparts + 1, dtype=np.uint64)
    np.cumsum(h, out=offsets[1:])
    cursors = DevBuffer(nparts * 8)
    shim.call("qk_h2d", cursors.ptr,
              np.ascontiguousarray(offsets[:nparts]).ctypes.data_as(c_vp),
              c_u64(nparts * 8))
    idx = DevColumn(np.uint32, max(1, n))
    shim.call("qk_partition_scatter", sh, c_u64(n), keys_col.ptr,
              c_u32(nparts), cursors.ptr, idx.ptr)
    if stream:
        stream.sync()
    hist.free()
    cursors.free()
    idx.n = n
    return offsets, idx
