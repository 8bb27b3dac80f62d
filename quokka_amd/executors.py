"""Drop-in Executor subclasses and partition function for pyquokka.

These mirror the reference's plugin boundary exactly
(pyquokka/executors/base_executor.py:26-32, call sites core.py:632/:667,
task.py:131-134): stateful objects whose `execute(batches, stream_id,
channel_id)` consumes `list[pyarrow.Table]` and whose `done(channel_id)`
flushes. Stream mapping for joins: stream 1 = build, stream 0 = probe
(logical.py:459-471). Objects must be picklable at registration time
(quokka_runtime.py:325) — all GPU state is created lazily on first
execute, never in __init__.

A pyquokka deployment drops these in at lowering time in place of
BuildProbeJoinExecutor / SQLAggExecutor."""
import re

import numpy as np


class Executor:
    """= pyquokka.executors.base_executor.Executor (:26-32)."""

    def __init__(self):
        raise NotImplementedError

    def execute(self, batches, stream_id, executor_id):
        raise NotImplementedError

    def done(self, executor_id):
        raise NotImplementedError


def _lazy_gpu():
    """Import the HIP shim at first use (fails loudly without the .so /
    a GPU; keeps executors picklable before first execute)."""
    from . import ops, shim, staging
    return ops, shim, staging


def _to_table(d):
    import pyarrow as pa
    return pa.table({k: v for k, v in d.items()})


def _is_stringish(col):
    """pyarrow string / large_string / dictionary-of-string column."""
    import pyarrow as pa
    t = col.type
    if pa.types.is_dictionary(t):
        t = t.value_type
    return pa.types.is_string(t) or pa.types.is_large_string(t)


class _ArrowStrings:
    """A string key column of gpu_partition_fn kept as its Arrow array
    (chunks combined, a dictionary decoded) next to the numpy host
    columns: dtype object like the raw string columns, rows selected
    with take. The key is hashed on the device from the Arrow offsets
    and bytes, so no Python string per row is ever made."""
    dtype = np.dtype(object)

    def __init__(self, col):
        import pyarrow as pa
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks()
        if pa.types.is_dictionary(col.type):
            col = col.dictionary_decode() if hasattr(col, "dictionary_decode") \
                else col.cast(col.type.value_type)
        self.arr = col

    def __len__(self):
        return len(self.arr)

    def __getitem__(self, sel):
        return _ArrowStrings(self.arr.take(sel))


def _concat_col(parts):
    import pyarrow as pa
    chunks = []
    for p in parts:
        chunks.extend(p.chunks if isinstance(p, pa.ChunkedArray) else [p])
    return pa.chunked_array(chunks)


def _split_payload(name, col, staging):
    """One numeric join payload column (null_payloads=True) -> (host values
    in the device storage type, bool mask or None when it has no nulls).
    bool is stored as uint8, date32 as int32, narrow ints as int64 and
    float32 as float64 (all exact, cast back at emit); int64 stays int64.
    Anything else raises TypeError: nothing is staged approximately."""
    import pyarrow as pa
    t = col.type
    if not (pa.types.is_boolean(t) or pa.types.is_date32(t) or
            pa.types.is_signed_integer(t) or pa.types.is_uint8(t) or
            pa.types.is_uint32(t) or pa.types.is_float32(t) or
            pa.types.is_float64(t)):
        raise TypeError("join payload column %r: type %s unsupported with "
                        "null_payloads=True (ints, date32, bool, floats and "
                        "strings are)" % (name, t))
    if not col.null_count:
        return staging.column_to_numpy(col), None
    filled, mask = staging.split_nulls(col)
    return staging.column_to_numpy(filled), mask


def _payload_device(ops, shim, values, mask):
    """Staged payload -> DevColumn, or NullableColumn when it has nulls."""
    if mask is None or mask.all():
        return shim.DevColumn.from_numpy(values)
    return ops.NullableColumn.from_numpy(values, mask)


def _take_to_arrow(ops, src, idx, n_idx, arrow_type):
    """src[idx] through the optional gather (NO_ROW and source nulls come
    back NULL) as a host Arrow array of arrow_type; the cast from the
    storage type keeps the validity buffer."""
    from . import bridge
    g = ops.take_optional(src, idx, n_idx)
    arr = bridge.column_to_arrow(g)
    g.free()
    return arr if arr.type == arrow_type else arr.cast(arrow_type)


def _take_strings(col, rows, no_row=None):
    """Host Arrow take of a string column at device-produced row indices;
    an index equal to no_row selects NULL."""
    import pyarrow as pa
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    mask = None if no_row is None else rows == no_row
    return col.take(pa.array(rows.astype(np.int64), mask=mask))


class GPUBuildProbeJoinExecutor(Executor):
    """GPU replacement for BuildProbeJoinExecutor (sql_executors.py:325-377).

    Same constructor signature and argument meaning; same stream contract
    (1 = build, vstacked into state; 0 = probe, one result per probe batch);
    same `how` set {inner, left, semi, anti}; key_to_keep renames the key
    column like :372-373. Differences documented in DESIGN.md: the build
    state is a device hash table (the reference's vstack+sort+polars-join is
    an implementation detail, :358/:369); result row ORDER within a batch is
    unspecified (as is polars'). i64 keys supported.

    null_keys=True admits NULL join keys, int or string, on both sides: a
    NULL matches nothing, as in polars, so inner and semi drop such rows
    and left and anti keep the probe's, with the key column still in its
    type and NULL (DESIGN.md §3a'''). The default refuses or mangles them
    as before.

    null_payloads=True keeps NULLs in the non-key columns of both sides and
    hands every column back in the Arrow type it arrived in: numeric
    payloads travel as value + validity bitmap and are emitted by one
    optional gather per column, strings by an Arrow take with the device
    indices, and how="left" is a single left probe whose unmatched rows
    carry NO_ROW, which the gather turns into NULL (DESIGN.md §3a''''').
    The output of such a join is a valid input of the next one. A payload
    type the device cannot hold raises TypeError naming the column."""

    def __init__(self, on=None, left_on=None, right_on=None, how="inner",
                 key_to_keep="left", null_keys=False, null_payloads=False):
        if on is not None:
            if left_on is not None or right_on is not None:
                raise ValueError("pass either on= or left_on=/right_on=, "
                                 "not both (sql_executors.py:327-343)")
            self.left_on = on
            self.right_on = on
        else:
            if left_on is None or right_on is None:
                raise ValueError("join needs on= or both left_on= and "
                                 "right_on=")
            self.left_on = left_on
            self.right_on = right_on
        if how not in {"inner", "left", "semi", "anti"}:
            raise ValueError("unsupported join how=%r (inner/left/semi/"
                             "anti, as the reference)" % (how,))
        self.how = how
        self.key_to_keep = key_to_keep
        self.null_keys = bool(null_keys)
        self.null_payloads = bool(null_payloads)
        self._build_key_masks = []  # null_keys: one bool mask per batch
        # null_payloads: per numeric payload column, one bool mask (or None,
        # no nulls) per build batch, and the Arrow type to hand back
        self._build_pay_masks = {}
        self._build_types = {}
        self.phase = "build"
        # lazy GPU state (created on first execute, never in __init__)
        self._table = None
        self._build_cols = None     # dict name -> list of numpy arrays
        self._build_names = None
        self._key_dict = None       # DeviceStringDict for string keys
        self._build_payload_host = {}

    def __getstate__(self):
        assert self._table is None, "executor must be pickled before first execute"
        d = dict(self.__dict__)
        return d

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        ops, shim, staging = _lazy_gpu()
        batches = [b for b in batches if b is not None and len(b) > 0]
        if len(batches) == 0:
            return
        batch = pa.concat_tables(batches)

        if stream_id == 1:                       # build (state vstack)
            assert self.phase == "build"
            self._stage_build_batch(batch)
            return

        # probe
        if self._table is None and self._build_cols is None:
            if self.how == "anti":
                return batch
            return
        if self.phase == "build":
            self._finish_build()
        self.phase = "probe"
        return self._probe(batch)

    def _stage_build_batch(self, batch):
        ops, shim, staging = _lazy_gpu()
        if self._build_cols is None:
            self._build_names = [c for c in batch.column_names]
            self._build_cols = {c: [] for c in self._build_names}
        for c in self._build_names:
            col = batch.column(c)
            if _is_stringish(col):
                # string columns stay Arrow until _finish_build:
                # KEYS go through the device string dictionary,
                # payloads are host-gathered at emit
                self._build_cols[c].append(col)
            elif self.null_keys and c == self.right_on:
                # the key's mask travels beside its values, so an int
                # key with nulls stays int
                mask = np.ones(len(col), dtype=bool)
                if col.null_count:
                    col, mask = staging.split_nulls(col)
                self._build_cols[c].append(staging.column_to_numpy(col))
                self._build_key_masks.append(mask)
            elif self.null_payloads and c != self.right_on:
                vals, mask = _split_payload(c, col, staging)
                self._build_cols[c].append(vals)
                self._build_pay_masks.setdefault(c, []).append(mask)
                self._build_types[c] = col.type
            else:
                self._build_cols[c].append(
                    staging.column_to_numpy(col))

    def _encode_string_keys(self, col):
        """String key column -> (i64 dictionary codes, bool mask or None).
        Without null_keys nulls raise, as before."""
        if not self.null_keys:
            return self._key_dict.encode_column(col).astype(np.int64), None
        codes, mask = self._key_dict.encode_column(col, nulls="mask")
        return codes.astype(np.int64), mask

    def _finish_build(self):
        ops, shim, staging = _lazy_gpu()
        self._host_build = {}
        self._build_payload_host = {}     # string payloads, host-gathered
        kmask = None                      # null_keys: validity of the keys
        if self._build_key_masks:
            kmask = np.concatenate(self._build_key_masks)
            self._build_key_masks = []
        for c, v in self._build_cols.items():
            if v and not isinstance(v[0], np.ndarray):
                col = _concat_col(v)
                if c == self.right_on:
                    # string join key: device string dictionary -> dense
                    # codes; probe side encodes into the SAME dict so
                    # equal strings get equal codes (bytes verified)
                    self._key_dict = ops.DeviceStringDict(
                        expected=max(1024, col.length()))
                    self._host_build[c], kmask = \
                        self._encode_string_keys(col)
                elif self.null_payloads:
                    # stays Arrow: taken with the build indices at emit
                    self._build_payload_host[c] = col.combine_chunks()
                else:
                    self._build_payload_host[c] = np.asarray(
                        col.to_pylist(), dtype=object)
            else:
                arr = np.concatenate(v)
                if arr.dtype == object:   # broadcast-join host strings
                    import pyarrow as pa
                    if c == self.right_on:
                        self._key_dict = ops.DeviceStringDict(
                            expected=max(1024, len(arr)))
                        self._host_build[c], kmask = \
                            self._encode_string_keys(
                                pa.chunked_array([pa.array(arr)]))
                    else:
                        self._build_payload_host[c] = arr
                else:
                    self._host_build[c] = arr
        keys = self._host_build[self.right_on]
        if keys.dtype != np.int64:
            if keys.dtype.kind in "iu":   # any int key, as the reference
                keys = keys.astype(np.int64)
            else:
                raise TypeError("GPU join requires integer or string keys,"
                                " got %s" % keys.dtype)
        if kmask is not None and kmask.all():
            kmask = None
        if self._key_dict is None:      # dictionary codes are >= 0
            ops.check_no_sentinel_key(
                keys if kmask is None else keys[kmask],
                type(self).__name__, self.right_on)
        n = len(keys)
        self._table = ops.JoinTable(max(16, n))
        if n:
            kcol = shim.DevColumn.from_numpy(keys)
            if kmask is None:
                self._table.build(kcol)
            else:
                self._table.build(kcol, valid=kmask)
            kcol.free()
        self._build_payload_dev = {}
        for c in self._build_names:
            if c == self.right_on or c in self._build_payload_host:
                continue
            masks = self._build_pay_masks.get(c)
            if masks is None or all(m is None for m in masks):
                self._build_payload_dev[c] = shim.DevColumn.from_numpy(
                    self._host_build[c])
                continue
            # a batch without nulls gets an all-true mask beside the others
            mask = np.concatenate([
                np.ones(len(v), dtype=bool) if m is None else m
                for v, m in zip(self._build_cols[c], masks)])
            self._build_payload_dev[c] = _payload_device(
                ops, shim, self._host_build[c], mask)
        self._build_pay_masks = {}
        self._build_cols = None

    def _stage_probe_keys(self, key_col):
        """Probe key column -> (i64 host keys, bool mask or None, the
        numeric key 0-filled under nulls or None)."""
        ops, shim, staging = _lazy_gpu()
        pmask = None            # null_keys: validity of the probe keys
        key_vals = None         # ... and the numeric key, 0 under nulls
        if _is_stringish(key_col):
            if self._key_dict is None:
                raise TypeError("string probe keys against a non-string "
                                "build side")
            # same device dictionary as the build side: equal strings ==
            # equal codes (bytes verified in-kernel)
            probe_keys, pmask = self._encode_string_keys(key_col)
        elif self.null_keys and key_col.null_count:
            filled, pmask = staging.split_nulls(key_col)
            probe_keys = key_vals = staging.column_to_numpy(filled)
        else:
            probe_keys = staging.column_to_numpy(key_col)
        if probe_keys.dtype != np.int64:
            if probe_keys.dtype.kind in "iu":
                probe_keys = probe_keys.astype(np.int64)
            else:
                raise TypeError("GPU join requires integer or string keys,"
                                " got %s" % probe_keys.dtype)
        return probe_keys, pmask, key_vals

    def _probe_null_payloads(self, batch):
        """null_payloads=True: one probe (left = mode 3, whose misses carry
        NO_ROW), then every column through the optional gather, which
        writes value and validity together."""
        import pyarrow as pa
        ops, shim, staging = _lazy_gpu()
        key_col = batch.column(self.left_on)
        probe_keys, pmask, _ = self._stage_probe_keys(key_col)
        kcol = _payload_device(ops, shim, probe_keys, pmask)
        mode = {"inner": 0, "left": 3, "semi": 1, "anti": 2}[self.how]
        pidx, bidx, nm = self._table.probe(kcol, mode=mode)
        sel = bsel = None       # host copies of the indices, for strings
        out = {}
        for c in batch.column_names:
            col = batch.column(c)
            if _is_stringish(col):
                if sel is None:
                    sel = pidx.to_numpy(nm)
                out[c] = _take_strings(col, sel)
            elif c == self.left_on:
                # the staged i64 key, with its bitmap when it has nulls
                out[c] = _take_to_arrow(ops, kcol, pidx, nm, col.type)
            else:
                src = _payload_device(ops, shim,
                                      *_split_payload(c, col, staging))
                out[c] = _take_to_arrow(ops, src, pidx, nm, col.type)
                src.free()
        if bidx is not None:
            for c, dev in self._build_payload_dev.items():
                out[c] = _take_to_arrow(ops, dev, bidx, nm,
                                        self._build_types[c])
            for c, arr in self._build_payload_host.items():
                if bsel is None:
                    bsel = bidx.to_numpy(nm)
                out[c] = _take_strings(arr, bsel, no_row=ops.NO_ROW)
            bidx.free()
        pidx.free()
        kcol.free()
        # as the default path's rename: the renamed key goes last
        if self.key_to_keep == "right" and self.left_on != self.right_on:
            out[self.right_on] = out.pop(self.left_on)
        return pa.table(out)

    def _probe(self, batch):
        if self.null_payloads:
            return self._probe_null_payloads(batch)
        ops, shim, staging = _lazy_gpu()
        key_col = batch.column(self.left_on)
        probe_keys, pmask, key_vals = self._stage_probe_keys(key_col)
        kcol = shim.DevColumn.from_numpy(probe_keys)
        mode = {"inner": 0, "left": 0, "semi": 1, "anti": 2}[self.how]
        if pmask is None:
            pidx, bidx, nm = self._table.probe(kcol, mode=mode)
        else:
            pidx, bidx, nm = self._table.probe(kcol, mode=mode, valid=pmask)

        def dev_gather(host_arr, idx_col):
            """stage -> device gather by idx -> one DMA into a PINNED
            buffer (the payload gather is the polars-join emit step,
            sql_executors.py:371; pyarrow wraps the pinned array
            zero-copy — quokka_amd.bridge, §8f row 3)."""
            from . import bridge
            src = shim.DevColumn.from_numpy(host_arr)
            g = src.gather(idx_col, nm)
            res = bridge.to_pinned_numpy(g, nm)
            src.free()
            g.free()
            return res

        # the reference renames the kept key column after EVERY join emit
        # (sql_executors.py:372-373), regardless of how/path
        def rename_key(cols):
            if self.key_to_keep == "right" and self.left_on != self.right_on \
                    and self.left_on in cols:
                cols[self.right_on] = cols.pop(self.left_on)
            return cols

        sel = pidx.to_numpy(nm)

        def probe_col_rows(c, rows_dev, rows_host):
            """One probe-side column at the selected rows: strings gather
            host-side (emit is host Arrow anyway), numerics through the
            device gather like the reference's polars emit."""
            col = batch.column(c)
            if c == self.left_on and pmask is not None:
                return null_key_rows(col, rows_dev, rows_host)
            if _is_stringish(col):
                return np.asarray(col.to_pylist(), dtype=object)[rows_host]
            return dev_gather(staging.column_to_numpy(col), rows_dev)

        def null_key_rows(col, rows_dev, rows_host):
            """The key column when it holds nulls (null_keys=True): type
            and nulls kept. Only anti emits null-key rows from the device
            indices; inner, semi and the matched part of left select none,
            so the filled values are gathered as any numeric column."""
            import pyarrow as pa
            if key_vals is None:        # string key: Arrow take on the host
                return col.combine_chunks().take(
                    pa.array(rows_host, type=pa.int64()))
            if self.how != "anti" or not nm:
                return dev_gather(key_vals, rows_dev)
            from . import bridge
            src = ops.NullableColumn.from_numpy(key_vals, pmask)
            g = ops.take_nullable(src, rows_dev, nm)
            res = bridge.column_to_arrow(g)
            src.free()
            g.free()
            return res

        out = {}
        if self.how in ("semi", "anti"):
            for c in batch.column_names:
                out[c] = probe_col_rows(c, pidx, sel)
        else:
            for c in batch.column_names:
                out[c] = probe_col_rows(c, pidx, sel)
            bsel = bidx.to_numpy(nm)
            from . import bridge
            for c, dev in self._build_payload_dev.items():
                g = dev.gather(bidx, nm)
                out[c] = bridge.to_pinned_numpy(g, nm)
                g.free()
            for c, arr in self._build_payload_host.items():
                out[c] = arr[bsel]
            if self.how == "left":
                # unmatched probe rows appended with null build payload
                matched = np.zeros(len(probe_keys), dtype=bool)
                matched[sel] = True
                un = np.nonzero(~matched)[0]
                if len(un):
                    import pyarrow as pa
                    for c in batch.column_names:
                        col = batch.column(c)
                        if c == self.left_on and pmask is not None:
                            # unmatched rows include every null-key row
                            if key_vals is None:
                                tail = col.combine_chunks().take(
                                    pa.array(un, type=pa.int64()))
                                head = out[c]
                            else:
                                tail = pa.array(key_vals[un],
                                                mask=~pmask[un])
                                head = pa.array(out[c])
                            out[c] = pa.concat_arrays([head, tail])
                            continue
                        if _is_stringish(col):
                            tailv = np.asarray(col.to_pylist(),
                                               dtype=object)[un]
                        else:
                            tailv = staging.column_to_numpy(col)[un]
                        out[c] = np.concatenate([out[c], tailv])
                    probe_cols = rename_key(
                        {k: v for k, v in out.items()
                         if k in batch.column_names})
                    tbl = _to_table(probe_cols)
                    pay = {}
                    for c in (list(self._build_payload_dev) +
                              list(self._build_payload_host)):
                        a = pa.array(out[c])
                        pay[c] = pa.chunked_array([
                            a, pa.nulls(len(un), a.type)])
                    for c, v in pay.items():
                        tbl = tbl.append_column(c, v)
                    pidx.free()
                    if bidx:
                        bidx.free()
                    kcol.free()
                    return tbl
        rename_key(out)
        pidx.free()
        if bidx:
            bidx.free()
        kcol.free()
        return _to_table(out)

    def done(self, executor_id):
        pass


_AGG_RE = re.compile(r"(sum|min|max)\s*\(\s*([A-Za-z_][A-Za-z0-9_]*)\s*\)",
                     re.I)
_AGG_OP = {"sum": 0, "min": 1, "max": 2}

_CANON_NAN = np.float64(np.nan)


def key_to_words(arr):
    """Host numpy key column -> np.int64 words, one per row, such that two
    rows hold equal words exactly when SQL puts them in one group:
    bool and signed/unsigned ints are widened (uint64 keeps its bit
    pattern), datetime64/timedelta64 give their integer count, floats give
    the float64 bit pattern with -0.0 turned into +0.0 and every NaN into
    one canonical NaN. words_to_key is the inverse."""
    arr = np.asarray(arr)
    kind = arr.dtype.kind
    if kind == "b":
        return arr.astype(np.int64)
    if kind == "i":
        return arr.astype(np.int64)
    if kind == "u":
        if arr.dtype.itemsize == 8:
            return np.ascontiguousarray(arr).view(np.int64)
        return arr.astype(np.int64)
    if kind in "mM":
        return np.ascontiguousarray(arr).view(np.int64)
    if kind == "f":
        f = arr.astype(np.float64)              # a copy
        f[np.isnan(f)] = _CANON_NAN
        f += 0.0                                # -0.0 + 0.0 == +0.0
        return f.view(np.int64)
    raise TypeError("key_to_words: unsupported key dtype %s" % arr.dtype)


def words_to_key(words, dtype):
    """Inverse of key_to_words for a column of numpy dtype `dtype` (a
    float32 column comes back as float32, exactly)."""
    words = np.ascontiguousarray(words, dtype=np.int64)
    dtype = np.dtype(dtype)
    kind = dtype.kind
    if kind == "b":
        return words != 0
    if kind == "i":
        return words.astype(dtype)
    if kind == "u":
        if dtype.itemsize == 8:
            return words.view(np.uint64)
        return words.astype(dtype)
    if kind in "mM":
        return words.view(dtype)
    if kind == "f":
        return words.view(np.float64).astype(dtype)
    raise TypeError("words_to_key: unsupported key dtype %s" % dtype)


class _KeyWords:
    """Per-executor state that turns the key columns of a batch into
    64-bit words (one np.int64 array per key) and back: the Arrow type of
    each key from the first batch, and one DeviceStringDict per string
    key. Numeric, bool and date/time keys convert on the host through
    key_to_words; a string key's word is its dictionary code.

    null_keys=True admits NULL keys: words() then also returns one host
    bool mask (True = valid) or None per key, the word under a null is 0,
    and decode() / to_arrow() take the mask back."""

    def __init__(self, names, null_keys=False):
        self.names = list(names)
        self.null_keys = bool(null_keys)
        self.types = {}
        self.dicts = {}

    @staticmethod
    def _storage(col):
        """Arrow key column -> numpy array key_to_words accepts."""
        import pyarrow as pa
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks()
        t = col.type
        if pa.types.is_dictionary(t):
            col = col.dictionary_decode() if hasattr(col, "dictionary_decode") \
                else col.cast(t.value_type)
            t = col.type
        if pa.types.is_date32(t) or pa.types.is_time32(t):
            return col.cast(pa.int32()).to_numpy(zero_copy_only=False)
        if pa.types.is_temporal(t):
            return col.cast(pa.int64()).to_numpy(zero_copy_only=False)
        if pa.types.is_boolean(t) or pa.types.is_integer(t) or \
                pa.types.is_floating(t):
            return col.to_numpy(zero_copy_only=False)
        raise TypeError("unsupported group key type %s" % t)

    def check(self, batch, who):
        """Host-only: refuse null keys before any device work."""
        if self.null_keys:
            return
        for k in self.names:
            if batch.column(k).null_count:
                raise TypeError(
                    "%s: key column %r has nulls; null keys are not "
                    "supported (DESIGN.md §3a')" % (who, k))

    @staticmethod
    def _split_nulls(col):
        """Arrow key column with nulls -> (the column with its null slots
        filled with 0, host bool mask). staging.split_nulls for numeric,
        bool and date32 keys, so ints stay ints; the other temporal types,
        which it refuses, through their integer storage here."""
        import pyarrow as pa
        import pyarrow.compute as pc
        from . import staging
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks()
        t = col.type
        if pa.types.is_temporal(t) and not pa.types.is_date32(t):
            mask = pc.is_valid(col).to_numpy(zero_copy_only=False)
            store = pa.int32() if pa.types.is_time32(t) else pa.int64()
            return (col.cast(store).fill_null(0),
                    np.ascontiguousarray(mask, dtype=bool))
        return staging.split_nulls(col)

    def words(self, batch, ops):
        """-> one np.int64 word array per key; with null_keys=True
        (words, masks), masks[k] a host bool array or None."""
        outs, masks = [], []
        for k in self.names:
            col = batch.column(k)
            self.types.setdefault(k, col.type)
            mask = None
            if _is_stringish(col):
                sd = self.dicts.get(k)
                if sd is None:
                    sd = self.dicts[k] = ops.DeviceStringDict(expected=4096)
                if self.null_keys:
                    codes, mask = sd.encode_column(col, nulls="mask")
                    w = codes.astype(np.int64)
                    if mask is not None:
                        w[~mask] = 0
                    outs.append(w)
                else:
                    outs.append(sd.encode_column(col).astype(np.int64))
            elif self.null_keys and col.null_count:
                filled, mask = self._split_nulls(col)
                outs.append(key_to_words(self._storage(filled)))
            else:
                outs.append(key_to_words(self._storage(col)))
            masks.append(mask)
        return (outs, masks) if self.null_keys else outs

    def decode(self, name, words, mask=None):
        """words -> numpy values that sort like the column (strings as an
        object array, dates as their integer count). With a mask, string
        rows that are NULL come back as '' (their word is no code)."""
        import pyarrow as pa
        t = self.types[name]
        sd = self.dicts.get(name)
        if sd is not None and mask is not None:
            out = np.full(len(words), "", dtype=object)
            out[mask] = sd.decode(np.asarray(words)[mask])
            return out
        if sd is not None:
            return sd.decode(words)
        if pa.types.is_date32(t) or pa.types.is_time32(t):
            return words_to_key(words, np.int32)
        if pa.types.is_temporal(t):
            return words_to_key(words, np.int64)
        return words_to_key(words, t.to_pandas_dtype())

    def to_arrow(self, name, values, mask=None):
        """decode()'s values -> Arrow array of the key's original type (a
        dictionary-encoded key comes back in its value type); rows where
        `mask` is False are NULL."""
        import pyarrow as pa
        t = self.types[name]
        if pa.types.is_dictionary(t):
            t = t.value_type
        if mask is not None:
            nulls = ~np.asarray(mask, dtype=bool)
            if name in self.dicts:
                return pa.array(np.asarray(values, dtype=object), type=t,
                                mask=nulls)
            return pa.array(np.asarray(values), mask=nulls).cast(t)
        if name in self.dicts:
            return pa.array(values, type=t)
        return pa.array(values).cast(t)

    def free(self):
        for sd in self.dicts.values():
            sd.free()
        self.dicts = {}


class GPUAggExecutor(Executor):
    """GPU replacement for SQLAggExecutor (sql_executors.py:556-599).

    Same constructor contract: groupby_keys (list), orderby_keys (list of
    (key, 'asc'|'desc')), sql_statement = the FINAL aggregate clause the
    two-phase rewrite produces (sql_utils.py:379-413) — expressions over
    SUM(partial_col) terms with aliases, e.g.
    "sum(e0_agg_0) as revenue" or "sum(e3_agg_0) / sum(e3_agg_1) as avg_x";
    MIN(col)/MAX(col) partials are supported alongside SUM.

    execute() accumulates partial rows into a device group-by hash table
    (single i64 group key, or multiple keys composite-encoded — DESIGN.md);
    done() extracts groups, evaluates the final expressions host-side over
    the per-group sums (tiny), applies order-by, returns a pyarrow Table.

    device_keys=True lifts the limits of the composite encoding (at most 3
    keys, 2**21 distinct values each): every key column becomes one 64-bit
    word per row (key_to_words; strings by device dictionary code) and the
    word tuples are grouped on the device (ops.GroupByKeys, DESIGN.md
    §3a''): any number of keys, int / bool / date / float / string, up to
    2**31 - 1 groups, key columns returned in their original Arrow types.
    Null keys raise TypeError. The default is the composite path, as before.

    null_keys=True (with device_keys=True) makes NULL a group, one per
    null pattern across the keys, as DuckDB's GROUP BY does: done() returns
    the key columns in their Arrow types with the nulls in place, and an
    order-by over such a key puts its NULLs last in both directions
    (DESIGN.md §3a''').

    null_values=True admits NULLs in the aggregated value columns, with
    DuckDB's rules (DESIGN.md §3a''''): SUM / MIN / MAX skip them, an
    aggregate whose inputs were all NULL is NULL, and an output expression
    is NULL for a group when any aggregate it references is. Such an alias
    comes back as an Arrow float64 column with the nulls in place, and an
    order-by over it puts them last in both directions; an alias without a
    NULL comes back as it does by default. With group keys it needs
    device_keys=True (the hash-table path has no place to remember that a
    group met no value); a grand aggregate (groupby_keys == []) takes it as
    it is. It combines freely with null_keys=True, takes at most 64
    accumulators, and lets one column stand under several functions
    (min(b) beside max(b), one accumulator each), which the default
    refuses. By default a NULL in a value column arrives as NaN
    (an integer column with nulls turns float on the way) and is
    accumulated like any other value: one NULL makes its group's SUM NaN,
    and a MIN / MAX skips it like any NaN. NaN values follow Acero on every
    path: SUM with a NaN is NaN, MIN / MAX skip NaN beside other values,
    and a MIN / MAX whose inputs were all NaN is NaN, not the identity and,
    with null_values=True, not NULL (DESIGN.md §3a'''''')."""

    def __init__(self, groupby_keys, orderby_keys, sql_statement,
                 device_keys=False, null_keys=False, null_values=False):
        if not isinstance(groupby_keys, list):
            raise TypeError("groupby_keys must be a list (may be empty "
                            "for a grand aggregate)")
        if null_keys and not device_keys:
            raise ValueError("null_keys=True needs device_keys=True: the "
                             "composite key encoding has no place for NULL")
        if null_values and groupby_keys and not device_keys:
            raise ValueError("null_values=True with group keys needs "
                             "device_keys=True: the hash-table path keeps "
                             "no record of which aggregates met a value")
        self.groupby_keys = groupby_keys
        self.orderby_keys = orderby_keys or []
        self.sql_statement = sql_statement
        self.device_keys = bool(device_keys)
        self.null_keys = bool(null_keys)
        self.null_values = bool(null_values)
        self.sum_cols = []          # partial columns referenced by aggs
        self.agg_ops = []           # per column: 0 SUM / 1 MIN / 2 MAX
        self.exprs = []             # (alias, python expr over s['col'])
        # name of each accumulator in `s`: its column, or 'fn(col)' for a
        # further function over a column that has one (null_values only)
        self.agg_names = []
        self.expr_cols = []         # per expr: the accumulators it reads
        for part in self._split_top(sql_statement):
            alias = None
            m = re.search(r"\s+as\s+([A-Za-z_][A-Za-z0-9_]*)\s*$", part,
                          re.I)
            if m:
                alias = m.group(1)
                part = part[: m.start()]
            low = part.lower()
            if re.search(r"count\s*\(\s*distinct", low):
                raise ValueError(
                    "count(distinct ...) is not distributive and cannot "
                    "appear in the FINAL aggregate this executor computes; "
                    "the reference's two-phase rewrite (sql_utils.py:299-"
                    "413) does not emit it either — pre-aggregate "
                    "distinct keys upstream (e.g. GPUDistinctExecutor)")
            if re.search(r"\bavg\s*\(", low):
                raise ValueError(
                    "avg(...) must arrive REWRITTEN as sum(partial_sum)/"
                    "sum(partial_count) (the two-phase rewrite, "
                    "sql_utils.py:379-413); avg over partials would be "
                    "wrong: %r" % part)
            hits = _AGG_RE.findall(part)
            if not hits:
                raise ValueError("unsupported aggregate (supported: "
                                 "expressions over SUM/MIN/MAX(col) of "
                                 "partial columns): %r" % part)
            for fn, c in hits:
                if c not in self.sum_cols:
                    self.sum_cols.append(c)
                    self.agg_ops.append(_AGG_OP[fn.lower()])
                    self.agg_names.append(c)
                elif self._agg_name(fn, c) is None:
                    # min(b) beside max(b): DuckDB takes it, and the left
                    # join's NULL payloads ask for both at once; each
                    # function is one more accumulator over the column
                    if not self.null_values:
                        raise ValueError("column %r used with two different "
                                         "aggregate functions" % c)
                    self.sum_cols.append(c)
                    self.agg_ops.append(_AGG_OP[fn.lower()])
                    self.agg_names.append("%s(%s)" % (fn.lower(), c))
            expr = _AGG_RE.sub(
                lambda m: "s[%r]" % self._agg_name(m.group(1), m.group(2)),
                part)
            self.exprs.append((alias or part.strip(), expr))
            self.expr_cols.append(sorted({self._agg_name(fn, c)
                                          for fn, c in hits}))
        if self.null_values and len(self.sum_cols) > 64:
            raise ValueError("null_values=True takes at most 64 aggregated "
                             "columns, got %d" % len(self.sum_cols))
        self._gb = None
        self._key_state = None
        self._key_words = None      # _KeyWords of the device_keys path

    def _agg_name(self, fn, col):
        """Name in `s` of the accumulator of fn(col), None without one."""
        op = _AGG_OP[fn.lower()]
        for name, c, o in zip(self.agg_names, self.sum_cols, self.agg_ops):
            if c == col and o == op:
                return name
        return None

    @staticmethod
    def _split_top(s):
        parts, depth, cur = [], 0, []
        for ch in s:
            if ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
            if ch == "," and depth == 0:
                parts.append("".join(cur))
                cur = []
            else:
                cur.append(ch)
        if cur:
            parts.append("".join(cur))
        return [p.strip() for p in parts if p.strip()]

    def __getstate__(self):
        assert self._gb is None, "executor must be pickled before first execute"
        return dict(self.__dict__)

    def _encode_keys(self, batch):
        """Multiple group keys -> one i64 composite via accumulated host
        codebooks (DESIGN.md §Group keys). Single i64 key passes through."""
        ops, shim, staging = _lazy_gpu()
        if len(self.groupby_keys) > 3:
            raise ValueError(
                "composite group keys: at most 3 keys fit 63 bits at 21 "
                "bits/key (got %d)" % len(self.groupby_keys))
        if self._key_state is None:
            self._key_state = {"dicts": {}, "decode": []}
        arrs = []
        for k in self.groupby_keys:
            col = batch.column(k)
            if _is_stringish(col):
                # device string dictionary: unbounded cardinality, codes
                # consistent across batches (replaces the <=256-entry
                # host StringDict of round 1)
                sd = self._key_state["dicts"].get(k)
                if sd is None:
                    sd = ops.DeviceStringDict(expected=4096)
                    self._key_state["dicts"][k] = sd
                arr = sd.encode_column(col).astype(np.int64)
            else:
                arr = staging.column_to_numpy(col)
            arrs.append(arr)
        if len(arrs) == 1 and arrs[0].dtype == np.int64:
            self._key_state["mode"] = "passthrough"
            self._key_state["pass_dict"] = self._key_state["dicts"].get(
                self.groupby_keys[0])
            if self._key_state["pass_dict"] is None:  # codes are >= 0
                ops.check_no_sentinel_key(arrs[0], type(self).__name__,
                                          self.groupby_keys[0])
            return arrs[0]
        # composite: each non-i64 key coded via np codebook, packed base-N
        self._key_state["mode"] = "composite"
        packed = np.zeros(len(arrs[0]), dtype=np.int64)
        comps = []
        for k, arr in zip(self.groupby_keys, arrs):
            cb = self._key_state.setdefault("codebooks", {}).setdefault(k, {})
            vals, inv = np.unique(arr, return_inverse=True)
            codes = np.empty(len(vals), dtype=np.int64)
            for i, v in enumerate(vals):
                key = v.item() if hasattr(v, "item") else v
                if key not in cb:
                    if len(cb) >= (1 << 21):
                        raise ValueError(
                            "composite group key %r exceeds 2**21 distinct "
                            "values; exceeding the 21-bit field would "
                            "silently merge distinct groups" % k)
                    cb[key] = len(cb)
                codes[i] = cb[key]
            comps.append(codes[inv])
        for c in comps:
            packed = packed * (1 << 21) + c  # 21 bits per key, <= 3 keys
        self._key_state["ncomps"] = len(comps)
        return packed

    def _decode_keys(self, packed):
        ncomps = self._key_state.get("ncomps", 1)
        outs = []
        rem = packed.astype(np.int64)
        for _ in range(ncomps):
            outs.append(rem % (1 << 21))
            rem = rem // (1 << 21)
        outs.reverse()
        cols = {}
        for k, codes in zip(self.groupby_keys, outs):
            cb = self._key_state["codebooks"][k]
            inv = {v: kk for kk, v in cb.items()}
            vals = [inv[c] for c in codes.astype(np.int64)]
            # string columns were StringDict-coded before the codebook:
            # unwind that layer too so callers get the original strings
            sd = self._key_state["dicts"].get(k)
            if sd is not None and sd.values:
                vals = [sd.values[v] for v in vals]
            cols[k] = np.array(vals)
        return cols

    def _stage_values(self, batch):
        """-> (f64 DevColumns of the aggregated columns, per column a host
        bool mask or None). With null_values=True a column that has nulls
        is split first (staging.split_nulls), so an int64 column stays
        exact up to the cast to f64 and what Arrow holds under a null
        never reaches the device; masks is None otherwise."""
        _, shim, staging = _lazy_gpu()
        staged = {}                 # min(b) and max(b) share one upload
        for c in self.sum_cols:
            if c in staged:
                continue
            col, mask = batch.column(c), None
            if self.null_values and col.null_count:
                col, mask = staging.split_nulls(col)
            staged[c] = (shim.DevColumn.from_numpy(
                staging.column_to_numpy(col).astype(np.float64)), mask)
        vcols = [staged[c][0] for c in self.sum_cols]
        masks = [staged[c][1] for c in self.sum_cols]
        return vcols, (masks if self.null_values else None)

    def _execute_grand_nullable(self, batch):
        """null_values=True without keys: the dense accumulate over an
        all-zero code column, one record and one seen word."""
        ops, shim, _ = _lazy_gpu()
        if self._gb is None:
            self._gb = ops.DenseAcc(len(self.sum_cols), self.agg_ops,
                                    capacity=1, nullable_vals=True,
                                    who=type(self).__name__)
        n = len(batch)
        codes = shim.DevColumn(np.uint32, n)
        shim.call("qk_dmemset", codes.ptr, 0, shim.c_u64(n * 4))
        vcols, masks = self._stage_values(batch)
        try:
            self._gb.accumulate(codes, 1, vcols, n, masks)
        finally:
            for c in [codes] + list({id(v): v for v in vcols}.values()):
                c.free()

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        ops, shim, staging = _lazy_gpu()
        batches = [b for b in batches if b is not None and len(b) > 0]
        if not batches:
            return
        batch = pa.concat_tables(batches)
        if self.device_keys and self.groupby_keys:
            return self._execute_device_keys(batch)
        if self.null_values:        # no keys: refused with keys in __init__
            return self._execute_grand_nullable(batch)
        if self.groupby_keys:
            keys = self._encode_keys(batch)
        else:
            keys = np.zeros(len(batch), dtype=np.int64)
        if self._gb is None:
            self._gb = ops.GroupByI64(
                expected_groups=max(1024, len(batch)),
                nvals=len(self.sum_cols), agg_ops=self.agg_ops)
        kcol = shim.DevColumn.from_numpy(keys)
        vcols = [shim.DevColumn.from_numpy(
            staging.column_to_numpy(batch.column(c)).astype(np.float64))
            for c in self.sum_cols]
        self._gb.update(kcol, vcols)
        kcol.free()
        for v in vcols:
            v.free()

    def _execute_device_keys(self, batch):
        """device_keys=True: every key column becomes one 64-bit word per
        row, the tuple of words one dense code (ops.GroupByKeys). Any
        number of keys, any cardinality up to 2**31 - 1 groups."""
        ops, shim, staging = _lazy_gpu()
        if self._key_words is None:
            self._key_words = _KeyWords(self.groupby_keys, self.null_keys)
        self._key_words.check(batch, type(self).__name__)
        words, masks = self._key_words.words(batch, ops), None
        if self.null_keys:
            words, masks = words
        if self._gb is None:
            self._gb = ops.GroupByKeys(
                len(self.groupby_keys), len(self.sum_cols),
                agg_ops=self.agg_ops,
                expected_groups=max(1024, len(batch)),
                nullable_keys=self.null_keys,
                **({"nullable_vals": True} if self.null_values else {}))
        kcols = [shim.DevColumn.from_numpy(w) for w in words]
        vcols, vmasks = self._stage_values(batch)
        try:
            if self.null_values:
                self._gb.update(kcols, vcols, len(batch), key_valid=masks,
                                val_valid=vmasks)
            else:
                self._gb.update(kcols, vcols, len(batch), key_valid=masks)
        finally:
            for c in kcols + list({id(v): v for v in vcols}.values()):
                c.free()

    def _done_device_keys(self):
        key_words, sums = self._gb.extract()
        s = {c: sums[i] for i, c in enumerate(self.agg_names)}
        kw = self._key_words
        masks = {}
        if self.null_keys:
            masks = dict(zip(self.groupby_keys, self._gb.extract_valid()))
        out = {k: kw.decode(k, w, masks.get(k))
               for k, w in zip(self.groupby_keys, key_words)}
        vals_valid = None
        if self.null_values:
            vals_valid = dict(zip(self.agg_names,
                                  self._gb.extract_vals_valid()))
        out, masks = self._final_columns(out, s, vals_valid, masks)
        for k in self.groupby_keys:
            out[k] = kw.to_arrow(k, out[k], masks.get(k))
        self._gb.free()
        self._gb = None
        kw.free()
        self._key_words = None
        return _to_table(out)

    def _final_columns(self, out, s, vals_valid=None, masks=None):
        """The host end of done(), no device in it: evaluates the output
        expressions over the per-group aggregates s (column -> array [G]),
        adds them to the key columns in `out`, and applies the order-by.
        -> (columns, masks), both in output order.

        vals_valid (null_values=True): column -> bool array [G], False
        where that aggregate of the group is NULL. An expression is NULL
        where any aggregate it references is; identities stand under
        those slots, so it is evaluated with the floating-point warnings
        off. An alias that has a NULL joins `masks`, which puts its NULLs
        last in the order-by, and comes back as an Arrow float64 array
        with the nulls in place; every other alias comes back as the
        numpy array it has always been."""
        import contextlib
        masks = dict(masks or {})
        quiet = np.errstate(all="ignore") if vals_valid is not None \
            else contextlib.nullcontext()
        nullable = []
        with quiet:
            for (alias, expr), refs in zip(self.exprs, self.expr_cols):
                v = eval(expr, {"s": s})  # noqa: S307 — expr built above
                if vals_valid is not None:
                    ok = np.logical_and.reduce([vals_valid[c] for c in refs])
                    if not ok.all():
                        # NULL rows tie in the order-by whatever stood there
                        v = np.where(ok, v, 0.0)
                        masks[alias] = ok
                        nullable.append(alias)
                out[alias] = v
        # bool keys order as 0/1 (numpy refuses to negate a bool array)
        order = self._order_by({k: (v.astype(np.uint8)
                                    if getattr(v, "dtype", None) == np.bool_
                                    else v) for k, v in out.items()},
                               masks)
        if order is not None:
            out = {k: np.asarray(v)[order] for k, v in out.items()}
            masks = {k: m[order] for k, m in masks.items()}
        if nullable:
            import pyarrow as pa
            for alias in nullable:
                out[alias] = pa.array(
                    np.asarray(out[alias], dtype=np.float64),
                    type=pa.float64(), mask=~masks[alias])
        return out, masks

    def _order_by(self, out, masks=None):
        """Row order of the order-by clause over the output columns, or
        None without one. masks: column -> bool array (True = valid), the
        keys of the null_keys path and the aliases of the null_values
        path that hold a NULL; the NULLs of such a column sort last,
        ascending and descending alike."""
        if not self.orderby_keys:
            return None
        cols = []
        for item in reversed(self.orderby_keys):
            k, d = item if isinstance(item, (tuple, list)) else (item, "asc")
            v = np.asarray(out[k])
            if d == "desc":
                if v.dtype.kind in "biuf":
                    v = -v
                else:
                    # non-numeric desc (e.g. decoded string group keys):
                    # invert factorized rank instead of numeric negation
                    _, inv = np.unique(v, return_inverse=True)
                    v = inv.max() - inv
            cols.append(v)
            if masks and k in masks:
                # more significant than the key's own value, less than
                # the order-by keys before it
                cols.append(~masks[k])
        return np.lexsort(cols)

    def done(self, executor_id):
        if self._gb is None:
            return None
        if self.device_keys and self.groupby_keys:
            return self._done_device_keys()
        if self.null_values:
            sums, valid = self._gb.extract(1), self._gb.extract_valid(1)
            out, _ = self._final_columns(
                {}, {c: sums[i] for i, c in enumerate(self.agg_names)},
                dict(zip(self.agg_names, valid)))
            self._gb.free()
            self._gb = None
            return _to_table(out)
        keys, sums = self._gb.extract()
        s = {c: sums[i] for i, c in enumerate(self.sum_cols)}
        out = {}
        if self.groupby_keys:
            if self._key_state and self._key_state.get("mode") == "composite":
                out.update(self._decode_keys(keys))
            else:
                sd = (self._key_state or {}).get("pass_dict")
                out[self.groupby_keys[0]] = (sd.decode(keys) if sd
                                             else keys)
        for alias, expr in self.exprs:
            out[alias] = eval(expr, {"s": s})  # noqa: S307 — expr built above
        order = self._order_by(out)
        if order is not None:
            out = {k: np.asarray(v)[order] for k, v in out.items()}
        self._gb.free()
        self._gb = None
        return _to_table(out)


class GPUCountExecutor(Executor):
    """= CountExecutor (sql_executors.py:69-86): running row count,
    done() returns a one-row table."""

    def __init__(self):
        self.state = 0

    def execute(self, batches, stream_id, executor_id):
        self.state += sum(len(b) for b in batches
                          if b is not None)

    def done(self, executor_id):
        import pyarrow as pa
        return pa.table({"count": np.array([self.state], dtype=np.int64)})


class GPUBroadcastJoinExecutor(GPUBuildProbeJoinExecutor):
    """= BroadcastJoinExecutor (sql_executors.py:275-319): the small build
    side is given at CONSTRUCTION (broadcast to every channel) instead of
    arriving as stream 1; every execute() batch is a probe. Same device
    hash-table machinery as GPUBuildProbeJoinExecutor; picklable because
    the table is built lazily from the stored host columns."""

    def __init__(self, small_table, on=None, small_on=None, big_on=None,
                 suffix="_small", how="inner", null_keys=False,
                 null_payloads=False):
        if on is not None:
            assert small_on is None and big_on is None
            small_on = big_on = on
        super().__init__(left_on=big_on, right_on=small_on, how=how,
                         null_keys=null_keys, null_payloads=null_payloads)
        self.suffix = suffix
        import pyarrow as pa
        if not isinstance(small_table, pa.Table):
            small_table = pa.table(small_table)
        self._small_table = None
        if self.null_payloads:
            # kept as Arrow and staged like one build batch at first
            # execute, so payload nulls and types survive
            assert self.right_on in small_table.column_names
            self._small_table = small_table
            return
        self._small_host = {c: small_table.column(c).to_numpy(
            zero_copy_only=False) for c in small_table.column_names}
        assert self.right_on in self._small_host
        self._small_key_mask = None
        key = small_table.column(self.right_on)
        if self.null_keys and key.null_count and not _is_stringish(key):
            # a numeric key keeps its mask beside 0-filled values (a null
            # string key stays None in the object array and is masked
            # when _finish_build encodes it)
            from . import staging
            filled, self._small_key_mask = staging.split_nulls(key)
            self._small_host[self.right_on] = staging.column_to_numpy(filled)

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        batches = [b for b in batches if b is not None and len(b) > 0]
        if not batches:
            return
        if self._table is None and self._small_table is not None:
            self._stage_build_batch(self._small_table)
            self._finish_build()
        elif self._table is None:
            self._build_names = list(self._small_host.keys())
            self._build_cols = {c: [np.asarray(v)]
                                for c, v in self._small_host.items()}
            if self._small_key_mask is not None:
                self._build_key_masks = [self._small_key_mask]
            self._finish_build()
        self.phase = "probe"
        return self._probe(pa.concat_tables(batches))


class GPUDiskBuildProbeJoinExecutor(Executor):
    """GPU mirror of DiskBuildProbeJoinExecutor (sql_executors.py:456-514):
    build batches SPILL to Parquet chunks in `spill_dir` instead of
    accumulating in memory, and each probe batch joins against every
    spilled chunk with at most ONE chunk's hash table resident in HBM at
    a time — the out-of-HBM build-side path. The chunks round-trip
    through our own GPU Parquet decode (parquet_gpu), so the read-back
    is device-side like everything else.

    Same constructor signature as the reference (+ its spill_dir). Like
    the reference's per-chunk join-then-concat plan (its :505-507
    polars.concat of per-chunk lazy joins), the semantics are exact for
    INNER joins; other `how` values are refused with a typed error (the
    reference's concat silently duplicates unmatched rows for them).
    Integer keys, numeric payload columns (the spill subset)."""

    def __init__(self, on=None, left_on=None, right_on=None, how="inner",
                 key_to_keep="left", spill_dir=None):
        import secrets
        if on is not None:
            self.left_on = self.right_on = on
        else:
            if left_on is None or right_on is None:
                raise ValueError("join needs on= or both left_on= and "
                                 "right_on=")
            self.left_on, self.right_on = left_on, right_on
        if how != "inner":
            raise ValueError(
                "spill join supports how='inner' only: per-chunk "
                "join-then-concat is incorrect for left/semi/anti (the "
                "reference's DiskBuildProbeJoinExecutor concat has the "
                "same flaw); use GPUBuildProbeJoinExecutor for those")
        self.how = how
        self.key_to_keep = key_to_keep
        self.spill_dir = spill_dir or "/tmp"
        self.prefix = secrets.token_hex(6)
        self.count = 0
        self.phase = "build"

    def _path(self, executor_id, i):
        import os
        return os.path.join(self.spill_dir, "build_%s_%s_%d.parquet"
                            % (self.prefix, executor_id, i))

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        import pyarrow.parquet as pq
        batches = [b for b in batches if b is not None and len(b) > 0]
        if not batches:
            return
        batch = pa.concat_tables(batches)
        if stream_id == 1:                       # build: spill the chunk
            assert self.phase == "build"
            import pyarrow.types as pat
            bcol = batch.column(self.right_on)
            if pat.is_integer(bcol.type):
                from . import ops
                ops.check_no_sentinel_key(
                    bcol.to_numpy().astype(np.int64),
                    type(self).__name__, self.right_on)
            t = batch.cast(pa.schema([pa.field(f.name, f.type,
                                               nullable=False)
                                      for f in batch.schema]))
            pq.write_table(t, self._path(executor_id, self.count),
                           compression="NONE", data_page_version="1.0",
                           use_dictionary=False)
            self.count += 1
            return
        # probe
        if self.count == 0:
            return
        self.phase = "probe"
        ops, shim, staging = _lazy_gpu()
        from . import parquet_gpu, bridge
        probe_keys = staging.column_to_numpy(batch.column(self.left_on))
        if probe_keys.dtype.kind not in "iu":
            raise TypeError("spill join requires integer keys")
        kcol = shim.DevColumn.from_numpy(probe_keys.astype(np.int64))
        probe_dev = {c: shim.DevColumn.from_numpy(
            staging.column_to_numpy(batch.column(c)))
            for c in batch.column_names}
        outs = []
        for i in range(self.count):
            cols = parquet_gpu.read_table(self._path(executor_id, i))
            bkeys = cols[self.right_on]
            if bkeys.dtype != np.dtype(np.int64):
                tmp = bkeys.to_numpy(bkeys.n).astype(np.int64)
                bkeys.free()
                bkeys = shim.DevColumn.from_numpy(tmp)
                cols[self.right_on] = bkeys
            table = ops.JoinTable(max(16, bkeys.n))
            table.build(bkeys)
            pidx, bidx, nm = table.probe(kcol)
            if nm:
                out = {}
                for c, dev in probe_dev.items():
                    g = dev.gather(pidx, nm)
                    out[c] = bridge.to_pinned_numpy(g, nm)
                    g.free()
                for c, dev in cols.items():
                    if c == self.right_on:
                        continue
                    g = dev.gather(bidx, nm)
                    out[c] = bridge.to_pinned_numpy(g, nm)
                    g.free()
                if self.key_to_keep == "right" and \
                        self.left_on != self.right_on:
                    out[self.right_on] = out.pop(self.left_on)
                outs.append(_to_table(out))
            pidx.free()
            if bidx:
                bidx.free()
            table.free()
            for dev in cols.values():
                (dev[0] if isinstance(dev, tuple) else dev).free()
        kcol.free()
        for dev in probe_dev.values():
            dev.free()
        if not outs:
            return None
        import pyarrow as pa
        return pa.concat_tables(outs)

    def done(self, executor_id):
        import os
        for i in range(self.count):
            try:
                os.unlink(self._path(executor_id, i))
            except OSError:
                pass
        return None


class GPUDistinctExecutor(Executor):
    """= DistinctExecutor (sql_executors.py:517-554): per batch, emit the
    rows whose key was never seen before (batch.unique() then anti-join
    against the accumulated state, :529-543). Device hash table keyed i64;
    done() returns None like the reference (state already emitted).

    `keys` as a str or a one-element list is that single-column path. A
    list of two or more columns is the reference's unique(subset=keys)
    over all of them, through ops.DeviceKeyDict (DESIGN.md §3a'').

    null_keys=True admits NULL keys, which equal each other as in polars'
    unique: every form, the single key included, then goes through a
    nullable DeviceKeyDict (DESIGN.md §3a''')."""

    def __init__(self, keys, null_keys=False):
        self.null_keys = bool(null_keys)
        if self.null_keys and isinstance(keys, str):
            keys = [keys]
        self._multi = not isinstance(keys, str) and \
            (len(keys) >= 2 or (self.null_keys and len(keys) == 1))
        if self._multi:
            # unique(subset=keys) over two or more columns: every row's
            # key tuple -> one dense code (ops.DeviceKeyDict)
            self.keys = list(keys)
            if not all(isinstance(k, str) for k in self.keys):
                raise TypeError("distinct key column names expected")
        else:
            self.keys = keys if isinstance(keys, str) else keys[0]
            if not isinstance(self.keys, str):
                raise TypeError("single distinct key column expected")
        self._table = None
        self._n_rows = 0
        self._key_dict = None       # DeviceStringDict for string keys
        self._kd = None             # DeviceKeyDict of the multi-key path
        self._key_words = None

    def __getstate__(self):
        assert self._table is None and self._kd is None, \
            "pickle before first execute"
        return dict(self.__dict__)

    def _execute_multi(self, batch):
        """Emit the rows whose key tuple no earlier batch held and that
        are the first of this batch with it: code >= the code count before
        the batch, first occurrence of that code."""
        ops, shim, staging = _lazy_gpu()
        if self._key_words is None:
            self._key_words = _KeyWords(self.keys, self.null_keys)
        self._key_words.check(batch, type(self).__name__)
        words, masks = self._key_words.words(batch, ops), None
        if self.null_keys:
            words, masks = words
        if self._kd is None:
            self._kd = ops.DeviceKeyDict(len(self.keys),
                                         expected=max(1024, len(batch)),
                                         nullable=self.null_keys)
        before = self._kd.n_codes
        kcols = [shim.DevColumn.from_numpy(w) for w in words]
        try:
            dcodes = self._kd.encode(kcols, len(batch), valid=masks)
        finally:
            for c in kcols:
                c.free()
        codes = dcodes.to_numpy(len(batch))
        dcodes.free()
        ucodes, first_idx = np.unique(codes, return_index=True)
        sel = np.sort(first_idx[ucodes >= before])
        return batch.take(sel) if len(sel) else None

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        ops, shim, staging = _lazy_gpu()
        batches = [b for b in batches if b is not None and len(b) > 0]
        if not batches:
            return
        batch = pa.concat_tables(batches)
        if self._multi:
            return self._execute_multi(batch)
        key_col = batch.column(self.keys)
        if _is_stringish(key_col):
            # device string dictionary -> dense codes (consistent across
            # batches), distinct-on-codes == distinct-on-strings
            if self._key_dict is None:
                self._key_dict = ops.DeviceStringDict(
                    expected=max(1024, len(batch)))
            keys = self._key_dict.encode_column(key_col).astype(np.int64)
        else:
            keys = staging.column_to_numpy(key_col)
        if keys.dtype != np.int64:
            if keys.dtype.kind in "iu":
                keys = keys.astype(np.int64)
            else:
                raise TypeError("GPUDistinctExecutor requires integer or "
                                "string keys, got %s" % keys.dtype)
        if self._key_dict is None:      # dictionary codes are >= 0
            ops.check_no_sentinel_key(keys, type(self).__name__, self.keys)
        # within-batch unique (first occurrence), as batch.unique() does
        _, first_idx = np.unique(keys, return_index=True)
        first_idx.sort()
        batch = batch.take(first_idx)
        keys = keys[first_idx]
        if self._table is None:
            self._table = ops.JoinTable(max(1 << 16, 4 * len(keys)))
            self._seen = []
        if self._n_rows + len(keys) > min(self._table.chain_cap,
                                          self._table.cap // 2):
            self._grow(len(keys))
        kcol = shim.DevColumn.from_numpy(keys)
        pidx, _, nm = self._table.probe(kcol, mode=2)   # anti: unseen rows
        sel = np.sort(pidx.to_numpy(nm))
        contribution = batch.take(sel)
        new_keys = keys[sel]
        if len(new_keys):
            ncol = shim.DevColumn.from_numpy(new_keys)
            self._table.build(ncol)
            ncol.free()
            self._seen.append(new_keys)
            self._n_rows += len(new_keys)
        kcol.free()
        pidx.free()
        return contribution if len(contribution) else None

    def _grow(self, incoming):
        """Rebuild a larger table from the accumulated distinct keys
        (the reference's vstack state just grows, :542)."""
        ops, shim, staging = _lazy_gpu()
        self._table.free()
        allk = np.concatenate(self._seen) if self._seen else             np.empty(0, np.int64)
        self._table = ops.JoinTable(max(1 << 16,
                                        4 * (self._n_rows + incoming)))
        if len(allk):
            kcol = shim.DevColumn.from_numpy(allk)
            self._table.build(kcol)
            kcol.free()

    def done(self, executor_id):
        return None


class GPUSortExecutor(Executor):
    """Mirror of SuperFastSortExecutor (sql_executors.py:88-187): the
    operator that makes its output stream SORTED by `key`. The reference
    implements it as a disk-backed external merge sort (spill files +
    k-way merge) because its build ran on 64 GB hosts; with 288 GB of HBM
    the state fits device memory, so this mirror accumulates batches and
    done() returns the fully sorted table via the device radix sort
    (stable, ascending — the reference's output contract)."""

    def __init__(self, key, record_batch_rows=None, output_batch_rows=None,
                 file_prefix=None):
        # extra args accepted for signature compatibility (:89); the
        # spill tuning knobs have no meaning on the device path
        self.key = key
        self._batches = None

    def __getstate__(self):
        assert self._batches is None, "pickle before first execute"
        return dict(self.__dict__)

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        batches = [b for b in batches if b is not None and len(b) > 0]
        if not batches:
            return
        b = pa.concat_tables(batches)
        self._batches = b if self._batches is None             else pa.concat_tables([self._batches, b])
        return None

    def done(self, executor_id):
        if self._batches is None:
            return None
        ops, shim, staging = _lazy_gpu()
        t = self._batches
        key_col = t.column(self.key)
        if _is_stringish(key_col):
            # lexicographic string sort: dictionary codes are
            # arrival-ordered, so remap code -> lexicographic rank of
            # its value (host sorts the DISTINCT values only), then the
            # stable device radix sort runs on the ranks
            sd = ops.DeviceStringDict(expected=max(1024, t.num_rows))
            codes = sd.encode_column(key_col)
            vals = sd.values
            rank_of = np.empty(len(vals), dtype=np.int64)
            rank_of[np.argsort(np.asarray(vals, dtype=object))] = \
                np.arange(len(vals))
            keys = rank_of[codes]
            sd.free()
        else:
            keys = staging.column_to_numpy(key_col)
        kcol = shim.DevColumn.from_numpy(keys)
        perm = ops.sort_permutation(kcol)
        order = perm.to_numpy(perm.n)
        kcol.free()
        perm.free()
        return t.take(order)


class GPUTopKExecutor(Executor):
    """Mirror of ConcatThenSQLExecutor as lowered by DataStream.top_k
    (sql_executors.py:45-67; datastream.py:1746-1767): concatenate incoming
    batches, done() returns the top-k rows by `sort_keys`/`descending`.

    Like the reference (one DuckDB 'order by ... limit k' over the
    concatenated partials in done()), the final selection runs host-side —
    the inputs at this operator are the already-aggregated partials, tiny
    relative to the scan the GPU kernels consumed."""

    def __init__(self, sort_keys, k, descending=None):
        assert isinstance(sort_keys, list) and len(sort_keys) >= 1
        self.sort_keys = sort_keys
        self.k = int(k)
        self.descending = descending or [False] * len(sort_keys)
        self.state = None

    def execute(self, batches, stream_id, executor_id):
        import pyarrow as pa
        batches = [b for b in batches if b is not None and len(b) > 0]
        if not batches:
            return
        batch = pa.concat_tables(batches)
        self.state = batch if self.state is None \
            else pa.concat_tables([self.state, batch])
        return None

    def done(self, executor_id):
        if self.state is None:
            return None
        cols = []
        for key, desc in zip(reversed(self.sort_keys),
                             reversed(self.descending)):
            col = self.state.column(key)
            v = np.asarray(col.to_numpy(zero_copy_only=False))
            if desc:
                # descending = ascending on the reversed rank of the
                # distinct values: no arithmetic on the key itself, so
                # strings, unsigned and INT64_MIN keys order like any
                # other. NaN stays last, as it is ascending.
                _, inv = np.unique(v, return_inverse=True)
                inv = inv.reshape(-1)
                rank = inv.max() - inv
                if v.dtype.kind == "f":
                    rank[np.isnan(v)] = len(v)
                v = rank
            cols.append(v)
            if col.null_count and v.dtype.kind in "fiu":
                # a float NULL arrives as NaN: it sorts after the NaN
                # values in both directions (Acero's nulls-at-end order)
                cols.append(np.asarray(col.is_null().to_numpy(
                    zero_copy_only=False)))
        order = np.lexsort(cols)[: self.k]
        return self.state.take(order)


def gpu_partition_fn(data, source_channel, num_target_channels, key=None,
                     predicate=None, string_dicts=None, projection=None,
                     batch_agg=None, partitioner="hash", total_range=None,
                     transforms=None):
    """GPU partition function mirroring the reference's full partition_fn
    (core.py:152-195): optional PREDICATE (filter_sql grammar, JIT-fused
    on device via quokka_amd.jit) -> optional map-side PARTIAL AGGREGATE
    (`batch_agg`, the reference's folded batch_funcs, core.py:173-176 +
    df.py:1354-1394) -> hash partition (int key -> key % N, bit-exact
    with quokka_runtime.py:222) -> optional column projection (sorted
    order, core.py:191-193).

    A predicate may name a free-text string column (one with no entry in
    `string_dicts`) in `col LIKE 'pat'`, NOT LIKE, = 'lit', <> 'lit' and
    != 'lit' — the reference's filter_sql("o_comment not like
    '%special%requests%'") (apps/tpc-h/tpch.py:380) as written. Such a
    column is staged from its Arrow offsets + bytes buffers
    (ops.StringColumn) and matched per row on the device (ops.like); the
    flags feed the JIT predicate like any other input, on the plain and
    the batch_agg path alike. String columns the predicate does not name
    never reach the device.

    batch_agg = (group_keys, aggs) with group_keys a list of
    (u8_code_column, cardinality) and aggs the two-phase PARTIAL forms
    ('SUM(expr) as x' / 'COUNT(*) as n', sql_utils.py:299-413). The
    predicate and the aggregate run as ONE fused device pass
    (jit.JitAggregate — the Q1-shaped kernel), and what gets partitioned
    (by group id % N) is the tiny partial table, not rows: the map-side
    fusion that shrinks shuffle bytes from O(rows) to O(groups).
    transforms: list of (out_name, arith_expr) applied per batch AFTER
    the predicate (the reference's folded transform_sql maps inside
    batch_funcs, core.py:173-176 + datastream.py:652-815): each
    expression JIT-compiles to a device elementwise kernel (quokka_amd
    .jit.JitMap, f64 out) and the result column joins the partition +
    projection like any input column.
    Row ORDER within a partition is unspecified (the device scatter
    assigns block-chunk ranges; the reference's polars partition_by is
    input-ordered) — every consumer on this path is order-insensitive
    (joins/aggregates; sorts order explicitly).
    partitioner: "hash" (key % N, quokka_runtime.py:222), "range"
    (id = (key-1) // (total_range // N), quokka_runtime.py:234-243 —
    keys outside [1, total_range] are CLAMPED to the edge channels where
    the reference would misroute them; same key -> same channel either
    way), or "broadcast" (every channel gets the full table,
    quokka_runtime.py:245-246).
    `data`: pyarrow Table; returns dict target_channel -> pyarrow Table."""
    import pyarrow as pa
    ops, shim, staging = _lazy_gpu()
    if partitioner == "broadcast":
        return {i: data for i in range(num_target_channels)}
    assert partitioner in ("hash", "range"), partitioner
    def _col(c):
        try:
            return staging.column_to_numpy(data.column(c),
                                           (string_dicts or {}).get(c))
        except TypeError:
            col = data.column(c)
            if _is_stringish(col):       # general strings: host object
                if c == key:             # hashed from its Arrow buffers
                    return _ArrowStrings(col)
                return np.asarray(col.to_pylist(), dtype=object)
            raise

    host_cols = {c: _col(c) for c in data.column_names}

    def _jit_schema(dcols):
        """Device columns + every raw string column (object marker)."""
        schema = {c: v.dtype for c, v in dcols.items()}
        for c, v in host_cols.items():
            if v.dtype == object and _is_stringish(data.column(c)):
                schema[c] = np.dtype(object)
        return schema

    def _stage_raw_strings(prog, dcols):
        """Upload the raw string columns `prog`'s predicate names."""
        for c in sorted({t[1] for t in prog.str_terms}):
            dcols[c] = ops.StringColumn.from_arrow(data.column(c))

    if batch_agg is not None:
        if transforms:
            raise ValueError("batch_agg already aggregates arbitrary "
                             "arithmetic expressions; transforms cannot "
                             "be combined with it")
        from . import jit
        group_keys, aggs = batch_agg
        # COUNT(*) identifies which groups were actually observed (the
        # reference's partial tables contain only observed groups);
        # append one internally if the caller didn't ask for it
        have_count = any(a.lower().replace(" ", "").startswith("count(")
                         for a in aggs)
        run_aggs = list(aggs) + ([] if have_count
                                 else ["COUNT(*) as __qk_presence"])
        dcols = {c: shim.DevColumn.from_numpy(v)
                 for c, v in host_cols.items() if v.dtype != object}
        agg = jit.JitAggregate(_jit_schema(dcols), group_keys, run_aggs,
                               predicate, string_dicts)
        _stage_raw_strings(agg, dcols)
        acc = agg.make_acc()
        agg.run(dcols, acc)
        partials = agg.read(acc)               # (ngroups, naggs)
        acc.free()
        agg.free()
        for c in dcols.values():
            c.free()
        gid = np.arange(partials.shape[0])
        count_col = (len(aggs) if not have_count else
                     next(i for i, a in enumerate(aggs)
                          if a.lower().replace(" ", "")
                          .startswith("count(")))
        observed = partials[:, count_col] > 0
        cols_out = {}
        rem = gid
        for name, card in reversed(list(group_keys)):
            cols_out[name] = (rem % card).astype(np.uint8)
            rem = rem // card
        for j, aname in enumerate(agg.agg_names):
            if aname != "__qk_presence":
                cols_out[aname] = partials[:, j]
        parts = gid % num_target_channels      # group id is the int key
        out = {}
        for p in range(num_target_channels):
            m = (parts == p) & observed
            if m.any():
                out[p] = pa.table({c: v[m] for c, v in cols_out.items()})
        return out

    if predicate is not None:
        from . import jit
        dcols = {c: shim.DevColumn.from_numpy(v)
                 for c, v in host_cols.items() if v.dtype != object}
        f = jit.JitFilter(predicate, _jit_schema(dcols), string_dicts)
        _stage_raw_strings(f, dcols)
        fidx, k = f.run(dcols)
        sel0 = fidx.to_numpy(k)
        host_cols = {c: v[sel0] for c, v in host_cols.items()}
        f.free()
        fidx.free()
        for c in dcols.values():
            c.free()

    if transforms:
        from . import jit
        dcols = {c: shim.DevColumn.from_numpy(v)
                 for c, v in host_cols.items() if v.dtype != object}
        schema = {c: v.dtype for c, v in dcols.items()}
        for out_name, expr in transforms:
            m = jit.JitMap(expr, schema)
            o = m.run(dcols)
            host_cols[out_name] = o.to_numpy(o.n)
            o.free()
            m.free()
        for c in dcols.values():
            c.free()

    keys = host_cols[key]
    if isinstance(keys, _ArrowStrings):
        # string partition keys: a row's channel is (byte hash >> 1) % N,
        # a pure function of the key's bytes, so a key
        # meets its equals on one channel whichever batch, producer or
        # rank sent it. (The reference hashes strings inside polars,
        # quokka_runtime.py:224; its bucket ids are an implementation
        # detail, the contract is equal keys -> same channel. Range
        # partitioning needs an ordered key.)
        if partitioner != "hash":
            raise TypeError("string keys support hash partitioning only")
        kcol = ops.str_hash_i64(keys.arr)
        host_cols[key] = keys.arr
    else:
        if keys.dtype != np.int64:
            if keys.dtype.kind in "iu":
                keys = keys.astype(np.int64)
            else:
                raise TypeError("gpu_partition_fn: integer or string keys, "
                                "got %s" % keys.dtype)
        kcol = shim.DevColumn.from_numpy(keys)
    if partitioner == "range":
        assert total_range, "range partitioner needs total_range"
        from .shim import DevColumn, c_u64, c_i64, c_u32
        per = max(1, int(total_range) // num_target_channels)
        ids = DevColumn(np.int64, max(1, len(keys)))
        shim.call("qk_range_part_ids", None, c_u64(len(keys)), kcol.ptr,
                  c_i64(per), c_u32(num_target_channels), ids.ptr)
        kcol.free()
        kcol = ids
    offsets, idx = ops.partition_i64(kcol, num_target_channels)
    sel = idx.to_numpy(len(keys))
    names = sorted(projection) if projection else sorted(host_cols)
    out = {}
    for p in range(num_target_channels):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        if hi == lo:
            continue
        rows = sel[lo:hi]
        # ndarray.take for the host columns, Array.take for a string key
        out[p] = pa.table({c: host_cols[c].take(rows) for c in names})
    kcol.free()
    idx.free()
    return out
