"""GPU Parquet column decode for MI355X.

The reference's scan path decodes Parquet on the CPU with pyarrow
(pyquokka/dataset.py InputParquetDataset.get_next_batch and the
row-group fetch in InputS3FilesDataset) and hands host Arrow batches to
the executors. Here the division of labor is MI355X-first: the host
touches only METADATA — the footer (via pyarrow), each page's Thrift
header (parquet_thrift.py), definition-level runs and the RLE run
descriptors (a few bytes per ~1 MB page) — while the raw file bytes go
to HBM ONCE and the qk_pq_* kernels expand every value there.

Supported (the TPC-H hot-path column shapes):
- UNCOMPRESSED column chunks, data page v1 or v2
- PLAIN fixed-width (INT32/INT64/FLOAT/DOUBLE) pages
- RLE_DICTIONARY pages for fixed-width types (indices expanded on GPU,
  dictionary gathered on GPU)
- RLE_DICTIONARY BYTE_ARRAY columns -> (u32 code column in HBM, host
  value list), the string-dictionary form the executors already use
- flat nullable columns: with read_table's default nulls="raise" only
  columns with NO nulls present decode (definition levels are verified
  from the run descriptors) and actual nulls raise; nulls="mask" decodes
  them into an ops.NullableColumn (values + validity bitmap, both
  expanded on the GPU: qk_pq_def_pages, qk_valid_expand)

Anything else raises QkParquetError — loudly, no CPU value fallback.
"""
import numpy as np

from . import parquet_thrift as T
from .parquet_thrift import _varint

ENC_PLAIN = 0
ENC_RLE = 3
ENC_RLE_DICT = 8
ENC_PLAIN_DICT = 2

_PHYS = {"INT32": np.dtype(np.int32), "INT64": np.dtype(np.int64),
         "FLOAT": np.dtype(np.float32), "DOUBLE": np.dtype(np.float64)}

_TILE = 1 << 13          # values per PLAIN tile / max RLE entry length
# (8K values -> ~2900 workgroups per 24M-value column: tiles map 1:1 to
# workgroups, and the 256-CU chip needs >>256 of them; 64K tiles ran the
# decode at 4.9 GB/s, 8K at TB/s-class)


class QkParquetError(RuntimeError):
    pass


def _tile_block(data_off, dst_row, num_values, elem_size):
    """Vectorized per-page tile table (ntiles x 3 u64). A/B'd against
    the per-tile Python loop: roughly neutral at 1 MB pages (~5 ms per
    300 pages either way — planning cost is spread across per-page
    overheads), clearly ahead for small-page files; kept for the
    cheaper downstream vstack (0.8 vs 2.7 ms per 4800 tiles)."""
    starts = np.arange(0, num_values, _TILE, dtype=np.uint64)
    out = np.empty((len(starts), 3), dtype=np.uint64)
    out[:, 0] = data_off + starts * elem_size
    out[:, 1] = dst_row + starts
    out[:, 2] = np.minimum(_TILE, num_values - starts)
    return out


def _check_levels_v1(buf, pos, num_values, max_def, page_end=None):
    """Definition-levels block of a v1 data page ([u32 len][RLE runs]).
    Verify every level == max_def (no nulls) without expanding; return
    the position after the block. With page_end (the position after the
    page's last byte) a block that claims to run past its page is
    refused, as k_snappy_pages refuses it (err 1)."""
    if max_def.bit_length() != 1:
        raise QkParquetError("nested schemas unsupported (max_def=%d)"
                             % max_def)
    ln = int.from_bytes(buf[pos:pos + 4], "little")
    p = pos + 4
    end = p + ln
    if page_end is not None and (p > page_end or end > page_end):
        raise QkParquetError("definition levels run past the page")
    seen = 0
    while seen < num_values and p < end:
        h, p = _varint(buf, p)
        if h & 1:                       # bit-packed groups, bit width 1
            ngroups = h >> 1
            n = min(ngroups * 8, num_values - seen)
            full, rem = n // 8, n % 8
            chunk = bytes(buf[p:p + ngroups])
            if chunk[:full] != b"\xff" * full or \
                    (rem and (chunk[full] & ((1 << rem) - 1))
                     != (1 << rem) - 1):
                raise QkParquetError("page contains nulls")
            p += ngroups
            seen += n
        else:                           # fill run
            val = buf[p]
            p += 1
            n = min(h >> 1, num_values - seen)
            if n and val != max_def:
                raise QkParquetError("page contains nulls")
            seen += n
    return end


def _walk_rle(buf, pos, end, bitwidth, nvalues, dst0, ents):
    """RLE/bit-packed hybrid (parquet encoding.md), walked on the host:
    append run entries (kind, dst, count, value | first bit, bit width)
    covering `nvalues` values starting at output row dst0. The device
    path (qk_pq_rle_pages) parses the runs itself; the CPU plan tests
    keep this walker as their run-level model of a page."""
    seen = 0
    while seen < nvalues:
        if pos >= end:
            raise QkParquetError("RLE data truncated")
        h, pos = _varint(buf, pos)
        if h & 1:
            ngroups = h >> 1
            n = min(ngroups * 8, nvalues - seen)
            s = 0
            while s < n:
                m = min(_TILE, n - s)
                ents.append((1, dst0 + seen + s, m,
                             pos * 8 + s * bitwidth, bitwidth))
                s += m
            pos += ngroups * bitwidth
        else:
            nb = (bitwidth + 7) // 8
            val = int.from_bytes(buf[pos:pos + nb], "little")
            pos += nb
            n = min(h >> 1, nvalues - seen)
            s = 0
            while s < n:
                m = min(_TILE, n - s)
                ents.append((0, dst0 + seen + s, m, val, 0))
                s += m
        seen += n
    return pos


def _plain_page(data, pend, num_values, elem_size):
    """Refuse a PLAIN page whose values run past the page."""
    if data > pend or num_values * elem_size > pend - data:
        raise QkParquetError("PLAIN values run past the page")


def _dict_values(db, pos, end, num_values, dtype, is_ba):
    """Dictionary page db[pos:end] -> np array (fixed width) or list of
    str (BYTE_ARRAY); a page shorter than num_values entries is refused."""
    short = QkParquetError("dictionary page shorter than its %d entries"
                           % num_values)
    if not is_ba:
        if pos > end or num_values * dtype.itemsize > end - pos:
            raise short
        return np.frombuffer(db, dtype=dtype, count=num_values,
                             offset=pos).copy()
    vals = []
    for _ in range(num_values):
        if end - pos < 4:
            raise short
        ln = int.from_bytes(db[pos:pos + 4], "little")
        pos += 4
        if ln > end - pos:
            raise short
        vals.append(bytes(db[pos:pos + ln]).decode())
        pos += ln
    return vals


class _Chunk:
    """Decode plan for one column chunk: PLAIN tiles and/or dictionary
    (values + RLE index entries), all offsets absolute into the file."""

    def __init__(self, buf, col, max_def, dst0, mask=False):
        if col.compression != "UNCOMPRESSED":
            raise QkParquetError("compressed chunks unsupported here (%s); "
                                 "SNAPPY goes through the GPU decompressor "
                                 "(_snappy_column), others are rejected"
                                 % col.compression)
        self.dtype = _PHYS.get(col.physical_type)
        self.is_ba = col.physical_type == "BYTE_ARRAY"
        if self.dtype is None and not self.is_ba:
            raise QkParquetError("unsupported physical type %s"
                                 % col.physical_type)
        start = col.data_page_offset
        if col.dictionary_page_offset is not None:
            start = min(start, col.dictionary_page_offset)
        self.plain_tiles = []
        self.rle_pages = []
        self.dict_vals = None          # np array (fixed) or list (strings)
        self.n = col.num_values
        # mask mode, nullable column: the value plan waits for the
        # device's per-page non-null counts (_decode_masked)
        self.def_pages = []
        mask = mask and max_def > 0
        if mask and max_def != 1:
            raise QkParquetError("nested schemas unsupported (max_def=%d)"
                                 % max_def)
        row = dst0
        for p in T.walk_pages(buf, start, col.total_compressed_size,
                              col.num_values):
            if p.kind == T.PAGE_DICT:
                if p.encoding not in (ENC_PLAIN, ENC_PLAIN_DICT):
                    raise QkParquetError("dict page encoding %d"
                                         % p.encoding)
                self._load_dict(buf, p)
                continue
            if mask:
                self.def_pages.append(
                    _def_page(p, p.data_off, p.data_len, row))
                row += p.num_values
                continue
            if p.kind == T.PAGE_DATA:
                data = p.data_off
                if max_def > 0:
                    data = _check_levels_v1(buf, data, p.num_values,
                                            max_def,
                                            p.data_off + p.data_len)
            else:                       # v2: levels first, lengths known
                if p.num_nulls:
                    raise QkParquetError("page contains nulls")
                data = p.data_off + p.v2_levels_len
            pend = p.data_off + p.data_len
            if p.encoding == ENC_PLAIN:
                if self.is_ba:
                    raise QkParquetError("PLAIN BYTE_ARRAY unsupported; "
                                         "write with use_dictionary=True")
                es = self.dtype.itemsize
                _plain_page(data, pend, p.num_values, es)
                self.plain_tiles.append(
                    _tile_block(data, row, p.num_values, es))
            elif p.encoding == ENC_RLE_DICT:
                if data >= pend:
                    raise QkParquetError("RLE_DICTIONARY page without a "
                                         "bit-width byte")
                bw = buf[data]
                if bw > 32:
                    raise QkParquetError("index bit width %d" % bw)
                # one descriptor per PAGE; the run stream is parsed on
                # the GPU (qk_pq_rle_pages) — low-cardinality columns
                # emit millions of tiny runs and walking them in host
                # Python measured seconds per file
                self.rle_pages.append((data + 1, pend, row,
                                       p.num_values, bw))
            else:
                raise QkParquetError("data page encoding %d" % p.encoding)
            row += p.num_values

    def _load_dict(self, buf, p):
        self.dict_vals = _dict_values(buf, p.data_off,
                                      p.data_off + p.data_len, p.num_values,
                                      self.dtype, self.is_ba)


def _def_page(p, off, size, row):
    """Mask-mode record of one data page whose `size` bytes (levels
    first) start at `off` in the decode source: (levels_off, page_end,
    v2 levels length or None for a v1 page, first row, num_values,
    encoding, v2 header num_nulls or None)."""
    v2 = p.kind != T.PAGE_DATA
    return (off, off + size, p.v2_levels_len if v2 else None, row,
            p.num_values, p.encoding, p.num_nulls if v2 else None)


class _PlanChunk:
    """Duck-typed like _Chunk for _decode_column: a decode plan whose
    offsets point into the DECOMPRESSED scratch buffer instead of the
    file bytes."""

    def __init__(self, col, dtype, is_ba, n):
        self.dtype = dtype
        self.is_ba = is_ba
        self.n = n
        self.plain_tiles = []
        self.rle_pages = []
        self.dict_vals = None
        self.def_pages = []


def _snappy_column(shim, raw, dev_file, cols_meta, max_def, dst0,
                   mask=False):
    """Plan + decompress one column whose chunks are SNAPPY-compressed
    (or a mix of SNAPPY and UNCOMPRESSED pages): every page's
    decompressed bytes land in one scratch DevBuffer via qk_snappy_pages
    (one wave per page; v1 definition levels verified in-kernel), then
    the normal qk_pq_plain_copy / qk_pq_rle_pages decode runs against
    the scratch. Returns (list of _PlanChunk, scratch DevBuffer) —
    caller passes scratch as the decode source and frees it.

    The reference reads compressed files transparently through pyarrow
    (unordered_readers.py:51); real TPC-H datasets usually ship snappy."""
    import ctypes
    from .shim import DevBuffer, c_u64, c_vp

    if max_def > 1 or (max_def and max_def.bit_length() != 1):
        raise QkParquetError("nested schemas unsupported (max_def=%d)"
                             % max_def)
    phys = cols_meta[0].physical_type
    dtype = _PHYS.get(phys)
    is_ba = phys == "BYTE_ARRAY"
    if dtype is None and not is_ba:
        raise QkParquetError("unsupported physical type %s" % phys)
    # mask mode, nullable column: levels stay in the scratch buffer for
    # qk_pq_def_pages, nothing here verifies or refuses them
    mask = mask and max_def > 0

    chunk_pages = []
    row = dst0
    for col in cols_meta:
        if col.compression not in ("SNAPPY", "GZIP", "UNCOMPRESSED"):
            raise QkParquetError("compression %s unsupported (SNAPPY, "
                                 "GZIP and UNCOMPRESSED only)"
                                 % col.compression)
        start = col.data_page_offset
        if col.dictionary_page_offset is not None:
            start = min(start, col.dictionary_page_offset)
        pl = T.walk_pages(raw, start, col.total_compressed_size,
                          col.num_values)
        chunk_pages.append((col, pl, row))
        row += col.num_values

    descs = []          # qk_snappy_pages descriptors
    gdescs = []         # qk_gzip_pages descriptors
    copies = []         # byte-copy tiles (uncompressed pages / v2 levels)
    plans = []          # per page: post-processing info
    off = 0
    for ci, (col, pl, row0) in enumerate(chunk_pages):
        rows = row0
        for p in pl:
            # v2 pages carry is_compressed (writers leave incompressible
            # pages raw and clear it) — those route to the byte-copy path
            codec = col.compression if p.is_compressed else "UNCOMPRESSED"
            if codec == "GZIP" and p.kind == T.PAGE_DATA and max_def > 0 \
                    and not mask:
                # a nullable v1 page keeps its def-levels INSIDE the
                # compressed stream; the gzip kernel (unlike snappy's)
                # does not parse them — write non-nullable or v2 pages
                raise QkParquetError(
                    "GZIP v1 pages with definition levels unsupported; "
                    "write the column non-nullable or data_page_version"
                    "='2.0'")
            ent = {"chunk": ci, "page": p, "off": off, "row": rows,
                   "desc": None, "codec": codec}
            if codec == "UNCOMPRESSED":
                copies.append((p.data_off, off, p.data_len))
                ent["kind"] = "raw"
                ent["size"] = p.data_len
            elif p.kind == T.PAGE_DATA:            # v1: levels inside
                ent["kind"] = "v1"
                ent["size"] = p.uncompressed_len
                if codec == "SNAPPY":
                    descs.append((p.data_off, p.data_len, off,
                                  p.uncompressed_len,
                                  2 if mask else 1 if max_def > 0 else 0,
                                  p.num_values, 0, 0))
                    ent["desc"] = len(descs) - 1
                else:
                    gdescs.append((p.data_off, p.data_len, off,
                                   p.uncompressed_len, 1, 0, 0, 0))
                    ent["gdesc"] = len(gdescs) - 1
            elif p.kind == T.PAGE_DICT:
                ent["kind"] = "dict"
                ent["size"] = p.uncompressed_len
                if codec == "SNAPPY":
                    descs.append((p.data_off, p.data_len, off,
                                  p.uncompressed_len, 0, p.num_values,
                                  0, 0))
                    ent["desc"] = len(descs) - 1
                else:
                    gdescs.append((p.data_off, p.data_len, off,
                                   p.uncompressed_len, 1, 0, 0, 0))
                    ent["gdesc"] = len(gdescs) - 1
            else:                                  # v2: levels NOT compressed
                if p.num_nulls and not mask:
                    raise QkParquetError("page contains nulls")
                lv = p.v2_levels_len
                if lv:
                    copies.append((p.data_off, off, lv))
                ent["kind"] = "v2"
                ent["size"] = p.uncompressed_len
                if codec == "SNAPPY":
                    descs.append((p.data_off + lv, p.data_len - lv,
                                  off + lv, p.uncompressed_len - lv, 0,
                                  p.num_values, 0, 0))
                    ent["desc"] = len(descs) - 1
                else:
                    gdescs.append((p.data_off + lv, p.data_len - lv,
                                   off + lv, p.uncompressed_len - lv, 1,
                                   0, 0, 0))
                    ent["gdesc"] = len(gdescs) - 1
            if p.kind != T.PAGE_DICT:
                rows += p.num_values
            plans.append(ent)
            off += ent["size"]

    scratch = DevBuffer(off + 8)
    try:                    # a refusal below gives the scratch back
        if copies:
            tiles = np.asarray(copies, dtype=np.uint64)
            dt = DevBuffer(tiles.nbytes)
            shim.call("qk_h2d", dt.ptr, tiles.ctypes.data_as(c_vp),
                      c_u64(tiles.nbytes))
            shim.call("qk_pq_plain_copy", None, c_u64(len(tiles)), dt.ptr,
                      dev_file.ptr, scratch.ptr, ctypes.c_uint32(1))
            dt.free()
        gresults = None
        if gdescs:
            ga = np.asarray(gdescs, dtype=np.uint64)
            gd = DevBuffer(ga.nbytes)
            shim.call("qk_h2d", gd.ptr, ga.ctypes.data_as(c_vp),
                      c_u64(ga.nbytes))
            gout = DevBuffer(len(gdescs) * 4 * 8)
            shim.call("qk_gzip_pages", None, c_u64(len(gdescs)), gd.ptr,
                      dev_file.ptr, scratch.ptr, gout.ptr)
            shim.call("qk_stream_sync", None)
            gresults = np.zeros(len(gdescs) * 4, dtype=np.int64)
            shim.call("qk_d2h", gresults.ctypes.data_as(c_vp), gout.ptr,
                      c_u64(gresults.nbytes))
            gresults = gresults.reshape(-1, 4)
            gd.free()
            gout.free()
            bad = np.nonzero(gresults[:, 1])[0]
            if bad.size:
                code = int(gresults[bad[0], 1])
                raise QkParquetError(
                    "gzip page %d failed: %s" % (
                        bad[0], {1: "corrupt stream",
                                 2: "uncompressed-length mismatch",
                                 3: "unsupported feature"}.get(code, code)))
        results = None
        if descs:
            da = np.asarray(descs, dtype=np.uint64)
            dd = DevBuffer(da.nbytes)
            shim.call("qk_h2d", dd.ptr, da.ctypes.data_as(c_vp),
                      c_u64(da.nbytes))
            dout = DevBuffer(len(descs) * 4 * 8)
            shim.call("qk_snappy_pages", None, c_u64(len(descs)), dd.ptr,
                      dev_file.ptr, scratch.ptr, dout.ptr)
            shim.call("qk_stream_sync", None)
            results = np.zeros(len(descs) * 4, dtype=np.int64)
            shim.call("qk_d2h", results.ctypes.data_as(c_vp), dout.ptr,
                      c_u64(results.nbytes))
            results = results.reshape(-1, 4)
            dd.free()
            dout.free()
            bad = np.nonzero(results[:, 1])[0]
            if bad.size:
                code = int(results[bad[0], 1])
                raise QkParquetError(
                    "snappy page %d failed: %s" % (
                        bad[0], {1: "corrupt stream",
                                 2: "uncompressed-length mismatch",
                                 3: "page contains nulls"}.get(code, code)))

        out_chunks = []
        cur = None
        scratch_host = {}       # chunk dict pages d2h'd lazily

        def _scratch_bytes(o, ln):
            arr = np.empty(ln, dtype=np.uint8)
            shim.call("qk_d2h", arr.ctypes.data_as(c_vp),
                      ctypes.c_void_p(scratch.ptr.value + o), c_u64(ln))
            return arr.tobytes()

        for ci, (col, pl, row0) in enumerate(chunk_pages):
            cur = _PlanChunk(col, dtype, is_ba, col.num_values)
            out_chunks.append(cur)
        for ent in plans:
            p = ent["page"]
            cur = out_chunks[ent["chunk"]]
            o = ent["off"]
            if ent["kind"] == "dict" or (ent["kind"] == "raw"
                                         and p.kind == T.PAGE_DICT):
                if p.encoding not in (ENC_PLAIN, ENC_PLAIN_DICT):
                    raise QkParquetError("dict page encoding %d" % p.encoding)
                if ent["kind"] == "dict":
                    db = _scratch_bytes(o, ent["size"])
                else:
                    db = bytes(raw[p.data_off:p.data_off + p.data_len])
                cur.dict_vals = _dict_values(db, 0, len(db), p.num_values,
                                             dtype, is_ba)
                continue
            if mask:
                # every kind of data page lies in the scratch at `o`, levels
                # first: raw pages with their file length, the others with
                # their uncompressed length
                cur.def_pages.append(_def_page(p, o, ent["size"], ent["row"]))
                continue
            # data pages: find where values start + the RLE bit-width byte
            if ent["kind"] == "v1":
                if ent.get("gdesc") is not None:
                    # GZIP v1 reaches here only with max_def == 0 (no
                    # levels inside): values start at the page start
                    data = o
                    first = int(gresults[ent["gdesc"]][2])
                else:
                    r = results[ent["desc"]]
                    data = o + int(r[0])
                    first = int(r[2])
                end = o + ent["size"]
            elif ent["kind"] == "v2":
                data = o + p.v2_levels_len
                if ent.get("gdesc") is not None:
                    first = int(gresults[ent["gdesc"]][2])
                else:
                    first = int(results[ent["desc"]][2])
                end = o + ent["size"]
            else:                                       # raw page in scratch
                data_abs = p.data_off
                if p.kind == T.PAGE_DATA:
                    if max_def > 0:
                        data_abs = _check_levels_v1(raw, data_abs,
                                                    p.num_values, max_def,
                                                    p.data_off + p.data_len)
                else:
                    if p.num_nulls:
                        raise QkParquetError("page contains nulls")
                    data_abs = p.data_off + p.v2_levels_len
                data = o + (data_abs - p.data_off)
                first = raw[data_abs] if data_abs < p.data_off + p.data_len \
                    else -1
                end = o + ent["size"]
            if p.encoding == ENC_PLAIN:
                if is_ba:
                    raise QkParquetError("PLAIN BYTE_ARRAY unsupported; "
                                         "write with use_dictionary=True")
                _plain_page(data, end, p.num_values, dtype.itemsize)
                cur.plain_tiles.append(
                    _tile_block(data, ent["row"], p.num_values,
                                dtype.itemsize))
            elif p.encoding == ENC_RLE_DICT:
                bw = first
                if bw < 0 or data >= end:
                    raise QkParquetError("RLE_DICTIONARY page without a "
                                         "bit-width byte")
                if bw > 32:
                    raise QkParquetError("index bit width %d" % bw)
                cur.rle_pages.append((data + 1, end, ent["row"],
                                      p.num_values, bw))
            else:
                raise QkParquetError("data page encoding %d" % p.encoding)
    except BaseException:
        scratch.free()
        raise
    return out_chunks, scratch


def _upload(shim, host_bytes):
    """File bytes -> device, with the 8-byte slack qk_pq_rle_pages needs."""
    from .shim import DevBuffer, c_u64, c_vp
    arr = np.frombuffer(host_bytes, dtype=np.uint8)
    buf = DevBuffer(len(arr) + 8)
    shim._bounce.h2d(buf.ptr, arr)
    return buf


_DEF_ERR = {1: "definition levels run past the page",
            2: "definition levels truncated",
            3: "definition level above 1 (nested schemas unsupported)"}
_RLE_ERR = {1: "index stream truncated",
            2: "index at or above the dictionary length",
            3: "bit width above 32 or stream offsets reversed"}
_V1 = (1 << 64) - 1     # qk_pq_def_pages: v2_levels_len marker of a v1 page


def _def_descs(chunks):
    """qk_pq_def_pages descriptors (npages x 6 u64) of a mask-mode column,
    in page order."""
    return np.asarray(
        [(off, end, _V1 if v2len is None else v2len, row, nv, 0)
         for ch in chunks
         for (off, end, v2len, row, nv, _enc, _nn) in ch.def_pages],
        dtype=np.uint64).reshape(-1, 6)


def _dense_plan(chunks, results):
    """Mask mode, after qk_pq_def_pages: `results` is its per-page table
    (npages x 4 i64 [non_null, values_off, err, first_value_byte]).
    Fills each chunk's plain_tiles / rle_pages so that every page decodes
    its `non_null` stored values to DENSE positions (host prefix sum of
    the per-page counts). Returns the total non-null count."""
    dense = 0
    k = 0
    for ch in chunks:
        ch.plain_tiles, ch.rle_pages = [], []
        for (off, end, v2len, row, nv, enc, hdr_nulls) in ch.def_pages:
            nn, voff, err, first = (int(x) for x in results[k])
            k += 1
            if err:
                raise QkParquetError("page %d: %s"
                                     % (k - 1, _DEF_ERR.get(err, err)))
            if hdr_nulls is not None and nn != nv - hdr_nulls:
                # v1 headers carry no null count; v2's must agree
                raise QkParquetError(
                    "page %d: definition levels give %d non-null values, "
                    "the page header %d" % (k - 1, nn, nv - hdr_nulls))
            if enc == ENC_PLAIN:
                if ch.is_ba:
                    raise QkParquetError("PLAIN BYTE_ARRAY unsupported; "
                                         "write with use_dictionary=True")
                if nn:
                    es = ch.dtype.itemsize
                    if voff + nn * es > end:
                        raise QkParquetError("PLAIN values run past the "
                                             "page")
                    ch.plain_tiles.append(_tile_block(voff, dense, nn, es))
            elif enc == ENC_RLE_DICT:
                # an all-null page has no index stream, possibly not even
                # the bit-width byte
                if nn:
                    if first < 0 or first > 32:
                        raise QkParquetError("index bit width %d" % first)
                    ch.rle_pages.append((voff + 1, end, dense, nn, first))
            else:
                raise QkParquetError("data page encoding %d" % enc)
            dense += nn
    return dense


def _decode_masked(shim, src, chunks, total):
    """Mask-mode decode of one nullable column from the decode source
    `src` (file bytes or decompressed scratch): qk_pq_def_pages ->
    validity bitmap + per-page counts, the unchanged value kernels into a
    dense temporary, qk_valid_expand into the row-aligned column.
    Returns an ops.NullableColumn — a plain DevColumn when no row is
    null — or (that, values list) for BYTE_ARRAY dictionary columns."""
    import ctypes
    from .ops import NullableColumn, valid_nbytes
    from .shim import DevBuffer, DevColumn, c_u64, c_vp
    descs = _def_descs(chunks)
    npages = len(descs)
    if npages and int((descs[:, 3] + descs[:, 4]).max()) > total:
        raise QkParquetError("pages hold more rows than the file")
    nb = valid_nbytes(total)
    valid = DevBuffer(nb)
    shim.call("qk_dmemset", valid.ptr, 0, c_u64(nb))
    results = np.zeros((npages, 4), dtype=np.int64)
    if npages:
        dd = DevBuffer(descs.nbytes)
        shim.call("qk_h2d", dd.ptr, descs.ctypes.data_as(c_vp),
                  c_u64(descs.nbytes))
        dout = DevBuffer(results.nbytes)
        shim.call("qk_pq_def_pages", None, c_u64(npages), dd.ptr, src.ptr,
                  valid.ptr, dout.ptr)
        shim.call("qk_stream_sync", None)
        shim.call("qk_d2h", results.ctypes.data_as(c_vp), dout.ptr,
                  c_u64(results.nbytes))
        dd.free()
        dout.free()
    try:
        nonnull = _dense_plan(chunks, results)
        dense = _decode_column(shim, src, chunks, nonnull)
    except QkParquetError:
        valid.free()
        raise
    vals = None
    if chunks[0].is_ba:
        dense, vals = dense
    if nonnull == total:
        valid.free()
        out = dense
    else:
        col = DevColumn(dense.dtype, max(1, total))
        col.n = total
        shim.call("qk_valid_expand", None, c_u64(total), valid.ptr,
                  dense.ptr, col.ptr, ctypes.c_uint32(dense.dtype.itemsize))
        shim.call("qk_stream_sync", None)
        dense.free()
        out = NullableColumn(col, valid, total, total - nonnull)
    return (out, vals) if vals is not None else out


def read_table(source, columns=None, nulls="raise"):
    """Decode a Parquet file into device columns.

    source: path or bytes. Returns dict name -> DevColumn for fixed-width
    columns, and name -> (DevColumn u32 codes, list values) for
    dictionary-encoded BYTE_ARRAY columns (the executors' string-dict
    form, quokka_amd/executors.py StringDict).

    nulls="raise" (default): a page that holds a null raises
    QkParquetError. nulls="mask": a flat nullable column with at least
    one null comes back as an ops.NullableColumn (null slots hold 0; for
    a dictionary BYTE_ARRAY column the u32 codes are the NullableColumn
    and null slots hold code 0); one without nulls still comes back as a
    plain DevColumn."""
    if nulls not in ("raise", "mask"):
        raise ValueError("nulls must be 'raise' or 'mask', got %r"
                         % (nulls,))
    mask = nulls == "mask"
    import pyarrow.parquet as pq
    from . import shim
    from .shim import DevBuffer, DevColumn, c_u64, c_vp
    import ctypes
    import io

    if isinstance(source, str):
        # mmap instead of read(): the page-cache copy then happens inside
        # the pinned upload bounce (4-thread memmove overlapped with DMA)
        # rather than as a separate full-file pass
        import mmap
        fh = open(source, "rb")
        raw = mmap.mmap(fh.fileno(), 0, prot=mmap.PROT_READ)
        f = pq.ParquetFile(source)
    else:
        raw = source
        f = pq.ParquetFile(io.BytesIO(raw))
    md = f.metadata
    names = [md.schema.column(i).name for i in range(md.num_columns)]
    want = [i for i, nm in enumerate(names)
            if columns is None or nm in columns]
    total = md.num_rows
    # overlap the file-bytes upload (DMA + memmove threads, GIL released)
    # with the host-side page planning below — the two dominant costs of
    # a warm scan after the kernels
    import threading
    up = {}

    def _up():
        up["dev"] = _upload(shim, raw)

    th = threading.Thread(target=_up)
    th.start()

    class _LazyDev:
        @property
        def ptr(self):
            th.join()
            return up["dev"].ptr

        def free(self):
            th.join()
            up["dev"].free()

    dev_file = _LazyDev()
    out = {}
    try:
        # phase 1 (host only, overlaps the upload): plan every
        # uncompressed column's pages/tiles
        plans = {}
        for ci in want:
            max_def = md.schema.column(ci).max_definition_level
            cols_meta = [md.row_group(rg).column(ci)
                         for rg in range(md.num_row_groups)]
            comps = {c.compression for c in cols_meta}
            if comps & {"SNAPPY", "GZIP"}:
                plans[ci] = ("snappy", cols_meta, max_def)
                continue
            chunks = []
            row = 0
            for col in cols_meta:
                ch = _Chunk(raw, col, max_def, row, mask)
                row += ch.n
                chunks.append(ch)
            assert row == total, (row, total)
            plans[ci] = ("plain", chunks, max_def)
        # phase 2: device decode (first ptr access joins the upload)
        for ci in want:
            kind, payload, max_def = plans[ci]
            masked = mask and max_def > 0
            if kind == "snappy":
                chunks, scratch = _snappy_column(shim, raw, dev_file,
                                                 payload, max_def, 0, mask)
                assert sum(ch.n for ch in chunks) == total
                decode = _decode_masked if masked else _decode_column
                try:
                    out[names[ci]] = decode(shim, scratch, chunks, total)
                    shim.call("qk_stream_sync", None)
                finally:
                    scratch.free()
            elif masked:
                out[names[ci]] = _decode_masked(shim, dev_file, payload,
                                                total)
            else:
                out[names[ci]] = _decode_column(shim, dev_file, payload,
                                                total)
        shim.call("qk_stream_sync", None)
        return out
    except QkParquetError:
        # columns decoded before the one that was refused
        for c in out.values():
            (c[0] if isinstance(c, tuple) else c).free()
        raise
    finally:
        dev_file.free()
        if isinstance(source, str):
            raw.close()
            fh.close()


def _rle_ents(chunks):
    """qk_pq_rle_pages descriptors of one column (npages x 8 u64
    [src_off, src_end, dst_off, count, bit_width, idx_off, dict_n, 0]):
    idx_off rebases each chunk's dictionary into the column-global
    concatenation, dict_n is that chunk's own dictionary length. Returns
    (ents, per-chunk dictionary parts, BYTE_ARRAY value -> global code).
    Pages that hold no value are dropped; a chunk whose pages hold values
    but whose dictionary is empty is refused, so the gather never meets
    an empty dictionary."""
    is_ba = chunks[0].is_ba
    pages = []
    dict_parts = []
    glob = {}
    if is_ba:
        for ch in chunks:
            for v in ch.dict_vals or []:
                glob.setdefault(v, len(glob))
    dict_off = 0
    for ch in chunks:
        rle = [pg for pg in ch.rle_pages if pg[3]]
        if not rle:
            continue
        if ch.dict_vals is None:
            raise QkParquetError("RLE_DICTIONARY page without dictionary "
                                 "page")
        if not len(ch.dict_vals):
            raise QkParquetError("RLE_DICTIONARY page with values but an "
                                 "empty dictionary")
        for (s, e, d, c, bw) in rle:
            pages.append((s, e, d, c, bw, dict_off, len(ch.dict_vals), 0))
        if is_ba:
            dict_parts.append(np.asarray([glob[v] for v in ch.dict_vals],
                                         dtype=np.int32))
        else:
            dict_parts.append(np.ascontiguousarray(ch.dict_vals))
        dict_off += len(ch.dict_vals)
    return (np.asarray(pages, dtype=np.uint64).reshape(-1, 8), dict_parts,
            glob)


def _decode_column(shim, dev_file, chunks, total):
    """Decode one column (all row-group chunks) with at most three
    launches: ONE qk_pq_rle_pages over every dictionary page of every
    chunk (per-page idx_off rebases each chunk's dictionary into the
    column-global concatenation), ONE gather through the concatenated
    dictionary, ONE qk_pq_plain_copy over every PLAIN tile (launched
    last so PLAIN rows overwrite the gather's placeholder writes —
    pyarrow's mid-chunk dictionary->PLAIN fallback leaves such rows).
    Per-chunk launches measured 0.34 ms each x hundreds of 1M-row
    chunks; batched, the whole column is a handful of full-chip
    launches. Returns a DevColumn, or (u32 code DevColumn, values list)
    for BYTE_ARRAY dictionary columns."""
    import ctypes
    from .shim import DevBuffer, DevColumn, c_u64, c_vp
    is_ba = chunks[0].is_ba
    ents, dict_parts, glob = _rle_ents(chunks)

    dt = np.dtype(np.uint32) if is_ba else chunks[0].dtype
    col_out = DevColumn(dt, max(1, total))
    col_out.n = total
    errs = derr = None
    if len(ents):
        dents = DevBuffer(ents.nbytes)
        shim.call("qk_h2d", dents.ptr, ents.ctypes.data_as(c_vp),
                  c_u64(ents.nbytes))
        idx = DevColumn(np.uint32, max(1, total))
        errs = np.zeros(len(ents), dtype=np.int64)
        derr = DevBuffer(errs.nbytes)
        # rows covered only by PLAIN pages keep index 0 here; the final
        # plain-copy launch overwrites them with decoded values
        shim.call("qk_dmemset", idx.ptr, 0, c_u64(4 * max(1, total)))
        shim.call("qk_pq_rle_pages", None, c_u64(len(ents)), dents.ptr,
                  dev_file.ptr, idx.ptr, derr.ptr)
        # the kernel keeps every index inside its chunk's dictionary, so
        # the gather is safe before the error table has been looked at
        dcat = DevColumn.from_numpy(np.concatenate(dict_parts))
        gather = {8: "qk_gather_i64", 4: "qk_gather_i32"}[dt.itemsize]
        shim.call(gather, None, c_u64(total), idx.ptr, dcat.ptr,
                  col_out.ptr)
        dents.free()
        idx.free()
        dcat.free()
    all_tiles = [np.atleast_2d(np.asarray(t, dtype=np.uint64))
                 for ch in chunks for t in ch.plain_tiles]
    if all_tiles:
        tiles = np.ascontiguousarray(np.vstack(all_tiles))
        dtile = DevBuffer(tiles.nbytes)
        shim.call("qk_h2d", dtile.ptr, tiles.ctypes.data_as(c_vp),
                  c_u64(tiles.nbytes))
        shim.call("qk_pq_plain_copy", None, c_u64(len(tiles)), dtile.ptr,
                  dev_file.ptr, col_out.ptr,
                  ctypes.c_uint32(dt.itemsize))
        dtile.free()
    if derr is not None:
        # one read-back per dictionary column, after all its launches
        shim.call("qk_stream_sync", None)
        shim.call("qk_d2h", errs.ctypes.data_as(c_vp), derr.ptr,
                  c_u64(errs.nbytes))
        derr.free()
        bad = np.nonzero(errs)[0]
        if bad.size:
            col_out.free()
            code = int(errs[bad[0]])
            raise QkParquetError("dictionary index page %d: %s"
                                 % (bad[0], _RLE_ERR.get(code, code)))
    if is_ba:
        return col_out, sorted(glob, key=glob.get)
    return col_out
