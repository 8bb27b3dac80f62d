"""CPU tests of the mask-mode Parquet decode PLAN (nulls="mask"): numpy
simulators of qk_pq_def_pages and qk_valid_expand run over the real plan
(_Chunk(mask=True) -> _def_descs -> _dense_plan) and the result is
compared with pyarrow's decode of the same file: values where valid, and
the is_valid() mask. Hand-built level blocks check that a corrupt stream
ends in an error code and never reads past its page. The GPU suite runs
the same shapes through the kernels."""
import io

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

from quokka_amd import parquet_gpu as P  # noqa: E402

ERR_PAST, ERR_TRUNC, ERR_LEVEL = 1, 2, 3


class Guard(bytes):
    """bytes that refuse an index at or past `limit` — the page end."""
    limit = None

    def __getitem__(self, i):
        assert isinstance(i, int) and 0 <= i < self.limit, \
            "read at %r, page ends at %d" % (i, self.limit)
        return bytes.__getitem__(self, i)


def sim_def_pages(src, descs, valid_words):
    """qk_pq_def_pages, lane by lane semantics folded into row loops.
    valid_words: np.uint64 bitmap, pre-zeroed, OR-ed into. Returns the
    npages x 4 result table."""
    out = np.zeros((len(descs), 4), dtype=np.int64)
    for pg, (pos, page_end, v2len, row0, nrows, _) in enumerate(
            np.asarray(descs, dtype=np.uint64).tolist()):
        err = 0
        if v2len == P._V1:
            if pos > page_end or page_end - pos < 4:
                err, end = ERR_PAST, pos
            else:
                ln = int.from_bytes(bytes(src[pos + i] for i in range(4)),
                                    "little")
                pos += 4
                end = pos + ln
                if end > page_end:
                    err = ERR_PAST
        else:
            end = pos + v2len
            if pos > page_end or v2len > page_end - pos:
                err = ERR_PAST
        row, remaining, nonnull = row0, nrows, 0
        steps = 0
        while not err and remaining and pos < end:
            steps += 1
            assert steps <= end, "run loop does not advance"
            h, shift, npos, bad = 0, 0, pos, ERR_TRUNC
            while npos < end and shift < 64:
                b = src[npos]
                npos += 1
                h |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    bad = 0
                    break
            val = 0
            if not bad and not h & 1:
                if npos >= end:
                    bad = ERR_TRUNC
                else:
                    val = src[npos]
                    npos += 1
                    if val > 1:
                        bad = ERR_LEVEL
            if bad:
                err = bad
                break
            if h & 1:
                ngroups = h >> 1
                if ngroups > end - npos:
                    err = ERR_TRUNC
                    break
                n = min(ngroups * 8, remaining)
                bits = [(src[npos + (i >> 3)] >> (i & 7)) & 1
                        for i in range(n)]
                npos += ngroups
            else:
                n = min(h >> 1, remaining)
                bits = [val] * n
            for i, b in enumerate(bits):
                if b:
                    r = row + i
                    valid_words[r >> 6] |= np.uint64(1 << (r & 63))
                    nonnull += 1
            row += n
            remaining -= n
            pos = npos
        if not err and remaining:
            err = ERR_TRUNC
        first = src[end] if not err and end < page_end else -1
        out[pg] = (nonnull, end, err, first)
    return out


def sim_valid_expand(valid_words, dense, n):
    """qk_valid_expand: out[row] = valid ? dense[rank(row)] : 0."""
    bits = np.unpackbits(valid_words.view(np.uint8),
                         bitorder="little")[:n].astype(bool)
    rank = np.cumsum(bits) - bits
    out = np.zeros(n, dtype=dense.dtype)
    out[bits] = dense[rank[bits]]
    return out, bits


def sim_rle_page(raw, src, end, cnt, bw):
    """One qk_pq_rle_pages descriptor -> u32 indices (host run walker)."""
    if bw == 0:
        return np.zeros(cnt, dtype=np.uint32)
    ents = []
    P._walk_rle(raw, src, end, bw, cnt, 0, ents)
    out = np.empty(cnt, dtype=np.uint32)
    pad = raw + b"\0" * 8
    for kind, dst, m, a, b in ents:
        if kind == 0:
            out[dst:dst + m] = a
        else:
            for i in range(m):
                bit = a + i * b
                w = int.from_bytes(pad[bit >> 3:(bit >> 3) + 8], "little")
                out[dst + i] = (w >> (bit & 7)) & ((1 << b) - 1)
    return out


def sim_masked_column(raw, ci):
    """Numpy run of read_table(nulls='mask') for one uncompressed column:
    -> (values with 0 in null slots, valid mask, dict values or None)."""
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    max_def = md.schema.column(ci).max_definition_level
    assert max_def == 1
    total = md.num_rows
    chunks, row = [], 0
    for rg in range(md.num_row_groups):
        ch = P._Chunk(raw, md.row_group(rg).column(ci), max_def, row,
                      mask=True)
        assert not ch.plain_tiles and not ch.rle_pages   # plan deferred
        row += ch.n
        chunks.append(ch)
    assert row == total
    descs = P._def_descs(chunks)
    assert descs.shape == (sum(len(c.def_pages) for c in chunks), 6)
    words = np.zeros(P_valid_words(total), dtype=np.uint64)
    results = sim_def_pages(raw, descs, words)
    nonnull = P._dense_plan(chunks, results)
    is_ba = chunks[0].is_ba
    dt = np.dtype(np.uint32) if is_ba else chunks[0].dtype
    dense = np.zeros(nonnull, dtype=dt)
    glob = {}
    for ch in chunks:
        for v in (ch.dict_vals or []) if is_ba else []:
            glob.setdefault(v, len(glob))
    for ch in chunks:
        for (s, e, d, c, bw) in ch.rle_pages:
            idx = sim_rle_page(raw, s, e, c, bw)
            if is_ba:
                remap = np.asarray([glob[v] for v in ch.dict_vals],
                                   dtype=np.uint32)
                dense[d:d + c] = remap[idx]
            else:
                dense[d:d + c] = ch.dict_vals[idx]
        for blk in ch.plain_tiles:
            for s, d, c in np.asarray(blk, dtype=np.int64).tolist():
                dense[d:d + c] = np.frombuffer(raw, dtype=dt, count=c,
                                               offset=s)
    out, bits = sim_valid_expand(words, dense, total)
    assert int(bits.sum()) == nonnull
    return out, bits, (sorted(glob, key=glob.get) if is_ba else None)


def P_valid_words(n):
    from quokka_amd.ops import valid_nbytes
    return valid_nbytes(n) // 8


N = 20_011


def null_mask(pattern, n, rng):
    """True = valid."""
    if pattern == "bernoulli":
        return rng.random(n) > 0.5
    if pattern == "blocks":
        return (np.arange(n) // 777) % 2 == 0
    if pattern == "allnull":
        return np.zeros(n, dtype=bool)
    if pattern == "lastnull":
        m = np.ones(n, dtype=bool)
        m[-1] = False
        return m
    assert pattern == "none"
    return np.ones(n, dtype=bool)


def make_array(kind, n, mask, rng):
    if kind == "i64":
        v = rng.integers(-1 << 40, 1 << 40, n)
        return pa.array(v, mask=~mask, type=pa.int64())
    if kind == "f64":
        return pa.array(rng.random(n) + 1.0, mask=~mask, type=pa.float64())
    if kind == "i32":
        v = rng.integers(1, 1 << 30, n).astype(np.int32)
        return pa.array(v, mask=~mask, type=pa.int32())
    if kind == "dict_i64":
        return pa.array(rng.integers(1, 40, n) * 1000, mask=~mask,
                        type=pa.int64())
    assert kind == "dict_str"
    words = np.asarray(["w%02d" % i for i in range(23)], dtype=object)
    return pa.array(words[rng.integers(0, 23, n)], mask=~mask,
                    type=pa.string())


def write(arr, version, compression="NONE", kind="i64"):
    buf = io.BytesIO()
    pq.write_table(pa.table({"x": arr}), buf, compression=compression,
                   data_page_version=version,
                   use_dictionary=kind.startswith("dict"),
                   data_page_size=2048, write_batch_size=500,
                   row_group_size=7001)
    return buf.getvalue()


def check(raw, arr, kind):
    got, bits, vals = sim_masked_column(raw, 0)
    want = pq.read_table(io.BytesIO(raw)).column("x").combine_chunks()
    assert want.equals(arr)
    wmask = want.is_valid().to_numpy(zero_copy_only=False)
    assert np.array_equal(bits, wmask)
    assert not got[~bits].any()                      # null slots hold 0
    if kind == "dict_str":
        wv = np.asarray(want.to_pylist(), dtype=object)[wmask]
        assert np.array_equal(np.asarray(vals, dtype=object)[got[bits]], wv)
    else:
        wv = want.fill_null(0).to_numpy(zero_copy_only=False)
        assert np.array_equal(got[bits], wv[wmask])


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("kind", ["i64", "f64", "i32", "dict_i64",
                                  "dict_str"])
@pytest.mark.parametrize("pattern", ["bernoulli", "blocks", "allnull",
                                     "lastnull", "none"])
def test_mask_plan_matches_pyarrow(pattern, kind, version):
    rng = np.random.default_rng(7)
    mask = null_mask(pattern, N, rng)
    arr = make_array(kind, N, mask, rng)
    raw = write(arr, version, kind=kind)
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    assert md.num_row_groups == 3
    check(raw, arr, kind)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8192, 8193])
def test_mask_plan_row_count_edges(n):
    rng = np.random.default_rng(n)
    mask = null_mask("bernoulli", n, rng)
    mask[-1] = False
    arr = make_array("i64", n, mask, rng)
    check(write(arr, "1.0"), arr, "i64")


def test_pages_start_mid_word():
    """The premise of the shared-edge-word rule: with these writer
    settings almost no page starts on a 64-row boundary."""
    rng = np.random.default_rng(1)
    arr = make_array("i64", N, null_mask("bernoulli", N, rng), rng)
    raw = write(arr, "1.0")
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    rows, row = [], 0
    for rg in range(md.num_row_groups):
        ch = P._Chunk(raw, md.row_group(rg).column(0), 1, row, mask=True)
        rows += [d[3] for d in ch.def_pages]
        row += ch.n
    assert len(rows) > 10
    assert sum(1 for r in rows if r % 64) >= len(rows) - 3


# ---- corrupt level blocks: an error code, never an overrun ---------------

def run_block(block, nrows, v2len=None, page_len=None):
    """One page made of `block` alone (page_len defaults to its length),
    followed by poison the simulator must not touch."""
    page_len = len(block) if page_len is None else page_len
    src = Guard(block + b"\xAA" * 64)
    src.limit = page_len
    words = np.zeros(P_valid_words(nrows), dtype=np.uint64)
    desc = [(0, page_len, P._V1 if v2len is None else v2len, 0, nrows, 0)]
    res = sim_def_pages(src, desc, words)[0]
    return res, words


def v1(levels):
    return len(levels).to_bytes(4, "little") + levels


def vi(x):
    """ULEB128 varint, the run-header encoding."""
    out = bytearray()
    while True:
        out.append((x & 0x7F) | (0x80 if x > 0x7F else 0))
        x >>= 7
        if not x:
            return bytes(out)


def test_good_blocks():
    # RLE run of 100 ones
    res, words = run_block(v1(vi(100 << 1) + b"\x01"), 100)
    assert res.tolist()[:3] == [100, 7, 0]
    assert int(words[0]) == (1 << 64) - 1 and int(words[1]) == (1 << 36) - 1
    # bit-packed: 2 groups, 13 rows used
    res, words = run_block(v1(bytes([(2 << 1) | 1, 0b10110101, 0xFF])), 13)
    assert res.tolist()[:3] == [10, 7, 0]
    assert int(words[0]) == 0b1111110110101
    # v2: no prefix
    res, _ = run_block(bytes([7 << 1, 0]), 7, v2len=2)
    assert res.tolist()[:3] == [0, 2, 0]


def test_truncated_run_header():
    # varint continuation bit set on the block's last byte
    res, _ = run_block(v1(bytes([0x80])), 50)
    assert res[2] == ERR_TRUNC
    # RLE header without its value byte
    res, _ = run_block(v1(bytes([50 << 1])), 50)
    assert res[2] == ERR_TRUNC
    # bit-packed header that claims more groups than the block holds
    res, _ = run_block(v1(bytes([(9 << 1) | 1, 0xFF, 0xFF])), 50)
    assert res[2] == ERR_TRUNC
    # the stream ends before the page's rows are covered
    res, _ = run_block(v1(bytes([10 << 1, 1])), 50)
    assert res[2] == ERR_TRUNC
    # zero-length runs advance and end, they cannot spin
    res, _ = run_block(v1(bytes([0, 1] * 20)), 50)
    assert res[2] == ERR_TRUNC


def test_length_prefix_past_page_end():
    block = (1000).to_bytes(4, "little") + vi(100 << 1) + b"\x01"
    res, words = run_block(block, 100)
    assert res[2] == ERR_PAST and not words.any()
    # a page too short for the prefix itself
    res, _ = run_block(b"\x02\x00", 10)
    assert res[2] == ERR_PAST
    # v2 length from the header past the page
    res, _ = run_block(bytes([7 << 1, 1]), 7, v2len=40)
    assert res[2] == ERR_PAST


def test_level_above_one():
    res, _ = run_block(v1(vi(100 << 1) + b"\x02"), 100)
    assert res[2] == ERR_LEVEL


def test_dense_plan_refuses_errors_and_header_mismatch():
    rng = np.random.default_rng(3)
    mask = null_mask("bernoulli", 3000, rng)
    arr = make_array("i64", 3000, mask, rng)
    raw = write(arr, "2.0")
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    ch = P._Chunk(raw, md.row_group(0).column(0), 1, 0, mask=True)
    descs = P._def_descs([ch])
    good = sim_def_pages(raw, descs,
                         np.zeros(P_valid_words(3000), dtype=np.uint64))
    bad = good.copy()
    bad[0, 2] = ERR_TRUNC
    with pytest.raises(P.QkParquetError, match="truncated"):
        P._dense_plan([ch], bad)
    bad = good.copy()
    bad[0, 0] += 1                      # disagrees with the v2 header
    with pytest.raises(P.QkParquetError, match="page header"):
        P._dense_plan([ch], bad)
    assert P._dense_plan([ch], good) == int(mask.sum())


def test_default_mode_plan_still_raises():
    rng = np.random.default_rng(4)
    arr = make_array("i64", 3000, null_mask("bernoulli", 3000, rng), rng)
    for version in ("1.0", "2.0"):
        raw = write(arr, version)
        md = pq.ParquetFile(io.BytesIO(raw)).metadata
        with pytest.raises(P.QkParquetError, match="nulls"):
            P._Chunk(raw, md.row_group(0).column(0), 1, 0)
