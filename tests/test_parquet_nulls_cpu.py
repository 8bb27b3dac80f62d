"""CPU tests of the mask-mode Parquet decode PLAN (nulls="mask"): numpy
simulators of qk_pq_def_pages and qk_valid_expand run over the real plan
(_Chunk(mask=True) -> _def_descs -> _dense_plan) and the result is
compared with pyarrow's decode of the same file: values where valid, and
the is_valid() mask. Hand-built level blocks check that a corrupt stream
ends in an error code and never reads past its page; the blocks live in
tests/_pq_hybrid_cases.py and tests/test_gpu_pq_hybrid.py runs the same
bytes through the kernel."""
import io
import os
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

from quokka_amd import parquet_gpu as P  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pq_hybrid_cases as C  # noqa: E402
from _pq_hybrid_cases import sim_def_pages  # noqa: E402

ERR_PAST, ERR_TRUNC, ERR_LEVEL = C.DEF_PAST, C.DEF_TRUNC, C.DEF_LEVEL
assert C.V1 == P._V1


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
    src = C.Guard(block + b"\xAA" * 64)
    src.limit = page_len
    words = np.zeros(P_valid_words(nrows), dtype=np.uint64)
    desc = [(0, page_len, P._V1 if v2len is None else v2len, 0, nrows, 0)]
    res = sim_def_pages(src, desc, words)[0]
    return res, words


def run_cases(err):
    """Every block of the shared def_pages list (tests/_pq_hybrid_cases.py;
    tests/test_gpu_pq_hybrid.py runs the same bytes through the kernel)
    that must end in `err`, with everything the case pins asserted."""
    cases = [c for c in C.def_cases() if c.err == err]
    for c in cases:
        res, words = run_block(c.block, c.nrows, c.v2len, c.page_len)
        assert res[2] == c.err, c
        if c.res3 is not None:
            assert res.tolist()[:3] == c.res3, c
        if c.words is not None:
            assert [int(w) for w in words[:len(c.words)]] == c.words, c
            assert not words[len(c.words):].any(), c
        if c.clean:
            assert not words.any(), c
    return [c.name for c in cases]


def test_good_blocks():
    names = run_cases(0)
    assert {"rle-100-ones", "packed-2-groups-13-rows",
            "v2-no-prefix"} <= set(names)


def test_truncated_run_header():
    assert run_cases(ERR_TRUNC) == [
        "varint-continues-on-last-byte", "rle-without-value-byte",
        "packed-groups-past-block", "covers-10-of-50",
        "twenty-zero-length-runs", "covers-150-of-200"]


def test_length_prefix_past_page_end():
    assert run_cases(ERR_PAST) == [
        "prefix-past-page", "page-shorter-than-prefix",
        "v2-length-past-page"]


def test_level_above_one():
    assert run_cases(ERR_LEVEL) == ["level-2"]


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
