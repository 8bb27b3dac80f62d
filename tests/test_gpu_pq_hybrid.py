"""Direct tests of the three Parquet value decoders, qk_pq_rle_pages,
qk_pq_def_pages and qk_pq_plain_copy, with hand-built descriptor tables
(the way parquet_gpu._decode_column / _decode_masked drive them) instead
of whole Parquet files.

pyarrow has one writer and emits a narrow slice of the hybrid encoding,
so every stream here is built for a named shape by the emitter of
tests/_pq_hybrid_cases.py. A valid page must decode to the indices its
layout was built from; a corrupt one must report the error the spec
decoder reports. tests/test_pq_hybrid_cases_cpu.py checks the same bytes
without a GPU.

One launch carries many pages. Source offsets cover all eight byte
alignments, destinations are pre-filled with a sentinel and separated by
guard words that must survive, and every page that must be refused sits
between two good pages that must still decode. The bytes after each page
are guard bytes below 0x80 (none can continue a varint), at least
4 * count + 16 of them, so a decoder that over-reads gives a wrong
answer, not an access outside the allocation. Every launch runs twice
with two guard fills; out, err_dev and the sentinels must not differ.
"""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pq_hybrid_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEF                       # out[] before the launch
FILLS = (0x55, 0x2B)                    # guard bytes of the two launches
NGUARD = 4                              # u32 guard words after each slice


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


class Dev:
    """Device copies of host arrays, freed together."""

    def __init__(self, shim):
        self.shim, self.bufs = shim, []

    def up(self, arr):
        from quokka_amd.shim import DevBuffer, c_u64, c_vp
        arr = np.ascontiguousarray(arr)
        b = DevBuffer(arr.nbytes)
        self.bufs.append(b)
        if arr.nbytes:
            self.shim.call("qk_h2d", b.ptr, arr.ctypes.data_as(c_vp),
                           c_u64(arr.nbytes))
        return b

    def down(self, buf, like):
        from quokka_amd.shim import c_u64, c_vp
        out = np.empty_like(like)
        if out.nbytes:
            self.shim.call("qk_d2h", out.ctypes.data_as(c_vp), buf.ptr,
                           c_u64(out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


# ---- qk_pq_rle_pages -----------------------------------------------------

def rle_launch(shim, src, ents, nout):
    """One launch over (src bytes, ents n x 8) -> (out u32[nout], err)."""
    from quokka_amd.shim import c_u64
    out0 = np.full(nout, SENT, dtype=np.uint32)
    err0 = np.full(len(ents), -7, dtype=np.int64)
    with Dev(shim) as d:
        d_src, d_ent = d.up(src), d.up(ents)
        d_out, d_err = d.up(out0), d.up(err0)
        shim.call("qk_pq_rle_pages", None, c_u64(len(ents)), d_ent.ptr,
                  d_src.ptr, d_out.ptr, d_err.ptr)
        shim.call("qk_stream_sync", None)
        return d.down(d_out, out0), d.down(d_err, err0)


def rle_twice(shim, build):
    """build(fill) -> (src, ents, nout). Runs it with both guard fills;
    what the kernel wrote must not depend on the fill."""
    runs = [rle_launch(shim, *build(f)) for f in FILLS]
    assert np.array_equal(runs[0][1], runs[1][1]), \
        "err_dev depends on bytes past src_end"
    diff = np.nonzero(runs[0][0] != runs[1][0])[0]
    assert diff.size == 0, \
        "out depends on bytes past src_end at %s" % diff[:8].tolist()
    return runs[0]


def lay_out(pages, fill):
    """pages: [(RleCase, source alignment 0..7)] -> (src, ents, nout,
    [dst_off per page])."""
    src = bytearray([fill] * 3)
    ents, dsts = [], []
    dst = 1
    for c, align in pages:
        src += bytes([fill]) * ((align - len(src)) % 8)
        assert len(src) % 8 == align
        s = len(src)
        src += c.stream
        e = len(src)
        src += bytes([fill]) * (4 * c.count + 16)
        if c.reverse:
            s, e = e, s
        ents.append((s, e, dst, c.count, c.bw, c.idx_off, c.dict_n, 0))
        dsts.append(dst)
        dst += c.count + NGUARD
    return (np.frombuffer(bytes(src), dtype=np.uint8),
            np.asarray(ents, dtype=np.uint64).reshape(-1, 8), dst, dsts)


def check_rle(shim, pages):
    """Decode all pages in one launch (twice) and compare every page with
    its case: err, the indices written, sentinels everywhere else."""
    laid = {f: lay_out(pages, f) for f in FILLS}
    out, err = rle_twice(shim, lambda f: laid[f][:3])
    dsts = laid[FILLS[0]][3]
    want = np.full(len(out), SENT, dtype=np.uint32)
    for (c, _), d in zip(pages, dsts):
        want[d:d + len(c.want)] = c.want + np.uint32(c.idx_off)
        if len(c.want):
            lo, hi = c.idx_off, c.idx_off + max(c.dict_n, 1)
            got = out[d:d + len(c.want)].astype(np.int64)
            assert ((got >= lo) & (got < hi)).all(), c
    bad = [(c.name, a, int(err[i]), c.err) for i, (c, a) in enumerate(pages)
           if err[i] != c.err]
    assert not bad, "err_dev (name, align, got, want): %s" % bad[:6]
    wrong = np.nonzero(out != want)[0]
    if wrong.size:
        i = int(np.searchsorted(dsts, wrong[0], side="right")) - 1
        raise AssertionError(
            "%d words wrong, first at %d (page %d %r align %d): got %#x "
            "want %#x" % (wrong.size, wrong[0], i, pages[i][0], pages[i][1],
                          out[wrong[0]], want[wrong[0]]))


def test_rle_every_bit_width_at_every_alignment(gpu):
    """bw 1..32, one packed run of 3 groups, count 24 and 17, values 0,
    2**bw - 1, 0x55.. and 0xAA.., source alignment 0..7: the 8-byte
    unaligned load at every bit offset, up to bit 7 + 32 bits."""
    check_rle(gpu, [(c, a) for c in C.rle_bitwidth_cases()
                    for a in range(8)])


def test_rle_valid_run_shapes(gpu):
    """All-ones RLE runs of 1..20,000 at the widths around each value
    byte count, packed runs with 2- and 3-byte headers, mixed layouts
    with run boundaries at many lane offsets, zero-length runs, a last
    run longer than the page, a last group with and without its padding
    bytes, bw 0, count 0, idx_off up to 2**31."""
    cases = C.rle_valid_cases()
    check_rle(gpu, [(c, i % 8) for i, c in enumerate(cases)])
    # and shifted, so that each case meets another alignment
    check_rle(gpu, [(c, (i + 3) % 8) for i, c in enumerate(cases)])


def test_rle_corrupt_pages_between_good_ones(gpu):
    good = [c for c in C.rle_valid_cases() if c.name.startswith("mixed")]
    for shift in (0, 5):
        pages = []
        for i, c in enumerate(C.rle_corrupt_cases()):
            pages.append((good[i % len(good)], (2 * i + shift) % 8))
            pages.append((c, (i + shift) % 8))
        pages.append((good[0], 7))
        check_rle(gpu, pages)


def test_rle_70001_pages_grid_stride(gpu):
    """More pages than the 65,536-block grid cap. Even pages hold one RLE
    run, odd pages one packed run of 2 groups at width 4; 1..9 values
    are used of either."""
    n, stride = 70_001, 73               # 73 = 1 mod 8: every alignment
    rng = np.random.default_rng(70001)
    cnt = rng.integers(1, 10, n).astype(np.uint64)
    off = (3 + stride * np.arange(n)).astype(np.uint64)
    odd = (np.arange(n) & 1).astype(bool)
    body = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    hdr = np.where(odd, 5, cnt << np.uint64(1)).astype(np.uint8)
    end = off + np.where(odd, 9, 2).astype(np.uint64)
    dst = np.concatenate([np.zeros(1, dtype=np.uint64),
                          np.cumsum(cnt + np.uint64(NGUARD))[:-1]]) \
        + np.uint64(1)
    nout = int(dst[-1] + cnt[-1]) + NGUARD
    ents = np.zeros((n, 8), dtype=np.uint64)
    ents[:, 0], ents[:, 1], ents[:, 2], ents[:, 3] = off, end, dst, cnt
    ents[:, 4] = np.where(odd, 4, 8)
    ents[:, 5] = 1000
    ents[:, 6] = np.where(odd, 16, 256)
    assert stride - 9 >= 4 * 9 + 16

    def build(fill):
        src = np.full(3 + stride * n + 8, fill, dtype=np.uint8)
        io_ = off.astype(np.int64)
        src[io_] = hdr
        for k in range(8):               # packed pages: 8 bytes, RLE: 1
            sel = odd if k else np.ones(n, dtype=bool)
            src[io_[sel] + 1 + k] = body[sel, k]
        return src, ents, nout

    out, err = rle_twice(gpu, build)
    assert not err.any(), np.nonzero(err)[0][:8]
    # expected, straight from the bytes laid down: nibbles, low first
    nib = np.empty((n, 16), dtype=np.uint32)
    nib[:, 0::2], nib[:, 1::2] = body & 15, body >> 4
    vals = np.where(odd[:, None], nib[:, :9], body[:, :1].astype(np.uint32))
    want = np.full(nout, SENT, dtype=np.uint32)
    for k in range(9):
        sel = cnt > k
        want[dst[sel].astype(np.int64) + k] = vals[sel, k] + 1000
    assert np.array_equal(out, want)


# ---- qk_pq_def_pages -----------------------------------------------------

def def_check(shim, src_of, descs, nrows_total, err_pages=()):
    """Launch (twice) and compare every bitmap word and the npages x 4
    table with sim_def_pages. A page that ends in an error keeps the
    words its runs completed and gives up the one it was gathering; the
    simulator models that with drop_partial, so erroring pages are
    compared bit for bit too."""
    from quokka_amd.shim import c_u64
    descs = np.asarray(descs, dtype=np.uint64).reshape(-1, 6)
    nw = C.valid_words(nrows_total)
    runs = []
    for f in FILLS:
        src = src_of(f)
        words0 = np.zeros(nw, dtype=np.uint64)
        tab0 = np.full((len(descs), 4), -7, dtype=np.int64)
        with Dev(shim) as d:
            d_src, d_desc = d.up(src), d.up(descs)
            d_w, d_t = d.up(words0), d.up(tab0)
            shim.call("qk_pq_def_pages", None, c_u64(len(descs)),
                      d_desc.ptr, d_src.ptr, d_w.ptr, d_t.ptr)
            shim.call("qk_stream_sync", None)
            runs.append((d.down(d_w, words0), d.down(d_t, tab0)))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1])
    words, tab = runs[0]
    sim_words = np.zeros(nw, dtype=np.uint64)
    sim_tab = C.sim_def_pages(src_of(FILLS[0]).tobytes(), descs, sim_words,
                              drop_partial=True)
    assert np.array_equal(tab, sim_tab), \
        np.nonzero((tab != sim_tab).any(axis=1))[0][:8]
    assert sorted(np.nonzero(tab[:, 2])[0].tolist()) == sorted(err_pages)
    got = np.unpackbits(words.view(np.uint8), bitorder="little")
    want = np.unpackbits(sim_words.view(np.uint8), bitorder="little")
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "bitmap differs at rows %s" % bad[:8].tolist()
    assert not got[nrows_total:].any()      # bits at or above n stay 0
    return words, tab


def framings(c):
    """The case's block as (block, v2len or None) in v1 and v2 framing."""
    if c.v2len is None:
        out = [(c.block, None, c.page_len)]
        if len(c.block) >= 4 and c.page_len == len(c.block):
            ln = int.from_bytes(c.block[:4], "little")
            out.append((c.block[4:], ln, c.page_len - 4))
        return out
    return [(c.block, c.v2len, c.page_len),
            (c.v2len.to_bytes(4, "little") + c.block, None, c.page_len + 4)]


def test_def_shared_case_list_v1_and_v2(gpu):
    """Every block of the shared list, good and corrupt, in v1 and v2
    framing, at first rows that are no multiple of 64."""
    pages = []
    for c in C.def_cases():
        for block, v2len, page_len in framings(c):
            pages.append((c, block, v2len, page_len))
    laid = {}
    for f in FILLS:
        src = bytearray([f] * 5)
        descs, row, errs = [], 37, []
        for i, (c, block, v2len, page_len) in enumerate(pages):
            off = len(src)
            src += block + bytes([f]) * 24
            descs.append((off, off + page_len, C.V1 if v2len is None
                          else v2len, row, c.nrows, 0))
            assert row % 64
            if c.err:
                errs.append(i)
            row += c.nrows + (3 if (row + c.nrows + 3) % 64 else 4)
        laid[f] = (np.frombuffer(bytes(src), dtype=np.uint8), descs, row,
                   errs)
    _, descs, total, errs = laid[FILLS[0]]
    assert len(errs) >= 15
    words, tab = def_check(gpu, lambda f: laid[f][0], descs, total, errs)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    for i, (c, *_r) in enumerate(pages):
        assert tab[i, 2] == c.err, (c, i)
        if c.clean:                     # refused before any bit is set
            r0 = int(descs[i][3])
            assert not bits[r0:r0 + c.nrows].any(), c


def _packed_levels(bits):
    pad = list(bits) + [1] * (-len(bits) % 8)       # padding ones: ignored
    body = np.packbits(np.asarray(pad, dtype=np.uint8), bitorder="little")
    return C.varint(((len(pad) // 8) << 1) | 1) + body.tobytes()


def test_def_pages_inside_and_on_word_edges(gpu):
    """Pages that start and end inside one word (three and more per
    word), a page of exactly 64 rows on a word boundary, a page whose
    last row is bit 63, v1 and v2 mixed."""
    spans = [(0, 7), (7, 1), (8, 30), (38, 2), (40, 24),      # word 0, full
             (64, 64),                                        # exactly word 1
             (130, 5), (135, 3), (138, 20), (170, 9),         # inside word 2
             (250, 6),                                        # ends on bit 63
             (256, 1), (257, 62), (319, 1), (320, 130)]
    laid = {}
    for f in FILLS:
        rng = np.random.default_rng(64)
        src = bytearray([f] * 3)
        descs = []
        for i, (row, n) in enumerate(spans):
            bits = rng.integers(0, 2, n)
            bits[-1] = 1
            lv = _packed_levels(bits) if i % 3 else \
                C.varint(n << 1) + b"\x01"
            off = len(src)
            if i % 2:
                src += C.v1(lv)
                descs.append((off, off + 4 + len(lv), C.V1, row, n, 0))
            else:
                src += lv
                descs.append((off, off + len(lv), len(lv), row, n, 0))
            src += bytes([f]) * 16
        laid[f] = np.frombuffer(bytes(src), dtype=np.uint8)
    words, _ = def_check(gpu, lambda f: laid[f], descs, 450)
    assert int(words[3]) >> 63 == 1


def test_def_70001_pages_end_to_end_rows(gpu):
    """70,001 pages of 1..9 rows laid end to end: words shared by up to
    64 pages, and more pages than the grid cap. Even pages are one RLE
    run, odd pages one packed run of 2 groups; v2 framing."""
    n, stride = 70_001, 24
    rng = np.random.default_rng(70002)
    cnt = rng.integers(1, 10, n).astype(np.uint64)
    odd = (np.arange(n) & 1).astype(bool)
    off = (3 + stride * np.arange(n)).astype(np.uint64)
    row = np.concatenate([np.zeros(1, dtype=np.uint64),
                          np.cumsum(cnt)[:-1]])
    b0 = np.where(odd, 5, cnt << np.uint64(1)).astype(np.uint8)
    b1 = np.where(odd, rng.integers(0, 256, n), rng.integers(0, 2, n)) \
        .astype(np.uint8)
    b2 = rng.integers(0, 256, n).astype(np.uint8)
    ln = np.where(odd, 3, 2).astype(np.uint64)
    descs = np.zeros((n, 6), dtype=np.uint64)
    descs[:, 0], descs[:, 1], descs[:, 2] = off, off + ln, ln
    descs[:, 3], descs[:, 4] = row, cnt

    def src_of(fill):
        src = np.full(3 + stride * n + 8, fill, dtype=np.uint8)
        io_ = off.astype(np.int64)
        src[io_], src[io_ + 1] = b0, b1
        src[io_[odd] + 2] = b2[odd]
        return src

    total = int(cnt.sum())
    _, tab = def_check(gpu, src_of, descs, total)
    assert not tab[:, 2].any() and (tab[:, 3] == -1).all()


# ---- qk_pq_plain_copy ----------------------------------------------------

@pytest.mark.parametrize("es,tiles", C.plain_cases(),
                         ids=["es%d" % e for e in C.PLAIN_ELEM_SIZES])
def test_plain_copy(gpu, es, tiles):
    """Tile counts 0..8192 at source byte offsets 0..7, guard elements
    between the destination tiles, against numpy.frombuffer."""
    import ctypes
    from quokka_amd.shim import c_u64
    rng = np.random.default_rng(es)
    dt = np.dtype("u%d" % es)
    src = bytearray(b"\x99" * 3)
    table, dst = [], 1
    for align, cnt in tiles:
        src += b"\x99" * ((align - len(src)) % 8)
        table.append((len(src), dst, cnt))
        src += rng.integers(0, 256, cnt * es, dtype=np.uint8).tobytes()
        src += b"\x99" * 5
        dst += cnt + 3
    assert {t[0] % 8 for t in table} == set(range(8))
    raw = bytes(src)
    sent = np.frombuffer(b"\xEE" * 8, dtype=dt)[0]
    before = np.full(dst, sent, dtype=dt)
    want = before.copy()
    for s, d, cnt in table:
        want[d:d + cnt] = np.frombuffer(raw, dtype=dt, count=cnt, offset=s)
    with Dev(gpu) as d:
        d_src = d.up(np.frombuffer(raw, dtype=np.uint8))
        d_tab = d.up(np.asarray(table, dtype=np.uint64))
        d_dst = d.up(before)
        gpu.call("qk_pq_plain_copy", None, c_u64(len(table)), d_tab.ptr,
                 d_src.ptr, d_dst.ptr, ctypes.c_uint32(es))
        gpu.call("qk_stream_sync", None)
        got = d.down(d_dst, before)
    assert np.array_equal(got, want)


def test_plain_copy_refuses_element_size_3(gpu):
    import ctypes
    from quokka_amd.shim import QkError, c_u64
    with Dev(gpu) as d:
        d_src = d.up(np.zeros(64, dtype=np.uint8))
        d_tab = d.up(np.asarray([(0, 0, 4)], dtype=np.uint64))
        d_dst = d.up(np.zeros(64, dtype=np.uint8))
        with pytest.raises(QkError):
            gpu.call("qk_pq_plain_copy", None, c_u64(1), d_tab.ptr,
                     d_src.ptr, d_dst.ptr, ctypes.c_uint32(3))


# ---- end to end on the device --------------------------------------------

def track_buffers(monkeypatch):
    """Every DevBuffer made from here on, held so that none is released
    by garbage collection: what is still allocated afterwards leaked."""
    from quokka_amd import shim
    made = []
    init = shim.DevBuffer.__init__

    def tracking_init(self, nbytes):
        init(self, nbytes)
        made.append(self)

    monkeypatch.setattr(shim.DevBuffer, "__init__", tracking_init)
    return made


def _free(cols):
    for c in cols.values():
        (c[0] if isinstance(c, tuple) else c).free()


@pytest.mark.parametrize("nulls", ["raise", "mask"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_corrupted_dictionary_index_raises(gpu, monkeypatch, version, nulls):
    """The 5-value file of tests/test_pq_hybrid_cases_cpu.py with its
    first index overwritten to 7: read_table raises where pyarrow raises
    (asserted there), in default mode and in mask mode on a nullable
    copy, and frees every device buffer it took. The uncorrupted file
    still decodes equal to pyarrow. Compressed variants are not needed:
    they decode through the same kernel from scratch memory."""
    import pyarrow.parquet as pq
    from quokka_amd import parquet_gpu as P
    mask = nulls == "mask"
    raw, t = C.five_value_file(version, nullable=mask)
    want = pq.read_table(io.BytesIO(raw)).column("x").combine_chunks()
    cols = P.read_table(raw, nulls=nulls)
    try:
        col = cols["x"]
        got = col.to_numpy() if mask else col.to_numpy(col.n)
        wv = want.fill_null(0).to_numpy(zero_copy_only=False)
        np.testing.assert_array_equal(got, wv)
        if mask:
            assert col.null_count == want.null_count > 0
    finally:
        _free(cols)
    s, e, d, c, bw = C.locate_rle_pages(raw, mask).rle_pages[0]
    bad = C.corrupt_first_index(raw, s, bw)

    made = track_buffers(monkeypatch)
    with pytest.raises(P.QkParquetError, match="dictionary length"):
        P.read_table(bad, nulls=nulls)
    monkeypatch.undo()
    assert made
    left = [b.nbytes for b in made if b.ptr is not None]
    assert not left, "device buffers still allocated: %s" % left


def test_snappy_planner_refusal_frees_the_scratch(gpu, monkeypatch):
    """The planner of the decompress path (_snappy_column; a page a writer
    left uncompressed is byte-copied into the same scratch buffer) refuses
    a PLAIN page whose values run past the page, and gives the scratch
    buffer back when it does."""
    from quokka_amd import parquet_gpu as P
    vals = np.arange(10, dtype=np.int64).tobytes()
    for nv, ok in ((10, True), (11, False)):
        raw, col = C.chunk([C.data_page(nv, P.ENC_PLAIN, vals)], nv)
        dev_file = P._upload(gpu, raw)
        made = track_buffers(monkeypatch)
        try:
            if ok:
                chunks, scratch = P._snappy_column(gpu, raw, dev_file, [col],
                                                   0, 0)
                out = P._decode_column(gpu, scratch, chunks, nv)
                got = out.to_numpy(nv)
                out.free()
                scratch.free()
                assert got.tolist() == list(range(10))
            else:
                with pytest.raises(P.QkParquetError,
                                   match="PLAIN values run past"):
                    P._snappy_column(gpu, raw, dev_file, [col], 0, 0)
        finally:
            monkeypatch.undo()
            dev_file.free()
        left = [b.nbytes for b in made if b.ptr is not None]
        assert made and not left, left


def test_truncated_index_stream_raises(gpu):
    """A hand-written chunk whose data page holds the bit-width byte and
    nothing else: the plan passes, the kernel reports the truncation,
    _decode_column raises instead of returning dictionary entry 0."""
    from quokka_amd import parquet_gpu as P
    dvals = np.arange(4, dtype=np.int64).tobytes()
    pages = [C.dict_page(4, dvals), C.data_page(6, P.ENC_RLE_DICT, b"\x02")]
    raw, col = C.chunk(pages, 6, has_dict=True)
    ch = P._Chunk(raw, col, 0, 0)
    dev_file = P._upload(gpu, raw)
    try:
        with pytest.raises(P.QkParquetError, match="truncated"):
            P._decode_column(gpu, dev_file, [ch], 6)
    finally:
        dev_file.free()
