"""CPU checks of the inputs tests/test_gpu_pq_hybrid.py feeds to
qk_pq_rle_pages / qk_pq_def_pages / qk_pq_plain_copy, and of the host
planner's refusals.

The spec decoder (tests/_pq_hybrid_cases.py) must return the emitter's
input for every valid stream and the named error for every corrupt one,
always under Guard, which asserts on any read at or past the page end.
It is anchored to an independent implementation: the index streams of
pyarrow-written dictionary pages must decode to the indices pyarrow's
own reader returns. Putting back any one behaviour of the unhardened
kernel in the decoder must make a named case fail."""
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


def decode(c, legacy=()):
    """Spec decoder over the case's descriptor, poison after the page."""
    if c.reverse:
        return C.spec_decode(C.guarded(c.stream), len(c.stream), 0, c.count,
                             c.bw, c.dict_n, legacy)
    return C.spec_decode(C.guarded(c.stream), 0, len(c.stream), c.count,
                         c.bw, c.dict_n, legacy)


def holds(c, legacy=()):
    """Does the decoder give what the case expects?"""
    try:
        got, err = decode(c, legacy)
    except AssertionError:              # Guard: read past the page end
        return False
    return err == c.err and got == c.want.tolist()


def all_valid():
    return C.rle_bitwidth_cases() + C.rle_valid_cases()


def test_case_lists_are_what_the_issue_names():
    names = [c.name for c in all_valid()]
    assert len(set(names)) == len(names)
    assert len(C.rle_bitwidth_cases()) == 64
    for bw in C.RLE_ONES_BW:
        for ln in C.RLE_ONES_LEN:
            assert "ones-bw%d-len%d" % (bw, ln) in names
    for must in ("packed-64groups-hdr2", "packed-2049groups-hdr2",
                 "packed-2049groups-hdr3", "packed-8192groups-hdr3",
                 "mixed-bw1", "mixed-bw32", "zero-runs-in-the-middle",
                 "last-rle-100-count-37",
                 "last-packed-5groups-count-33-padded",
                 "last-packed-5groups-count-33-cut", "bw0-no-stream",
                 "bw0-with-stream", "count0-no-stream", "idx_off-0",
                 "idx_off-7", "idx_off-%d" % (1 << 31)):
        assert must in names, must
    assert sum(C.MIXED_LENGTHS) == 232
    assert [(c.name, c.err) for c in C.rle_corrupt_cases()] == [
        ("varint-continues-on-last-byte", C.ERR_TRUNC),
        ("varint-11-bytes", C.ERR_TRUNC),
        ("rle-value-byte-missing-bw17", C.ERR_TRUNC),
        ("rle-value-byte-missing-bw25", C.ERR_TRUNC),
        ("packed-used-values-past-end", C.ERR_TRUNC),
        ("empty-stream", C.ERR_TRUNC),
        ("covers-10-of-50", C.ERR_TRUNC),
        ("twenty-zero-length-runs", C.ERR_TRUNC),
        ("rle-index-at-dict_n", C.ERR_INDEX),
        ("packed-index-above-dict_n", C.ERR_INDEX),
        ("out-of-range-only-in-padding", 0),
        ("bw33", C.ERR_DESC),
        ("src_off-above-src_end", C.ERR_DESC)]


def test_emitter_bytes_by_hand():
    """A few streams written out by hand from the spec, so that emitter
    and decoder cannot agree on a shared mistake."""
    # the spec's example: 0..7 at width 3 -> 0x88 0xC6 0xFA
    assert C.emit([("packed", list(range(8)), 1)], 3)[0] \
        == bytes([0x03, 0x88, 0xC6, 0xFA])
    assert C.emit([("rle", 0x1ABCD, 20_000)], 17)[0] \
        == bytes([0xC0, 0xB8, 0x02, 0xCD, 0xAB, 0x01])
    assert C.emit([("rle", 5, 3, {"hdr": 3})], 3)[0] \
        == bytes([0x86, 0x80, 0x00, 0x05])
    assert C.emit([("rle", 9, 0), ("packed", [], 0)], 4)[0] \
        == bytes([0x00, 0x09, 0x01])
    cut = C.emit([("packed", [1] * 9, 2, {"cut": True})], 3)[0]
    full = C.emit([("packed", [1] * 9, 2)], 3)[0]
    assert len(full) == 7 and cut == full[:1 + 4]
    assert C.spec_decode(C.guarded(bytes([0x03, 0x88, 0xC6, 0xFA])), 0, 4,
                         8, 3, 8) == (list(range(8)), 0)


def test_valid_streams_decode_to_the_emitter_input():
    for c in all_valid():
        assert c.err == 0
        got, err = decode(c)
        assert err == 0 and got == c.want.tolist(), c
        assert len(got) == c.count


def test_host_run_walker_agrees_on_valid_streams():
    """parquet_gpu._walk_rle, the run-level model the plan tests
    (test_parquet_cpu.py, test_parquet_nulls_cpu.py) expand pages with,
    against the emitter's input on every valid stream it can walk (it
    needs a stream for bw 0 and whole last groups)."""
    n = 0
    for c in all_valid():
        if c.bw == 0 or c.name.endswith("-cut") or not c.count:
            continue
        ents = []
        P._walk_rle(c.stream + b"\0" * 8, 0, len(c.stream), c.bw, c.count,
                    0, ents)
        got = np.empty(c.count, dtype=np.uint32)
        raw = c.stream + b"\0" * 8
        for kind, dst, m, a, b in ents:
            got[dst:dst + m] = a if kind == 0 else [
                (int.from_bytes(raw[bit >> 3:(bit >> 3) + 8], "little")
                 >> (bit & 7)) & ((1 << b) - 1)
                for bit in range(a, a + m * b, b)]
        assert got.tolist() == c.want.tolist(), c
        n += 1
    assert n >= 180


def test_corrupt_streams_give_the_named_error():
    for c in C.rle_corrupt_cases():
        got, err = decode(c)
        assert err == c.err and got == c.want.tolist(), c
    pad = next(c for c in C.rle_corrupt_cases()
               if c.name == "out-of-range-only-in-padding")
    assert pad.want.tolist() == [1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    # and the padding really holds the out-of-range pattern
    assert C.spec_decode(C.guarded(pad.stream), 0, len(pad.stream), 16, 3,
                         5)[1] == C.ERR_INDEX


# which named cases catch each behaviour of the unhardened kernel
CAUGHT_BY = {
    "unbounded_varint": {"varint-continues-on-last-byte",
                         "varint-11-bytes"},
    "no_end_check": {"rle-value-byte-missing-bw17",
                     "rle-value-byte-missing-bw25",
                     "packed-used-values-past-end"},
    "silent_exit": {"empty-stream", "covers-10-of-50",
                    "twenty-zero-length-runs"},
    "no_range_check": {"rle-index-at-dict_n", "packed-index-above-dict_n"},
}


@pytest.mark.parametrize("behaviour", C.LEGACY)
def test_each_parent_behaviour_fails_a_named_case(behaviour):
    every = all_valid() + C.rle_corrupt_cases()
    assert all(holds(c) for c in every)
    failed = {c.name for c in every if not holds(c, (behaviour,))}
    assert failed >= CAUGHT_BY[behaviour], failed
    assert failed, behaviour


# ---- anchor: pyarrow's own decode of pyarrow-written pages ---------------

CARDINALITIES = (1, 2, 3, 5, 9, 17, 33, 100, 200, 300, 1000, 1500, 3000,
                 5000, 12_000, 20_000, 40_000, 70_000, 140_000)
# every width from 1 to 18: a single-entry dictionary is written with
# width 1, not 0, and at 140,000 entries of this size pyarrow is close to
# the dictionary page limit set below, past which it writes PLAIN
WIDTHS_REACHED = set(range(1, 19))


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_spec_decoder_equals_pyarrow_indices(version):
    """Every index bit width pyarrow produces here (it falls back to
    PLAIN once the dictionary outgrows dictionary_pagesize_limit)."""
    rng = np.random.default_rng(77)
    widths = set()
    for card in CARDINALITIES:
        n = max(2000, card + card // 4)
        v = rng.integers(0, card, n)
        v[:card] = rng.permutation(card)        # every entry occurs
        raw = io.BytesIO()
        # read_dictionary hands back indices for BYTE_ARRAY columns only
        words = np.asarray(["v%07d" % i for i in range(card)], dtype=object)
        pq.write_table(pa.table({"x": pa.array(words[v], type=pa.string())}),
                       raw, compression="NONE",
                       data_page_version=version, use_dictionary=True,
                       dictionary_pagesize_limit=8 << 20,
                       data_page_size=16 << 10)
        raw = raw.getvalue()
        md = pq.ParquetFile(io.BytesIO(raw)).metadata
        assert md.num_row_groups == 1
        ch = P._Chunk(raw, md.row_group(0).column(0), 1, 0)
        assert not ch.plain_tiles and len(ch.dict_vals) == card
        got = np.empty(n, dtype=np.int64)
        for s, e, d, c, bw in ch.rle_pages:
            widths.add(bw)
            idx, err = C.spec_decode(raw, s, e, c, bw, card)
            assert err == 0
            got[d:d + c] = idx
        want = pq.read_table(io.BytesIO(raw), read_dictionary=["x"]) \
            .column("x").combine_chunks()
        assert want.dictionary.to_pylist() == ch.dict_vals
        assert np.array_equal(want.indices.to_numpy(), got), card
    assert widths == WIDTHS_REACHED, sorted(widths)


# ---- end to end: a corrupted dictionary page -----------------------------

@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_pyarrow_refuses_an_index_above_the_dictionary(version, nullable):
    """The reference behaviour the device decode must match."""
    raw, t = C.five_value_file(version, nullable)
    assert pq.read_table(io.BytesIO(raw)).equals(t)
    ch = C.locate_rle_pages(raw, nullable)
    assert len(ch.dict_vals) == 5
    s, e, d, c, bw = ch.rle_pages[0]
    assert bw == 3
    assert C.spec_decode(raw, s, e, c, bw, 5)[1] == 0
    bad = C.corrupt_first_index(raw, s, bw)
    idx, err = C.spec_decode(bad, s, e, c, bw, 5)
    assert err == C.ERR_INDEX
    with pytest.raises(Exception):
        pq.read_table(io.BytesIO(bad))


# ---- host planner refusals (default mode) --------------------------------

def test_plain_page_longer_than_its_bytes_is_refused():
    vals = np.arange(10, dtype=np.int64).tobytes()
    raw, col = C.chunk([C.data_page(10, P.ENC_PLAIN, vals)], 10)
    ch = P._Chunk(raw, col, 0, 0)
    assert int(ch.plain_tiles[0][0, 2]) == 10
    raw, col = C.chunk([C.data_page(11, P.ENC_PLAIN, vals)], 11)
    with pytest.raises(P.QkParquetError, match="PLAIN values run past"):
        P._Chunk(raw, col, 0, 0)
    # values of 4 bytes: 20 fit, 21 do not
    raw, col = C.chunk([C.data_page(20, P.ENC_PLAIN, vals)], 20, "INT32")
    P._Chunk(raw, col, 0, 0)
    raw, col = C.chunk([C.data_page(21, P.ENC_PLAIN, vals)], 21, "INT32")
    with pytest.raises(P.QkParquetError, match="PLAIN values run past"):
        P._Chunk(raw, col, 0, 0)


def test_dictionary_page_shorter_than_its_entries_is_refused():
    dvals = np.arange(4, dtype=np.int64).tobytes()
    idx = bytes([2]) + C.emit([("rle", 3, 6)], 2)[0]
    good = [C.dict_page(4, dvals), C.data_page(6, P.ENC_RLE_DICT, idx)]
    raw, col = C.chunk(good, 6, has_dict=True)
    ch = P._Chunk(raw, col, 0, 0)
    assert ch.dict_vals.tolist() == [0, 1, 2, 3]
    s, e, d, c, bw = ch.rle_pages[0]
    assert C.spec_decode(raw, s, e, c, bw, 4) == ([3] * 6, 0)
    raw, col = C.chunk([C.dict_page(5, dvals), good[1]], 6, has_dict=True)
    with pytest.raises(P.QkParquetError, match="dictionary page shorter"):
        P._Chunk(raw, col, 0, 0)
    # BYTE_ARRAY: an entry whose length runs past the page, and a page
    # that ends inside a length
    sb = b"\x02\x00\x00\x00ab" + b"\x03\x00\x00\x00cde"
    pages = [C.dict_page(2, sb), good[1]]
    raw, col = C.chunk(pages, 6, "BYTE_ARRAY", has_dict=True)
    assert P._Chunk(raw, col, 0, 0).dict_vals == ["ab", "cde"]
    for short in (sb[:-1], sb[:8], sb + b"\x01\x00"):
        n = 3 if len(short) > len(sb) else 2
        raw, col = C.chunk([C.dict_page(n, short), good[1]], 6,
                           "BYTE_ARRAY", has_dict=True)
        with pytest.raises(P.QkParquetError,
                           match="dictionary page shorter"):
            P._Chunk(raw, col, 0, 0)


def test_dictionary_data_page_without_bit_width_byte_is_refused():
    dvals = np.arange(4, dtype=np.int64).tobytes()
    pages = [C.dict_page(4, dvals), C.data_page(6, P.ENC_RLE_DICT, b"")]
    raw, col = C.chunk(pages, 6, has_dict=True)
    with pytest.raises(P.QkParquetError, match="bit-width byte"):
        P._Chunk(raw, col, 0, 0)
    # the byte is there, the stream is not: the plan passes, the kernel
    # reports the truncation (tests/test_gpu_pq_hybrid.py)
    pages[1] = C.data_page(6, P.ENC_RLE_DICT, b"\x02")
    raw, col = C.chunk(pages, 6, has_dict=True)
    s, e, d, c, bw = P._Chunk(raw, col, 0, 0).rle_pages[0]
    assert s == e and C.spec_decode(raw, s, e, c, bw, 4) == ([], C.ERR_TRUNC)


def _dict_chunk(nvalues, dict_n, count, row0=0):
    dvals = np.arange(dict_n, dtype=np.int64).tobytes()
    idx = bytes([2]) + C.emit([("rle", 1, count)], 2)[0]
    raw, col = C.chunk([C.dict_page(dict_n, dvals),
                        C.data_page(count, P.ENC_RLE_DICT, idx)], nvalues,
                       has_dict=True)
    return raw, P._Chunk(raw, col, 0, row0)


def test_rle_descriptor_carries_the_dictionary_length():
    """_rle_ents: rows are 8 wide, slot 5 rebases each chunk into the
    concatenated dictionary, slot 6 is the chunk's own dictionary length.
    Chunks lie in different files here; only the descriptor is looked
    at."""
    _, a = _dict_chunk(6, 4, 6)
    _, b = _dict_chunk(9, 3, 9, row0=6)
    ents, parts, _ = P._rle_ents([a, b])
    assert ents.shape == (2, 8) and ents.dtype == np.uint64
    sa, sb = a.rle_pages[0], b.rle_pages[0]
    assert ents[0].tolist() == [sa[0], sa[1], 0, 6, 2, 0, 4, 0]
    assert ents[1].tolist() == [sb[0], sb[1], 6, 9, 2, 4, 3, 0]
    assert [len(p) for p in parts] == [4, 3]


def test_empty_dictionary_with_values_is_refused():
    """The gather reads entry 0 for every index the kernel clamps, so a
    dictionary of no entries must not reach it."""
    _, ch = _dict_chunk(6, 0, 6)
    assert len(ch.dict_vals) == 0
    with pytest.raises(P.QkParquetError, match="empty dictionary"):
        P._rle_ents([ch])
    # no values, no descriptor, no gather
    _, ch = _dict_chunk(0, 0, 0)
    ents, parts, _ = P._rle_ents([ch])
    assert ents.shape == (0, 8) and parts == []


def test_rle_error_codes_have_messages_and_the_shim_six_arguments():
    assert set(P._RLE_ERR) == {C.ERR_TRUNC, C.ERR_INDEX, C.ERR_DESC}
    from quokka_amd import shim
    assert len(shim._SIGS["qk_pq_rle_pages"]) == 6
