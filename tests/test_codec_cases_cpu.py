"""CPU checks of the inputs that tests/test_gpu_codecs.py feeds to the
gzip and snappy page decoders: the RFC 1951 walker against zlib, the
hand-built gzip wrapper against the gzip module, the snappy emitter
against pyarrow's decoder, the levels pages against the host mirror, and
every precondition a GPU case is named for. No GPU needed."""
import gzip
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _codec_cases as C  # noqa: E402
from _deflate_walker import walk  # noqa: E402


def _check(case):
    w = C.walks()[case.name]
    assert w.data == zlib.decompress(case.raw, -15) == case.payload, case
    # the walker stopped inside the stream's last byte: nothing trails
    assert 8 * (len(case.raw) - 1) < w.end_bit <= 8 * len(case.raw), case
    return w


def test_walker_matches_zlib_on_matrix():
    walks = [_check(c) for c in C.gzip_matrix()]
    assert len(walks) == 7 * 4 * 4 * 9
    seen = {b for w in walks for b in w.blocks}
    assert seen == {"stored", "fixed", "dynamic"}


def test_walker_matches_zlib_on_special_streams():
    for case in C.gzip_special().values():
        _check(case)


def test_walker_refuses_invalid_streams():
    good = C.deflate(C.TEXT, 6, zlib.Z_DEFAULT_STRATEGY)
    stored = C.deflate(b"abcdef", 0, zlib.Z_DEFAULT_STRATEGY)
    assert walk(stored).blocks == ["stored"]
    bad_nlen = bytearray(stored)
    bad_nlen[3] ^= 1
    for bad in (good[:-1], good[:len(good) // 2], stored[:-1], b"\x07",
                bytes(bad_nlen), b"",
                C.fixed_stream([b"ab"])[:-1]):
        with pytest.raises(ValueError):
            walk(bad)
    # distance reaching before the start of the output
    w = C._BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    C._fixed_lit(w, 0x61)
    C._fixed_lit(w, 257)
    w.code(1, 5)                    # length 3, distance 2, 1 byte out
    C._fixed_lit(w, 256)
    with pytest.raises(ValueError):
        walk(w.bytes())


def test_huffman_then_stored_present():
    W = C.walks()
    hs = [c.name for c in C.gzip_matrix()
          if W[c.name].huffman_then_stored()]
    assert len(hs) >= 12
    assert C.EXAMPLE in hs
    ex = next(c for c in C.gzip_matrix() if c.name == C.EXAMPLE)
    assert ex.payload == b"the quick brown fox 64 " * 64
    assert ex.raw == C.deflate(ex.payload, 6, zlib.Z_RLE,
                               zlib.Z_FULL_FLUSH, 1471)
    assert W[ex.name].blocks[-3:-1] == ["dynamic", "stored"]
    assert W["natural-huff-stored"].huffman_then_stored()


def test_named_paths_are_reached():
    W = C.walks()
    fixed = C.fixed_block_cases()
    assert len(fixed) == 3 * 3 * 9
    assert all("fixed" in W[c.name].blocks for c in fixed)
    long_codes = C.long_code_cases()
    assert len(long_codes) == 3 * 9
    assert all(W[c.name].max_lit_bits > 10 for c in long_codes)
    w = W["fixed-maxdist"]
    assert w.blocks == ["fixed"]
    assert w.max_dist == 32768 and w.max_len == 258
    assert W["maxlen"].max_len == 258
    assert W["empty"].blocks == ["fixed"]
    assert W["empty"].data == b""
    for n in (65535, 65536, 70000):
        b = W["stored%d" % n].blocks
        assert set(b) == {"stored"} and len(b) >= (2 if n > 65535 else 1)


def test_gzip_wrapper_every_flag_combination():
    # FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16: every subset
    assert sorted(C.ALL_FLAGS) == list(range(0, 32, 2))
    cases = list(C.gzip_matrix()[::37]) + list(C.gzip_special().values())
    for i, case in enumerate(cases):
        for flags in (C.ALL_FLAGS if i < 3 else
                      (C.ALL_FLAGS[i % 16],)):
            wrapped = C.gzip_wrap(case.raw, case.payload, flags)
            assert wrapped[3] == flags
            assert gzip.decompress(wrapped) == case.payload, (case, flags)


def test_snappy_emitter_matches_pyarrow():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("snappy")
    cases = C.snappy_valid()
    for case in cases:
        got = codec.decompress(case.stream,
                               decompressed_size=len(case.expected))
        assert got.to_pybytes() == case.expected, case
    kinds = {k for case in cases for k in case.kinds}
    assert kinds == {"lit0", "lit1", "lit2", "lit3", "lit4", "copy1",
                     "copy2", "copy4"}
    # preamble lengths of 1, 2 and 3 bytes all occur
    assert {len(C.varint(len(case.expected))) for case in cases} \
        == {1, 2, 3}


def test_levels_cases_match_host_mirror():
    from quokka_amd import parquet_gpu as P
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("snappy")
    names = set()
    for case in C.levels_cases():
        names.add(case.name)
        stream = C.literal_only(case.page)
        assert codec.decompress(
            stream, decompressed_size=len(case.page)).to_pybytes() \
            == case.page
        try:
            end = P._check_levels_v1(case.page, 0, case.num_values, 1,
                                     len(case.page))
            err = 0
        except P.QkParquetError as e:
            err = 3 if "nulls" in str(e) else 1
            end = None
        assert err == case.err, case
        if end is not None:
            assert end == case.data_off, case
    assert len(names) == len(C.levels_cases())
