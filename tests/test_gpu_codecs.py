"""Direct tests of the two page decompressors, qk_gzip_pages and
qk_snappy_pages, with hand-built descriptor tables (the way
parquet_gpu._snappy_column drives them) instead of whole Parquet files.

pyarrow's writers use one zlib level and one snappy encoder, so files
reach only part of either format. Here every stream is built for a
named path (tests/_codec_cases.py), each case first asserts from the
RFC 1951 walker (tests/_deflate_walker.py) that its input really takes
that path, and the kernel's bytes are compared exactly with zlib /
pyarrow / the bytes the emitter built. tests/test_codec_cases_cpu.py
checks the same inputs without a GPU.

One launch carries many pages. Source and destination offsets are odd,
every destination slice is followed by 16 guard bytes that must survive,
and every page the decoder must refuse sits between two good pages that
must still decode.
"""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _codec_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = bytes(range(0xB0, 0xC0))        # 16 bytes, no two alike
SENTINEL = -7                           # out[] before the launch


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


class Page:
    """One descriptor: blob goes into the source buffer, the kernel is
    told about its first src_len bytes only."""

    def __init__(self, blob, ulen, mode=0, num_values=0, src_len=None):
        self.blob = bytes(blob)
        self.src_len = len(self.blob) if src_len is None else src_len
        self.ulen = ulen
        self.mode = mode
        self.num_values = num_values


def launch(shim, fn, pages):
    """Run `fn` over pages. Returns (out[n, 4] int64, [bytes per page]);
    asserts that no byte outside the destination slices changed."""
    from quokka_amd.shim import DevBuffer, c_u64, c_vp
    src = bytearray(b"\x99" * 3)
    descs, slices = [], []
    dst_off = 1
    for pg in pages:
        if len(src) % 2 == 0:
            src += b"\x99"                      # odd source offset
        descs.append((len(src), pg.src_len, dst_off, pg.ulen, pg.mode,
                      pg.num_values, 0, 0))
        src += pg.blob + b"\x99" * 5
        slices.append((dst_off, pg.ulen))
        dst_off += pg.ulen + len(GUARD)
        dst_off += 1 - (dst_off & 1)            # odd destination offset
    src += b"\x99" * 8                          # slack after the last page
    ndst = dst_off + len(GUARD)
    before = np.frombuffer((GUARD * (ndst // 16 + 1))[:ndst],
                           dtype=np.uint8).copy()
    h_src = np.frombuffer(bytes(src), dtype=np.uint8)
    h_desc = np.asarray(descs, dtype=np.uint64)
    h_out = np.full(len(pages) * 4, SENTINEL, dtype=np.int64)
    bufs = []

    def up(arr):
        b = DevBuffer(arr.nbytes)
        bufs.append(b)
        shim.call("qk_h2d", b.ptr, arr.ctypes.data_as(c_vp),
                  c_u64(arr.nbytes))
        return b

    try:
        d_src, d_dst = up(h_src), up(before)
        d_desc, d_out = up(h_desc), up(h_out)
        shim.call(fn, None, c_u64(len(pages)), d_desc.ptr, d_src.ptr,
                  d_dst.ptr, d_out.ptr)
        shim.call("qk_stream_sync", None)
        after = np.empty_like(before)
        shim.call("qk_d2h", after.ctypes.data_as(c_vp), d_dst.ptr,
                  c_u64(after.nbytes))
        shim.call("qk_d2h", h_out.ctypes.data_as(c_vp), d_out.ptr,
                  c_u64(h_out.nbytes))
    finally:
        for b in bufs:
            b.free()
    outside = np.ones(ndst, dtype=bool)
    for off, ln in slices:
        outside[off:off + ln] = False
    hit = np.nonzero(outside & (after != before))[0]
    assert hit.size == 0, "bytes outside the slices written at %s" \
        % hit[:8].tolist()
    got = [after[off:off + ln].tobytes() for off, ln in slices]
    return h_out.reshape(-1, 4), got


def gz_page(case, mode, flags=0):
    if mode == 0:
        return Page(case.raw, len(case.payload), 0)
    wrapped = C.gzip_wrap(case.raw, case.payload, flags)
    assert gzip.decompress(wrapped) == case.payload, case
    return Page(wrapped, len(case.payload), 1)


def check_gzip(shim, cases, mode, flags=None):
    """Decode every case in one launch; bit-exact against zlib."""
    pages = [gz_page(c, mode, C.ALL_FLAGS[i % 16] if flags is None
                     else flags[i]) for i, c in enumerate(cases)]
    for c in cases:
        assert zlib.decompress(c.raw, -15) == c.payload, c
    out, got = launch(shim, "qk_gzip_pages", pages)
    bad = [(c.name, out[i].tolist()) for i, c in enumerate(cases)
           if got[i] != c.payload or out[i].tolist() !=
           [len(c.payload), 0, c.payload[0] if c.payload else -1, 0]]
    assert not bad, "%d of %d pages wrong (mode %d): %s; first: %s" % (
        len(bad), len(cases), mode, " ".join(n for n, _ in bad), bad[:4])


MODES = pytest.mark.parametrize("mode", [0, 1], ids=["raw", "gzip"])


@MODES
def test_gzip_matrix(gpu, mode):
    """levels 0/1/6/9 x default/Z_FIXED/Z_RLE/Z_HUFFMAN_ONLY x no flush or
    a full/sync flush at byte 1, the middle, len-1 and len, over seven
    payload families; in gzip mode the header flag combinations cycle."""
    W = C.walks()
    cases = C.gzip_matrix()
    hs = [c.name for c in cases if W[c.name].huffman_then_stored()]
    assert len(hs) >= 12 and C.EXAMPLE in hs
    assert {b for c in cases for b in W[c.name].blocks} \
        == {"stored", "fixed", "dynamic"}
    check_gzip(gpu, cases, mode)


@MODES
def test_gzip_flushed_example(gpu, mode):
    """(b"the quick brown fox 64 " * 64), level 6, Z_RLE, full flush after
    1471 of its 1472 bytes: a Huffman block whose end-of-block code is
    short, then
    the flush's empty stored block. The 10-bit table lookup has fetched a
    whole byte past the block header by then; LEN/NLEN must still be
    read from the right place."""
    ex = next(c for c in C.gzip_matrix() if c.name == C.EXAMPLE)
    w = C.walks()[ex.name]
    assert w.huffman_then_stored() and w.data == ex.payload
    check_gzip(gpu, [ex], mode, flags=[0])


@MODES
def test_gzip_huffman_then_stored(gpu, mode):
    """Every matrix stream where a stored block follows a Huffman block,
    and the unflushed one (text, then bytes zlib chooses to store)."""
    W = C.walks()
    cases = [c for c in C.gzip_matrix() if W[c.name].huffman_then_stored()]
    cases.append(C.gzip_special()["natural-huff-stored"])
    assert len(cases) >= 13
    assert all(W[c.name].huffman_then_stored() for c in cases)
    check_gzip(gpu, cases, mode)


@MODES
def test_gzip_fixed_blocks(gpu, mode):
    W = C.walks()
    cases = C.fixed_block_cases()
    assert cases and all("fixed" in W[c.name].blocks for c in cases)
    check_gzip(gpu, cases, mode)


@MODES
def test_gzip_codes_longer_than_lut(gpu, mode):
    """Literal codes longer than the decoder's 10-bit table."""
    W = C.walks()
    cases = C.long_code_cases()
    assert cases and all(W[c.name].max_lit_bits > 10 for c in cases)
    check_gzip(gpu, cases, mode)


@MODES
def test_gzip_max_distance_and_length(gpu, mode):
    W = C.walks()
    S = C.gzip_special()
    w = W["fixed-maxdist"]
    assert w.blocks == ["fixed"]
    assert w.max_dist == 32768 and w.max_len == 258
    assert W["maxlen"].max_len == 258
    cases = [S["fixed-maxdist"], S["maxlen"], S["dist32k-L1"],
             S["dist32k-L6"], S["dist32k-L9"]]
    check_gzip(gpu, cases, mode)


@MODES
@pytest.mark.parametrize("n", [65535, 65536, 70000])
def test_gzip_stored_block_splitting(gpu, mode, n):
    case = C.gzip_special()["stored%d" % n]
    b = C.walks()[case.name].blocks
    assert set(b) == {"stored"} and len(b) >= (2 if n > 65535 else 1)
    check_gzip(gpu, [case], mode)


@MODES
def test_gzip_empty_stream(gpu, mode):
    case = C.gzip_special()["empty"]
    assert C.walks()["empty"].data == b"" and case.payload == b""
    # between two non-empty pages: a zero-length slice shares its offset
    # with the guard bytes that follow it
    text = next(c for c in C.gzip_matrix() if c.name == "text-L6-default")
    check_gzip(gpu, [text, case, text], mode)


def test_gzip_every_header_flag_combination(gpu):
    """FEXTRA (with zero bytes inside), FNAME, FCOMMENT, FHCRC: all 16
    subsets, on a dynamic, a flushed and a stored stream."""
    by = {c.name: c for c in C.gzip_matrix()}
    cases, flags = [], []
    for name in ("text-L6-default", C.EXAMPLE, "random-L0-default"):
        for f in C.ALL_FLAGS:
            cases.append(by[name])
            flags.append(f)
    check_gzip(gpu, cases, 1, flags=flags)


def _neighbours():
    by = {c.name: c for c in C.gzip_matrix()}
    return by["text-L9-default"], by["const-L1-fixed"]


@pytest.mark.parametrize("bad", C.gzip_refused(), ids=lambda r: r.name)
def test_gzip_refused(gpu, bad):
    """The bad page sits between two good ones: it reports its code,
    writes nothing past its slice, and both neighbours decode."""
    a, b = _neighbours()
    pages = [gz_page(a, 0),
             Page(bad.blob, bad.ulen, bad.mode, src_len=bad.src_len),
             gz_page(b, 1, C.FEXTRA | C.FCOMMENT)]
    out, got = launch(gpu, "qk_gzip_pages", pages)
    assert out[1].tolist()[:2] == [0, bad.err], (bad, out[1].tolist())
    assert got[0] == a.payload and got[2] == b.payload
    assert out[0].tolist() == [len(a.payload), 0, a.payload[0], 0]
    assert out[2].tolist() == [len(b.payload), 0, b.payload[0], 0]


# ---- snappy ---------------------------------------------------------------

def check_snappy(shim, streams, expected, names):
    import pyarrow as pa
    codec = pa.Codec("snappy")
    for s, e in zip(streams, expected):
        assert codec.decompress(
            s, decompressed_size=len(e)).to_pybytes() == e
    pages = [Page(s, len(e)) for s, e in zip(streams, expected)]
    out, got = launch(shim, "qk_snappy_pages", pages)
    bad = [(n, out[i].tolist()) for i, n in enumerate(names)
           if got[i] != expected[i] or out[i].tolist() !=
           [0, 0, expected[i][0] if expected[i] else -1, 0]]
    assert not bad, "%d of %d pages wrong, first: %s" % (
        len(bad), len(names), bad[:12])


def test_snappy_emitted_elements(gpu):
    """Every literal-length form at its boundaries, copy1 / copy2 / copy4
    at the corners of their length and offset ranges, overlapped copies
    around the 64-lane stride, literal/copy adjacency."""
    cases = C.snappy_valid()
    kinds = {k for c in cases for k in c.kinds}
    assert kinds == {"lit0", "lit1", "lit2", "lit3", "lit4", "copy1",
                     "copy2", "copy4"}
    assert {len(C.varint(len(c.expected))) for c in cases} == {1, 2, 3}
    names = {c.name for c in cases}
    assert {"lit%d" % n for n in C.LITERAL_LENGTHS} <= names
    assert {"copy1-len%d-off%d" % (ln, off) for ln in range(4, 12)
            for off in (1, 2, 255, 256, 2047)} <= names
    assert {"overlap-copy2-len%d-off%d" % (ln, off) for ln in (64, 11, 5)
            for off in C.OVERLAP_OFFSETS} <= names
    check_snappy(gpu, [c.stream for c in cases],
                 [c.expected for c in cases], [c.name for c in cases])


def test_snappy_encoder_streams(gpu):
    """What a real encoder emits for the gzip payload families."""
    import pyarrow as pa
    codec = pa.Codec("snappy")
    P = dict(C.payloads())
    P["maxdist"] = C.gzip_special()["fixed-maxdist"].payload
    P["text-then-random"] = C.gzip_special()["natural-huff-stored"].payload
    names = sorted(P)
    streams = [codec.compress(P[n]).to_pybytes() for n in names]
    check_snappy(gpu, streams, [P[n] for n in names], names)


@pytest.mark.parametrize("case", C.levels_cases(), ids=lambda c: c.name)
def test_snappy_v1_levels(gpu, case):
    """mode 1: the kernel's definition-levels verifier against the host
    mirror parquet_gpu._check_levels_v1 on the same page bytes."""
    from quokka_amd import parquet_gpu as P
    try:
        end = P._check_levels_v1(case.page, 0, case.num_values, 1,
                                 len(case.page))
        host = [end, 0, case.page[end] if end < len(case.page) else -1]
    except P.QkParquetError as e:
        host = [case.data_off, 3 if "nulls" in str(e) else 1, -1]
    assert host == [case.data_off, case.err, case.first], case
    ok = C.levels_page(C.bit_packed([1] * 8), b"\x03ok")
    pages = [Page(C.literal_only(ok), len(ok), 1, 8),
             Page(C.literal_only(case.page), len(case.page), 1,
                  case.num_values),
             Page(C.literal_only(ok), len(ok), 1, 8)]
    out, got = launch(gpu, "qk_snappy_pages", pages)
    assert got == [ok, case.page, ok]
    assert out[1].tolist() == host + [0], (case, out[1].tolist())
    assert out[0].tolist() == out[2].tolist() == [6, 0, 3, 0]


def _snappy_neighbours():
    a = next(c for c in C.snappy_valid() if c.name == "interleaved")
    b = next(c for c in C.snappy_valid() if c.name == "copy1-len7-off255")
    return a, b


def _refuse_snappy(shim, bad):
    a, b = _snappy_neighbours()
    pages = [Page(a.stream, len(a.expected)),
             Page(bad.blob, bad.ulen, 0, src_len=bad.src_len),
             Page(b.stream, len(b.expected))]
    out, got = launch(shim, "qk_snappy_pages", pages)
    assert got[0] == a.expected and got[2] == b.expected
    assert out[0].tolist() == [0, 0, a.expected[0], 0]
    assert out[2].tolist() == [0, 0, b.expected[0], 0]
    return out[1].tolist()


@pytest.mark.parametrize("bad", C.snappy_refused(), ids=lambda r: r.name)
def test_snappy_refused(gpu, bad):
    got = _refuse_snappy(gpu, bad)
    assert got[1] == bad.err, (bad, got)


@pytest.mark.parametrize("name,bad,full", C.snappy_cut_operands(),
                         ids=[c[0] for c in C.snappy_cut_operands()])
def test_snappy_operand_bytes_outside_slice(gpu, name, bad, full):
    """The last element's offset (or literal-length) bytes lie past
    src_len, and the true bytes follow the slice in the buffer as the
    next page's would. Borrowing them makes a cut page decode 'cleanly';
    the kernel must report err 1 instead."""
    import pyarrow as pa
    assert pa.Codec("snappy").decompress(
        bad.blob, decompressed_size=bad.ulen).to_pybytes() == full
    assert bad.src_len < len(bad.blob) and len(full) == bad.ulen
    got = _refuse_snappy(gpu, bad)
    assert got[1] == 1, (bad, got)
