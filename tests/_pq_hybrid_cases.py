"""Inputs for the direct tests of the Parquet value decoders:
qk_pq_rle_pages (RLE/bit-packed hybrid dictionary indices),
qk_pq_def_pages (definition levels -> validity bitmap) and
qk_pq_plain_copy.

Everything here is host-only and deterministic. An emitter writes hybrid
streams from an explicit run layout, so the expected output of a valid
case is the index array the layout was built from, not the output of any
decoder. spec_decode is a decoder written from the Parquet encoding spec
(Encodings.md, "Run Length Encoding / Bit-Packing Hybrid") under the
error rules of include/quokka_amd.h; it is the model of the kernel.
tests/test_pq_hybrid_cases_cpu.py checks emitter, decoder and case lists
against each other and against pyarrow without a GPU;
tests/test_gpu_pq_hybrid.py feeds the same bytes to the kernels.
"""
import functools

import numpy as np

ERR_TRUNC, ERR_INDEX, ERR_DESC = 1, 2, 3          # qk_pq_rle_pages
DEF_PAST, DEF_TRUNC, DEF_LEVEL = 1, 2, 3          # qk_pq_def_pages
V1 = (1 << 64) - 1       # qk_pq_def_pages: v2_levels_len marker of a v1 page
U64 = (1 << 64) - 1


class Guard(bytes):
    """bytes that refuse an index at or past `limit` — the page end."""
    limit = None

    def __getitem__(self, i):
        assert isinstance(i, int) and 0 <= i < self.limit, \
            "read at %r, page ends at %d" % (i, self.limit)
        return bytes.__getitem__(self, i)


def guarded(stream, poison=b"\xAA" * 64):
    """`stream` followed by poison no decoder may touch."""
    g = Guard(bytes(stream) + poison)
    g.limit = len(stream)
    return g


# ---- emitter -------------------------------------------------------------

def varint(x, width=None):
    """ULEB128; `width` pads it with continuation bytes to that length."""
    out = bytearray()
    while True:
        out.append(x & 0x7F)
        x >>= 7
        if not x:
            break
    assert width is None or width >= len(out)
    out += b"\x00" * ((width or len(out)) - len(out))
    for i in range(len(out) - 1):
        out[i] |= 0x80
    return bytes(out)


def emit(layout, bw):
    """Run layout -> (stream bytes, index list).

    ("rle", value, length[, opts]): one RLE run; the value takes
    (bw + 7) // 8 bytes.
    ("packed", values, ngroups[, opts]): one bit-packed run of `ngroups`
    groups of 8; `values` are the ones that count, the rest of the last
    group(s) is padding (opts["pad"], default 0).
    opts: "hdr": header varint width in bytes; "cut": end the run's bytes
    at ceil(len(values) * bw / 8), as older parquet-mr writers end a
    page; "pad": the padding value.
    A zero-length RLE run and a zero-group packed run are legal."""
    out = bytearray()
    idx = []
    for run in layout:
        kind, a, b = run[:3]
        opts = run[3] if len(run) > 3 else {}
        if kind == "rle":
            out += varint(b << 1, opts.get("hdr"))
            out += int(a).to_bytes((bw + 7) // 8, "little")
            idx += [a] * b
        else:
            assert kind == "packed" and len(a) <= b * 8
            out += varint((b << 1) | 1, opts.get("hdr"))
            vals = list(a) + [opts.get("pad", 0)] * (b * 8 - len(a))
            acc = 0
            for i, v in enumerate(vals):
                assert 0 <= v < (1 << bw) or bw == 0
                acc |= v << (i * bw)
            body = acc.to_bytes(b * bw, "little")
            if opts.get("cut"):
                body = body[:(len(a) * bw + 7) // 8]
            out += body
            idx += list(a)
    return bytes(out), idx


# ---- spec decoder --------------------------------------------------------

# the parent kernel's behaviours, for the mutation test: putting any one
# back must make a named case fail
LEGACY = ("unbounded_varint", "no_end_check", "silent_exit",
          "no_range_check")


def spec_decode(src, pos, end, count, bw, dict_n, legacy=()):
    """Decode `count` indices from src[pos:end]. Returns (indices
    written, err): the first error in stream order ends the page; an
    index >= dict_n is written as 0 and its run is still completed.
    `src` is indexed one byte at a time, so a Guard catches any read at
    or past the page end. bw == 0 carries no information: every index is
    0 and the stream is not read."""
    if bw > 32 or pos > end:
        return [], ERR_DESC
    if bw == 0:
        return [0] * count, (ERR_INDEX if count and dict_n == 0 else 0)
    out = []
    mask = (1 << bw) - 1
    while len(out) < count:
        if pos >= end:
            return out, (0 if "silent_exit" in legacy else ERR_TRUNC)
        # header: ULEB128 of at most 10 bytes, all before `end`
        h, nbytes = 0, 0
        while True:
            if "unbounded_varint" not in legacy and \
                    (pos >= end or nbytes == 10):
                return out, ERR_TRUNC
            b = src[pos]
            pos += 1
            h |= (b & 0x7F) << (7 * nbytes)
            nbytes += 1
            if not b & 0x80:
                break
        h &= U64
        left = count - len(out)
        if h & 1:                       # bit-packed: (h >> 1) groups of 8
            ngroups = h >> 1
            n = min(ngroups * 8, left)
            need = (n * bw + 7) // 8    # bytes of the values used
            if need > end - pos and "no_end_check" not in legacy:
                return out, ERR_TRUNC
            vals = []
            for i in range(n):
                bit = i * bw
                nb = ((bit & 7) + bw + 7) // 8
                w = int.from_bytes(
                    bytes(src[pos + (bit >> 3) + k] for k in range(nb)),
                    "little")
                vals.append((w >> (bit & 7)) & mask)
            pos += ngroups * bw
        else:                           # RLE: value in ceil(bw / 8) bytes
            nb = (bw + 7) // 8
            if end - pos < nb and "no_end_check" not in legacy:
                return out, ERR_TRUNC
            val = int.from_bytes(bytes(src[pos + k] for k in range(nb)),
                                 "little")
            pos += nb
            n = min(h >> 1, left)
            vals = [val] * n
        if "no_range_check" in legacy:
            out += vals
            continue
        bad = any(v >= dict_n for v in vals)
        out += [v if v < dict_n else 0 for v in vals]
        if bad:
            return out, ERR_INDEX
    return out, 0


# ---- qk_pq_rle_pages cases -----------------------------------------------

class RleCase:
    """stream: the page's bytes [src_off, src_end); want: the indices
    (before idx_off) the page must write, a prefix of `count` when err is
    set; reverse: hand the kernel src_off > src_end."""
    __slots__ = ("name", "stream", "count", "bw", "dict_n", "idx_off",
                 "want", "err", "reverse")

    def __init__(self, name, stream, count, bw, dict_n, want, err=0,
                 idx_off=0, reverse=False):
        self.name, self.stream, self.count = name, bytes(stream), count
        self.bw, self.dict_n, self.idx_off = bw, dict_n, idx_off
        self.want = np.asarray(want, dtype=np.uint32)
        self.err, self.reverse = err, reverse

    def __repr__(self):
        return "RleCase(%s)" % self.name


def _valid(name, layout, bw, count=None, dict_n=None, idx_off=0):
    stream, idx = emit(layout, bw)
    count = len(idx) if count is None else count
    assert count <= len(idx)
    return RleCase(name, stream, count, bw,
                   (1 << bw) if dict_n is None else dict_n, idx[:count],
                   idx_off=idx_off)


def _pattern(bw, n, rng):
    """n values of width bw: 0, all ones, both alternating patterns, then
    random ones; the last is all ones again."""
    m = (1 << bw) - 1
    v = [0, m, 0x55555555 & m, 0xAAAAAAAA & m]
    v += [int(x) for x in rng.integers(0, m + 1, n - 5)] + [m]
    return v[:n]


RLE_ONES_BW = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32)
RLE_ONES_LEN = (1, 7, 8, 63, 64, 65, 129, 20_000)
MIXED_LENGTHS = (1, 8, 3, 16, 61, 72, 2, 64, 5)     # rle, packed, rle, ...


@functools.lru_cache(maxsize=None)
def rle_bitwidth_cases():
    """Every bw in 1..32: one packed run of 3 groups, count 24 and 17."""
    rng = np.random.default_rng(3201)
    out = []
    for bw in range(1, 33):
        for count in (24, 17):
            out.append(_valid("bw%d-count%d" % (bw, count),
                              [("packed", _pattern(bw, 24, rng), 3)], bw,
                              count=count))
    return tuple(out)


def _mixed(bw, rng, lengths=MIXED_LENGTHS, first="rle"):
    m = (1 << bw) - 1
    layout = []
    packed = first == "packed"
    for ln in lengths:
        if packed and ln % 8 == 0:
            layout.append(("packed", _pattern(bw, ln, rng), ln // 8))
        else:
            layout.append(("rle", int(rng.integers(0, m + 1)), ln))
        packed = not packed
    return layout


@functools.lru_cache(maxsize=None)
def rle_valid_cases():
    rng = np.random.default_rng(3202)
    out = []
    for bw in RLE_ONES_BW:
        for ln in RLE_ONES_LEN:
            c = _valid("ones-bw%d-len%d" % (bw, ln),
                       [("rle", (1 << bw) - 1, ln)], bw)
            # 20,000 << 1 needs a 3-byte header
            assert (ln == 20_000) == (len(c.stream) == 3 + (bw + 7) // 8)
            out.append(c)
    for ngroups, hdr, hlen in ((64, None, 2), (2049, None, 2),
                               (2049, 3, 3), (8192, None, 3)):
        bw = 5 if ngroups < 8192 else 2
        vals = [int(x) for x in rng.integers(0, 1 << bw, ngroups * 8)]
        c = _valid("packed-%dgroups-hdr%d" % (ngroups, hlen),
                   [("packed", vals, ngroups, {"hdr": hdr})], bw)
        assert len(c.stream) == hlen + ngroups * bw
        out.append(c)
    for bw in (1, 3, 12, 20, 32):
        out.append(_valid("mixed-bw%d" % bw, _mixed(bw, rng), bw))
        # the same lengths rotated, packed first: other lane offsets
        rot = MIXED_LENGTHS[1:] + MIXED_LENGTHS[:1]
        out.append(_valid("mixed-rot-bw%d" % bw,
                          _mixed(bw, rng, rot, first="packed"), bw))
    out.append(_valid("padded-headers", [
        ("rle", 5, 9, {"hdr": 2}), ("packed", [1, 2, 3, 4, 5, 6, 7, 0], 1,
                                    {"hdr": 3}),
        ("rle", 6, 70, {"hdr": 3})], 3))
    out.append(_valid("header-10-bytes", [("rle", 6, 20, {"hdr": 10}),
                                          ("rle", 1, 4)], 3))
    out.append(_valid("zero-runs-in-the-middle", [
        ("rle", 3, 10), ("rle", 7, 0), ("packed", [], 0),
        ("packed", [1, 0, 7, 6, 5, 4, 3, 2], 1), ("packed", [], 0, {"hdr": 2}),
        ("rle", 0, 0, {"hdr": 3}), ("rle", 2, 11)], 3))
    out.append(_valid("last-rle-100-count-37",
                      [("packed", _pattern(6, 8, rng), 1), ("rle", 33, 100)],
                      6, count=37))
    for cut in (False, True):
        vals = _pattern(11, 33, rng)
        c = _valid("last-packed-5groups-count-33-%s"
                   % ("cut" if cut else "padded"),
                   [("packed", vals, 5, {"cut": cut})], 11)
        assert len(c.stream) == 1 + (46 if cut else 55) and c.count == 33
        out.append(c)
    out.append(RleCase("bw0-no-stream", b"", 10, 0, 1, [0] * 10))
    out.append(RleCase("bw0-with-stream", varint(10 << 1), 10, 0, 1,
                       [0] * 10))
    out.append(RleCase("count0-no-stream", b"", 0, 4, 16, []))
    out.append(_valid("count0-with-stream", [("rle", 3, 5)], 4, count=0))
    for idx_off, dict_n in ((0, 200), (7, 200), (1 << 31, 1 << 20)):
        bw = 8 if dict_n == 200 else 20
        layout = [("rle", dict_n - 1, 3),
                  ("packed", [dict_n - 1, 0, 1, dict_n - 2, 5, 6, 7, 8], 1),
                  ("rle", 0, 70)]
        out.append(_valid("idx_off-%d" % idx_off, layout, bw, dict_n=dict_n,
                          idx_off=idx_off))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rle_corrupt_cases():
    """(case with the error code written down by hand); `want` is the
    prefix the spec decoder writes before it stops."""
    def bad(name, stream, count, bw, dict_n, err, **kw):
        want, got = spec_decode(guarded(stream), 0, len(stream), count, bw,
                                dict_n)
        if kw.get("reverse"):
            want, got = [], ERR_DESC
        assert got == err, (name, got, err)
        return RleCase(name, stream, count, bw, dict_n, want, err, **kw)

    ten = emit([("rle", 4, 10)], 3)[0]
    pad_vals = [1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]        # 11 used of 16
    return (
        bad("varint-continues-on-last-byte", ten + b"\x83", 20, 3, 8,
            ERR_TRUNC),
        # a run of 5 whose header is padded to 11 bytes: a decoder that
        # takes any length of varint decodes the page
        bad("varint-11-bytes", varint(5 << 1, 11) + b"\x03", 5, 3, 8,
            ERR_TRUNC),
        bad("rle-value-byte-missing-bw17",
            emit([("rle", 0x1FFFF, 9)], 17)[0][:-1], 9, 17, 1 << 17,
            ERR_TRUNC),
        bad("rle-value-byte-missing-bw25",
            emit([("rle", 0x1FFFFFF, 9)], 25)[0][:-1], 9, 25, 1 << 25,
            ERR_TRUNC),
        bad("packed-used-values-past-end",
            emit([("packed", list(range(24)), 3)], 5)[0][:10], 24, 5, 32,
            ERR_TRUNC),
        bad("empty-stream", b"", 5, 3, 8, ERR_TRUNC),
        bad("covers-10-of-50", ten, 50, 3, 8, ERR_TRUNC),
        bad("twenty-zero-length-runs", emit([("rle", 1, 0)] * 20, 3)[0], 50,
            3, 8, ERR_TRUNC),
        bad("rle-index-at-dict_n", emit([("rle", 2, 4), ("rle", 5, 6),
                                         ("rle", 1, 3)], 3)[0], 13, 3, 5,
            ERR_INDEX),
        bad("packed-index-above-dict_n",
            emit([("rle", 2, 4), ("packed", [0, 1, 2, 3, 4, 7, 0, 1], 1),
                  ("rle", 1, 3)], 3)[0], 15, 3, 5, ERR_INDEX),
        # 7 >= dict_n only in the padding of the clipped last group
        bad("out-of-range-only-in-padding",
            emit([("packed", pad_vals, 2, {"pad": 7})], 3)[0], 11, 3, 5, 0),
        bad("bw33", ten, 10, 33, 8, ERR_DESC),
        bad("src_off-above-src_end", ten, 10, 3, 8, ERR_DESC, reverse=True),
    )


# ---- qk_pq_def_pages -----------------------------------------------------

def sim_def_pages(src, descs, valid_words, drop_partial=False):
    """qk_pq_def_pages, lane by lane semantics folded into row loops.
    valid_words: np.uint64 bitmap, pre-zeroed, OR-ed into. Returns the
    npages x 4 result table. The kernel writes a word once the page's
    runs have passed its last row and gives up the word it is gathering
    when the page ends in an error; drop_partial=True models that (the
    bits of an erroring page at or above the last 64-row boundary its
    runs reached are not written), the default keeps every bit decoded
    before the error."""
    out = np.zeros((len(descs), 4), dtype=np.int64)
    words = {}
    for pg, (pos, page_end, v2len, row0, nrows, _) in enumerate(
            np.asarray(descs, dtype=np.uint64).tolist()):
        err = 0
        if v2len == V1:
            if pos > page_end or page_end - pos < 4:
                err, end = DEF_PAST, pos
            else:
                ln = int.from_bytes(bytes(src[pos + i] for i in range(4)),
                                    "little")
                pos += 4
                end = pos + ln
                if end > page_end:
                    err = DEF_PAST
        else:
            end = pos + v2len
            if pos > page_end or v2len > page_end - pos:
                err = DEF_PAST
        row, remaining, nonnull = row0, nrows, 0
        mine = {}
        steps = 0
        while not err and remaining and pos < end:
            steps += 1
            assert steps <= end, "run loop does not advance"
            h, shift, npos, bad = 0, 0, pos, DEF_TRUNC
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
                    bad = DEF_TRUNC
                else:
                    val = src[npos]
                    npos += 1
                    if val > 1:
                        bad = DEF_LEVEL
            if bad:
                err = bad
                break
            if h & 1:
                ngroups = h >> 1
                if ngroups > end - npos:
                    err = DEF_TRUNC
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
                    mine[r >> 6] = mine.get(r >> 6, 0) | (1 << (r & 63))
                    nonnull += 1
            row += n
            remaining -= n
            pos = npos
        if not err and remaining:
            err = DEF_TRUNC
        if err and drop_partial:
            mine.pop(row >> 6, None)    # rows below `row` are decoded
        for w, bits in mine.items():
            words[w] = words.get(w, 0) | bits
        first = src[end] if not err and end < page_end else -1
        out[pg] = (nonnull, end, err, first)
    for w, bits in words.items():
        valid_words[w] |= np.uint64(bits)
    return out


def v1(levels):
    return len(levels).to_bytes(4, "little") + levels


class DefCase:
    """One page made of `block` alone (page_len defaults to its length).
    v2len None: a v1 block with its own length prefix. res3: the first
    three result fields [non_null, values_off, err] where the case pins
    them all; words: the bitmap words it pins; clean: the bitmap must
    stay zero."""
    __slots__ = ("name", "block", "nrows", "v2len", "page_len", "err",
                 "res3", "words", "clean")

    def __init__(self, name, block, nrows, err, v2len=None, page_len=None,
                 res3=None, words=None, clean=False):
        self.name, self.block, self.nrows = name, bytes(block), nrows
        self.v2len, self.err = v2len, err
        self.page_len = len(self.block) if page_len is None else page_len
        self.res3, self.words, self.clean = res3, words, clean

    def __repr__(self):
        return "DefCase(%s)" % self.name


@functools.lru_cache(maxsize=None)
def def_cases():
    vi = varint
    return (
        # ---- good blocks
        DefCase("rle-100-ones", v1(vi(100 << 1) + b"\x01"), 100, 0,
                res3=[100, 7, 0], words=[(1 << 64) - 1, (1 << 36) - 1]),
        DefCase("packed-2-groups-13-rows",
                v1(bytes([(2 << 1) | 1, 0b10110101, 0xFF])), 13, 0,
                res3=[10, 7, 0], words=[0b1111110110101]),
        DefCase("v2-no-prefix", bytes([7 << 1, 0]), 7, 0, v2len=2,
                res3=[0, 2, 0]),
        DefCase("rows-64", v1(vi(64 << 1) + b"\x01"), 64, 0,
                res3=[64, 7, 0], words=[(1 << 64) - 1]),
        DefCase("mixed-runs",
                v1(vi(3 << 1) + b"\x01" + bytes([(1 << 1) | 1, 0x5A])
                   + vi(70 << 1) + b"\x00" + vi(9 << 1) + b"\x01"), 90, 0,
                res3=[3 + 4 + 9, 13, 0]),
        # ---- truncated
        # varint continuation bit set on the block's last byte
        DefCase("varint-continues-on-last-byte", v1(bytes([0x80])), 50,
                DEF_TRUNC),
        # RLE header without its value byte
        DefCase("rle-without-value-byte", v1(bytes([50 << 1])), 50,
                DEF_TRUNC),
        # bit-packed header that claims more groups than the block holds
        DefCase("packed-groups-past-block",
                v1(bytes([(9 << 1) | 1, 0xFF, 0xFF])), 50, DEF_TRUNC),
        # the stream ends before the page's rows are covered
        DefCase("covers-10-of-50", v1(bytes([10 << 1, 1])), 50, DEF_TRUNC),
        # zero-length runs advance and end, they cannot spin
        DefCase("twenty-zero-length-runs", v1(bytes([0, 1] * 20)), 50,
                DEF_TRUNC),
        # whole bitmap words are done before the stream runs out
        DefCase("covers-150-of-200", v1(vi(150 << 1) + b"\x01"), 200,
                DEF_TRUNC, res3=[150, 7, DEF_TRUNC]),
        # ---- length prefix past the page end
        DefCase("prefix-past-page",
                (1000).to_bytes(4, "little") + vi(100 << 1) + b"\x01", 100,
                DEF_PAST, clean=True),
        # a page too short for the prefix itself
        DefCase("page-shorter-than-prefix", b"\x02\x00", 10, DEF_PAST),
        # v2 length from the header past the page
        DefCase("v2-length-past-page", bytes([7 << 1, 1]), 7, DEF_PAST,
                v2len=40),
        # ---- a level above 1
        DefCase("level-2", v1(vi(100 << 1) + b"\x02"), 100, DEF_LEVEL),
    )


def valid_words(n):
    """u64 words of a validity bitmap of n rows (ops.valid_nbytes / 8)."""
    return ((n + 63) // 64 * 8 + 8) // 8


# ---- qk_pq_plain_copy ----------------------------------------------------

PLAIN_ELEM_SIZES = (1, 2, 4, 8)
PLAIN_SRC_OFFSETS = tuple(range(8))
PLAIN_TILE_COUNTS = (0, 1, 255, 256, 257, 8192)


def plain_cases():
    """(elem_size, [(src_byte_off mod 8, count), ...]): every tile count
    at every source alignment."""
    return tuple((es, tuple((a, cnt) for cnt in PLAIN_TILE_COUNTS
                            for a in PLAIN_SRC_OFFSETS))
                 for es in PLAIN_ELEM_SIZES)


# ---- hand-written column chunks and corrupted files ----------------------

def _zz(n):
    """Thrift compact zigzag varint."""
    return varint(n << 1)


def data_page(num_values, encoding, body):
    """v1 DATA_PAGE: PageHeader{1: type 0, 2: uncompressed, 3: compressed,
    5: DataPageHeader{1: num_values, 2: encoding, 3: RLE, 4: RLE}}."""
    return (b"\x15" + _zz(0) + b"\x15" + _zz(len(body)) + b"\x15"
            + _zz(len(body)) + b"\x2c" + b"\x15" + _zz(num_values)
            + b"\x15" + _zz(encoding) + b"\x15" + _zz(3) + b"\x15" + _zz(3)
            + b"\x00\x00" + body)


def dict_page(num_values, body):
    """DICTIONARY_PAGE: PageHeader{1: type 2, 2, 3: sizes,
    7: DictionaryPageHeader{1: num_values, 2: PLAIN}}."""
    return (b"\x15" + _zz(2) + b"\x15" + _zz(len(body)) + b"\x15"
            + _zz(len(body)) + b"\x4c" + b"\x15" + _zz(num_values)
            + b"\x15" + _zz(0) + b"\x00\x00" + body)


def chunk(pages, num_values, physical_type="INT64", has_dict=False):
    """Uncompressed required-column chunk made of `pages` -> (raw file
    bytes, column-chunk metadata as _Chunk reads it)."""
    import types
    lead = b"PAR1" + b"\x00" * 3
    body = b"".join(pages)
    raw = lead + body + b"\x00" * 16
    col = types.SimpleNamespace(
        compression="UNCOMPRESSED", physical_type=physical_type,
        data_page_offset=len(lead) + (len(pages[0]) if has_dict else 0),
        dictionary_page_offset=len(lead) if has_dict else None,
        total_compressed_size=len(body), num_values=num_values)
    return raw, col


def five_value_file(version, nullable=False):
    """A small dictionary file written by pyarrow: 5 distinct int64
    values, uncompressed, one row group. -> (raw bytes, table)."""
    import io
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(55)
    vals = (rng.integers(0, 5, 1000) + 1) * 1000
    if nullable:
        arr = pa.array(vals, mask=rng.random(1000) < 0.2, type=pa.int64())
        t = pa.table({"x": arr})
    else:
        t = pa.table({"x": pa.array(vals, type=pa.int64())}).cast(
            pa.schema([pa.field("x", pa.int64(), nullable=False)]))
    buf = io.BytesIO()
    pq.write_table(t, buf, compression="NONE", data_page_version=version,
                   use_dictionary=True)
    return buf.getvalue(), t


def locate_rle_pages(raw, mask):
    """_Chunk plan of the file's one column chunk with rle_pages filled;
    in mask mode through the simulated definition-level pass."""
    import io
    import pyarrow.parquet as pq
    from quokka_amd import parquet_gpu as P
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    max_def = md.schema.column(0).max_definition_level
    ch = P._Chunk(raw, md.row_group(0).column(0), max_def, 0, mask)
    if mask:
        words = np.zeros(valid_words(md.num_rows), dtype=np.uint64)
        P._dense_plan([ch], sim_def_pages(raw, P._def_descs([ch]), words))
    return ch


def corrupt_first_index(raw, stream_off, bw):
    """Overwrite the first run's value bits so that its first index is
    2**bw - 1. Returns the patched file bytes."""
    out = bytearray(raw)
    pos, h, shift = stream_off, 0, 0
    while True:
        b = raw[pos]
        pos += 1
        h |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    assert h >> 1, "empty first run"
    out[pos] |= (1 << bw) - 1 if bw < 8 else 0xFF
    assert bw <= 8
    return bytes(out)
